"""GpuProver.prove_minimal_record / prove_minimal_records (ss_p_decommit_minimal, ss_p_minimal_pack_dev): the proof as the
minimal record, planned and gathered by the GPU, against the set-based definition applied to the numpy prover's proof --
word for word, nothing written behind the record."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import stwo_prover  # noqa: E402

import stark_symphony_amd as ss  # noqa: E402
from stark_symphony_amd import formats, verifier  # noqa: E402

pytestmark = pytest.mark.gpu
SMALL = dict(n_cols=4, trace_log=5, log_blowup=1, n_queries=4, pow_bits=5)
PROOF_JSON = dict(n_cols=4, trace_log=9, log_blowup=4, n_queries=16, pow_bits=5)
FILL = 0x5A5A5A5A


@pytest.fixture(scope="module")
def gp():
    from stark_symphony_amd import prover
    return prover.GpuProver(verifier.Verifier(0))


def reference(seed, **kw):
    return verifier.stwo_minimal_record(formats.stwo_minimise(ss.stwo_from_json(stwo_prover.prove(seed=seed, **kw))))


# seeds 0 and 1 of every configuration; the Q = 64 one (both seeds) has a repeated position, two queried siblings and
# lists of length 0, the 65-column one at seed 0 as well (checked with the numpy prover)
@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("kw,transcript", [
    (dict(n_cols=4, trace_log=3, log_blowup=1, n_queries=1, pow_bits=5), "host"),   # proof_test.json: one query, every node lone
    (dict(n_cols=3, trace_log=1, log_blowup=2, n_queries=3, pow_bits=1), "host"),   # K = 0, trees of 1-3 levels, one pair level
    (PROOF_JSON, "host"),                                                           # proof.json
    (dict(n_cols=20, trace_log=4, log_blowup=2, n_queries=64, pow_bits=3, hash="blake2s"), "host"),  # Q = 64 = positions
    (dict(n_cols=65, trace_log=2, log_blowup=1, n_queries=5, pow_bits=1), "host"),  # > 64 columns: the strided value gather
    (PROOF_JSON, "device"),
])
def test_minimal_record_equals_the_definition(gp, kw, transcript, seed):
    want = reference(seed, **kw)
    cs = verifier.stwo_cfg_struct(gp.config(**kw), verifier.MODE_FIXTURE)
    max_words = gp.lib.ss_stwo_minimal_max_words(cs)
    out = gp.torch.full((max_words,), FILL, dtype=gp.torch.int32, device=gp.dev)  # a word written behind the record shows
    words = gp.torch.zeros(1, dtype=gp.torch.int32, device=gp.dev)
    got = gp.prove_minimal_record(out=out, words_out=words, transcript=transcript, seed=seed, **kw)
    host = out.cpu().numpy().view(np.uint32)
    assert int(words.item()) == want.size == got.numel() and got.data_ptr() == out.data_ptr()
    assert np.array_equal(host[:want.size], want)
    assert (host[want.size:] == FILL).all()


def test_packed_batch_round_trip(gp):
    records, offs = gp.prove_minimal_records(seeds=range(6), workers=3, **SMALL)
    o = offs.cpu().numpy()
    assert o[0] == 0 and o[6] == records.numel()
    host = records.cpu().numpy()
    for i in range(6):
        assert np.array_equal(host[o[i]:o[i + 1]], gp.prove_minimal_record(seed=i, **SMALL).cpu().numpy()), i
    cfg = gp.config(**SMALL)
    batch = verifier.StwoMinimalDeviceBatch(gp.ver, cfg, verifier.MODE_FIXTURE, (records, offs))
    batch.run()
    assert batch.status().tolist() == [0] * 6
    # one bit of record 2's first trace sibling: behind the fixed words, the values and the fold partners
    K, fixed = cfg.n_layers, 24 + 4 * (cfg.n_cols + 16) + 8 * (cfg.n_layers + 1) + 6
    counts = host[o[2] + fixed:o[2] + fixed + 2 * K + 6].view(np.uint32)
    assert counts[3 + K] > 0
    bad = records.clone()
    bad[int(o[2]) + fixed + 2 * K + 6 + int(counts[0]) * (cfg.n_cols + 16) + 4 * int(counts[2:3 + K].sum()) + 3] ^= 1 << 7
    batch = verifier.StwoMinimalDeviceBatch(gp.ver, cfg, verifier.MODE_FIXTURE, (bad, offs))
    batch.run()
    bad_host = bad.cpu().numpy().view(np.uint32)
    want = gp.ver.verify_stwo_minimal_records(cfg, [bad_host[o[i]:o[i + 1]] for i in range(6)])
    assert batch.status().tolist() == want.tolist() and want[2] != 0 and not want[[0, 1, 3, 4, 5]].any()


def test_span_fallback(gp):
    seed = next(s for s in range(8) if ss.stwo_from_json(stwo_prover.prove(seed=s, **SMALL)).pow_nonce > 0)
    got = gp.prove_minimal_record(seed=seed, pow_span=1, **SMALL)
    assert np.array_equal(got.cpu().numpy().view(np.uint32), reference(seed, **SMALL))
