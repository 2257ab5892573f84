"""GpuProver.prove_record / prove_records (ss_p_finish_dev + ss_p_decommit_record): the proof as the verifier's
per-query record, written by the GPU, against the record of the numpy prover's proof -- word for word."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import stwo_prover  # noqa: E402

import stark_symphony_amd as ss  # noqa: E402
from stark_symphony_amd import verifier  # noqa: E402

pytestmark = pytest.mark.gpu
SMALL = dict(n_cols=4, trace_log=5, log_blowup=1, n_queries=1, pow_bits=5)


@pytest.fixture(scope="module")
def gp():
    from stark_symphony_amd import prover
    return prover.GpuProver(verifier.Verifier(0))


@pytest.fixture(scope="module")
def rows(gp):
    return gp.prove_records(seeds=range(6), workers=3, **SMALL)


@pytest.mark.parametrize("kw,min_nonce", [
    (dict(n_cols=3, trace_log=1, log_blowup=2, n_queries=3, pow_bits=1), 0),   # two rows: chains of 1 or 2 levels
    (dict(n_cols=4, trace_log=3, log_blowup=1, n_queries=1, pow_bits=5), 0),   # proof_test.json: one query
    (dict(n_cols=4, trace_log=9, log_blowup=4, n_queries=16, pow_bits=5), 0),  # proof.json
    (dict(n_cols=20, trace_log=4, log_blowup=2, n_queries=64, pow_bits=3, hash="blake2s"), 0),  # N > 16, Q = 64 = positions
    (dict(n_cols=5, trace_log=12, log_blowup=2, n_queries=11, pow_bits=10, hash="blake2s"), 256),  # nonce past one round
])
def test_record_equals_the_numpy_provers(gp, kw, min_nonce):
    for seed in range(8):
        proof = ss.stwo_from_json(stwo_prover.prove(seed=seed, **kw))
        if proof.pow_nonce >= min_nonce:
            break
    assert proof.pow_nonce >= min_nonce
    want = verifier.stwo_record(proof)
    out = gp.torch.full((want.size,), 0x5A5A5A5A, dtype=gp.torch.int32, device=gp.dev)  # an unwritten word shows
    got = gp.prove_record(out=out, seed=seed, **kw)
    assert got is out and np.array_equal(got.cpu().numpy().view(np.uint32), want)


def test_rows_are_the_single_records(gp, rows):
    host = rows.cpu().numpy()
    for i in range(6):
        assert np.array_equal(host[i], gp.prove_record(seed=i, **SMALL).cpu().numpy()), i
    assert len({host[i].tobytes() for i in range(6)}) == 6


def test_resident_round_trip(gp, rows):
    cfg = gp.config(**SMALL)
    batch = verifier.StwoDeviceBatch(gp.ver, cfg, verifier.MODE_FIXTURE, rows)
    batch.run()
    assert batch.status().tolist() == [0] * 6
    bad = rows.clone()
    bad[2, 24 + 4 * (cfg.n_cols + 16) + 8 * (cfg.n_layers + 1) + 6 + cfg.n_cols + 16 + 8 + 3] ^= 1 << 7  # trace path, sibling 1, word 3
    batch = verifier.StwoDeviceBatch(gp.ver, cfg, verifier.MODE_FIXTURE, bad)
    batch.run()
    want = gp.ver.verify_stwo_records(cfg, bad.cpu().numpy().view(np.uint32))
    assert batch.status().tolist() == want.tolist() and want[2] != 0 and not want[[0, 1, 3, 4, 5]].any()


def test_span_fallback(gp):
    refs = [ss.stwo_from_json(stwo_prover.prove(seed=s, **SMALL)) for s in range(8)]
    seed = next((s for s, p in enumerate(refs) if p.pow_nonce > 0), None)
    assert seed is not None
    got = gp.prove_record(seed=seed, pow_span=1, **SMALL)
    assert np.array_equal(got.cpu().numpy().view(np.uint32), verifier.stwo_record(refs[seed]))
