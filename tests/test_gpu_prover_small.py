"""GpuProver.prove_records(one_launch=True) / ss_p_prove_small_dev (include/ss_prover_small.h): a batch of small proofs in one
launch, one workgroup per proof, against the record of the numpy prover's proof -- word for word, on rows pre-filled with a
pattern and with one guard row behind the batch."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import stwo_prover  # noqa: E402

import stark_symphony_amd as ss  # noqa: E402
from stark_symphony_amd import binding, prover, verifier  # noqa: E402

pytestmark = pytest.mark.gpu
FILL, ERR_POW_SPAN = 0x5A5A5A5A, 2
TEST_JSON = dict(n_cols=4, trace_log=3, log_blowup=1, n_queries=1, pow_bits=5)
# (shape, smallest nonce the first seed must have)
CASES = [
    (dict(n_cols=3, trace_log=1, log_blowup=2, n_queries=3, pow_bits=1), 0),   # two rows: constant partitions, chains of 1 or 2 levels
    (TEST_JSON, 0),                                                            # proof_test.json: one query, trees in registers only
    (dict(n_cols=4, trace_log=9, log_blowup=4, n_queries=16, pow_bits=5), 0),  # proof.json: the limit shape
    (dict(n_cols=20, trace_log=4, log_blowup=2, n_queries=64, pow_bits=3, hash="blake2s"), 0),  # two-block leaves, Q = all positions
    (dict(n_cols=5, trace_log=7, log_blowup=2, n_queries=11, pow_bits=8, hash="blake2s"), 512),  # a nonce past the first round
]


@pytest.fixture(scope="module")
def gp():
    return prover.GpuProver(verifier.Verifier(0))


@functools.lru_cache(maxsize=None)
def reference(case, count=3):
    """-> (seeds, the numpy prover's records of them): `count` consecutive seeds, the first with a nonce >= the case's bound"""
    kw, min_nonce = CASES[case]
    proofs = {}
    for first in range(64):
        proofs[first] = ss.stwo_from_json(stwo_prover.prove(seed=first, **kw))
        if proofs[first].pow_nonce >= min_nonce:
            break
    assert proofs[first].pow_nonce >= min_nonce
    seeds = list(range(first, first + count))
    return seeds, np.stack([verifier.stwo_record(proofs.get(s) or ss.stwo_from_json(stwo_prover.prove(seed=s, **kw))) for s in seeds])


def launch(gp, kw, seeds, n_groups=0, pow_span=None):
    """the C entry on rows (and error words) filled with a pattern, a guard row behind them -> (rows, error words) on the host"""
    cs = verifier.stwo_cfg_struct(gp.config(**kw), verifier.MODE_FIXTURE)
    words, n = gp.lib.ss_stwo_record_words(C.byref(cs)), len(seeds)
    rows = gp.torch.full((n + 1, words), FILL, dtype=gp.torch.int32, device=gp.dev)
    err = gp.torch.full((n + 1,), FILL, dtype=gp.torch.int32, device=gp.dev)
    groups = n_groups or n
    arena = gp._empty(gp.lib.ss_p_small_arena_words(C.byref(cs), groups))
    n_log, l_log = kw["trace_log"], kw["trace_log"] + kw["log_blowup"]
    (_, itw_n, _), (tw_c, itw_c, hxhy_c), (tw_l, itw_l, hxhy_l) = gp.domain(n_log), gp.domain(n_log + 1), gp.domain(l_log)
    tables = prover.SmallTables(*[x.data_ptr() for x in (itw_n, tw_c, itw_c, hxhy_c, tw_l, itw_l, hxhy_l)])
    root = (C.c_uint32 * 8)(*np.frombuffer(prover.HASHES[kw.get("hash", "sha256")](b"").digest(), dtype=">u4"))
    seeds_dev = gp.torch.tensor(list(seeds) + [0], dtype=gp.torch.int64, device=gp.dev)
    rc = gp.lib.ss_p_prove_small_dev(gp.ver.ctx, C.byref(cs), cs.pow_target, pow_span or 1 << (kw["pow_bits"] + 8), seeds_dev.data_ptr(),
                                     n, n_groups, C.byref(tables), root, arena.data_ptr(), arena.numel(), rows.data_ptr(), words,
                                     err.data_ptr(), gp._stream())
    gp.torch.cuda.synchronize(gp.dev)
    host = rows.cpu().numpy().view(np.uint32)
    assert (host[n] == FILL).all() and int(err[n].cpu()) == FILL  # the guard row, the guard word
    return rc, host[:n], err[:n].cpu().numpy()


@pytest.mark.parametrize("case", range(len(CASES)))
def test_rows_equal_the_numpy_provers(gp, case):
    seeds, want = reference(case)
    rc, got, err = launch(gp, CASES[case][0], seeds)
    assert rc == 0 and not err.any() and np.array_equal(got, want)
    assert np.array_equal(gp.prove_records(seeds, one_launch=True, **CASES[case][0]).cpu().numpy().view(np.uint32), want)


def test_two_columns_have_no_constraint(gp):
    """n_cols = 2: trace_row stores its second column and never enters its recurrence, and composition_point reads two
    columns and sums no constraint (the composition polynomial is zero).  The one-launch rows against the launch chain
    of prove_record on the device transcript, which calls the same steps from its grid kernels, and against the numpy prover."""
    kw = dict(n_cols=2, trace_log=2, log_blowup=1, n_queries=2, pow_bits=1)
    seeds = [0, 1, 2]
    want = np.stack([verifier.stwo_record(ss.stwo_from_json(stwo_prover.prove(seed=s, **kw))) for s in seeds])
    rc, got, err = launch(gp, kw, seeds)
    assert rc == 0 and not err.any() and np.array_equal(got, want)
    for i, s in enumerate(seeds):
        assert np.array_equal(got[i], gp.prove_record(seed=s, transcript="device", **kw).cpu().numpy().view(np.uint32)), s


def test_a_slot_is_reused_from_proof_to_proof(gp):
    rc, got, err = launch(gp, TEST_JSON, range(5), n_groups=2)
    assert rc == 0 and not err.any() and len({r.tobytes() for r in got}) == 5
    for i in range(5):
        assert np.array_equal(got[i], gp.prove_record(seed=i, transcript="device", **TEST_JSON).cpu().numpy().view(np.uint32)), i


def test_resident_round_trip(gp):
    seeds, _ = reference(2)
    kw = CASES[2][0]
    cfg, rows = gp.config(**kw), gp.prove_records(seeds, one_launch=True, **kw)
    batch = verifier.StwoDeviceBatch(gp.ver, cfg, verifier.MODE_FIXTURE, rows)
    batch.run()
    assert batch.status().tolist() == [0, 0, 0]
    bad = rows.clone()
    bad[1, 24 + 4 * (cfg.n_cols + 16) + 8 * (cfg.n_layers + 1) + 6 + cfg.n_cols + 16 + 8 + 3] ^= 1 << 7  # trace path, sibling 1, word 3
    batch = verifier.StwoDeviceBatch(gp.ver, cfg, verifier.MODE_FIXTURE, bad)
    batch.run()
    status = batch.status().tolist()
    assert status[1] != 0 and status[0] == status[2] == 0


def test_a_nonce_outside_the_span_is_flagged_and_redone(gp):
    kw = CASES[0][0]  # one bit of work: every other seed's nonce is 0
    nonce = {s: ss.stwo_from_json(stwo_prover.prove(seed=s, **kw)).pow_nonce for s in range(16)}
    seeds = [s for s in nonce if nonce[s] == 0][:2]
    seeds.insert(1, next(s for s in nonce if nonce[s] > 0))
    rc, _, err = launch(gp, kw, seeds, pow_span=1)
    assert rc == 0 and err.tolist() == [0, ERR_POW_SPAN, 0]
    got = gp.prove_records(seeds, one_launch=True, pow_span=1, **kw).cpu().numpy().view(np.uint32)
    want = np.stack([verifier.stwo_record(ss.stwo_from_json(stwo_prover.prove(seed=s, **kw))) for s in seeds])
    assert gp.small_errors.tolist() == [0, ERR_POW_SPAN, 0] and np.array_equal(got, want)


@pytest.mark.parametrize("kw,seeds", [
    (dict(TEST_JSON, log_blowup=11), [0]),  # lde_log one above the limit
    (dict(TEST_JSON, n_cols=33), [0]),
    (TEST_JSON, []),
], ids=["lde_log", "n_cols", "no_seeds"])
def test_refused_shapes(gp, kw, seeds):
    assert gp.small_limits() == (13, 32, 64)
    cs = verifier.stwo_cfg_struct(gp.config(**kw), verifier.MODE_FIXTURE)
    buf = gp.torch.full((4096,), FILL, dtype=gp.torch.int32, device=gp.dev)  # stands for every device argument: nothing is launched
    tables = prover.SmallTables(*[buf.data_ptr()] * 7)
    rc = gp.lib.ss_p_prove_small_dev(gp.ver.ctx, C.byref(cs), cs.pow_target, 1 << 13, buf.data_ptr(), len(seeds), 0, C.byref(tables),
                                     (C.c_uint32 * 8)(), buf.data_ptr(), 1 << 40, buf.data_ptr(), 1 << 30, buf.data_ptr(), gp._stream())
    gp.torch.cuda.synchronize(gp.dev)
    assert rc == binding.SS_ERR_ARG and bool((buf == FILL).all())
    with pytest.raises(ValueError):
        gp.prove_records(seeds, one_launch=True, **kw)
