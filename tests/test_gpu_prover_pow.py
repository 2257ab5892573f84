"""ss_p_finish_grid_dev (include/ss_prover_pow.h): the end of the transcript with the proof of work ground by a grid of
workgroups.  The kernel alone against a hashlib loop from nonce 0 and the Python channel, word for word; its span edges,
its self-cleaning work words, the arguments it refuses; records made with grid_pow=True against the numpy prover's.
A nonce at or above 2^32 cannot be reached in a test of seconds: the path of the nonce's high word (fixed within a chunk,
hashed once per chunk) is covered by reading csrc/ss_prover_pow.hip only."""
import functools
import hashlib
import os
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (before the library is loaded: it must bind the HIP runtime torch ships, binding.process_defaults)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import stwo_prover  # noqa: E402

import stark_symphony_amd as ss  # noqa: E402
from stark_symphony_amd import binding, formats, prover, verifier  # noqa: E402

pytestmark = pytest.mark.gpu
FILL = 0x5A5A5A5A
L, Q, LAST = 13, 11, (5, 6, 7, 8)  # 11 queries: two draws, the second cut short
STATE = np.frombuffer(hashlib.sha256(b"grid-pow-0").digest() + bytes(4), dtype=">u4").astype(np.uint32)  # counter 0
ERR_LAST_LAYER, ERR_POW_SPAN = 1, 2


@pytest.fixture(scope="module")
def gp():
    return prover.GpuProver(verifier.Verifier(0))


@functools.lru_cache(maxsize=None)
def first_nonce(hash, pow_bits):
    """the smallest nonce of STATE's channel after the last layer's mix (below 2^21 for every case here: 503 400 at most)"""
    H = prover.HASHES[hash]
    digest, target = H(STATE[:8].astype(">u4").tobytes() + prover._be(LAST)).digest(), (1 << (64 - pow_bits)) - 1
    return next(n for n in range(1 << 21) if int.from_bytes(H(digest + n.to_bytes(8, "big")).digest()[24:], "little") < target)


def expected(hash, pow_bits, span):
    """-> (state, queries, nonce hi lo, error bits) of the tail over [0, span), by the Python channel of prover.py"""
    nonce = first_nonce(hash, pow_bits)
    if nonce >= span:
        return STATE, np.zeros(Q, np.uint32), np.full(2, FILL, np.uint32), ERR_POW_SPAN
    ch = prover._Channel(prover.HASHES[hash])
    ch.digest = STATE[:8].astype(">u4").tobytes()
    ch.mix(prover._be(LAST))
    ch.mix(nonce.to_bytes(8, "big"))
    queries = [w & ((1 << L) - 1) for w in ch.draw_words() + ch.draw_words()][:Q]
    state = np.concatenate([np.frombuffer(ch.digest, dtype=">u4"), [ch.counter]]).astype(np.uint32)
    return state, np.array(queries, np.uint32), np.array([nonce >> 32, nonce & 0xFFFFFFFF], np.uint32), 0


def run(gp, hash, pow_bits, span, work, last=None):
    """one launch on fresh buffers -> (state, queries, nonce, error bits) as the device left them"""
    dev = lambda a: gp.torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to(gp.dev)  # noqa: E731
    state, tail, err = dev(STATE), dev(np.full(Q + 2, FILL, np.uint32)), gp._zeros(1)
    last = dev(np.tile(np.array(LAST, np.uint32), (32, 1)) if last is None else last)
    gp._call("ss_p_finish_grid_dev", int(hash == "blake2s"), L, Q, (1 << (64 - pow_bits)) - 1, span, state.data_ptr(),
             last.data_ptr(), last.shape[0], tail.data_ptr(), tail[Q:].data_ptr(), err.data_ptr(), work.data_ptr())
    host = lambda t: t.cpu().numpy().view(np.uint32)  # noqa: E731
    return host(state), host(tail)[:Q], host(tail)[Q:], int(err.cpu()[0])


def check(got, want):
    for name, g, w in zip(("state", "queries", "nonce", "error bits"), got, want):
        assert np.array_equal(g, w), (name, g, w)


def work_words(gp):
    return gp.torch.zeros(3, dtype=gp.torch.int64, device=gp.dev)


# 0 bits: lane 0 of chunk 0.  4 bits over 2^20: hits in every chunk in flight at once, where "smallest" can go wrong.
# 12 and 18 bits: the hit lies one chunk and many chunks away from the start.
@pytest.mark.parametrize("hash", ["sha256", "blake2s"])
@pytest.mark.parametrize("pow_bits", [0, 4, 12, 18])
def test_kernel_equals_hashlib_and_the_python_channel(gp, hash, pow_bits):
    span = 1 << (pow_bits + 8 if pow_bits != 4 else 20)
    work = work_words(gp)
    check(run(gp, hash, pow_bits, span, work), expected(hash, pow_bits, span))
    assert not work.any()


# n* = 4430 (SHA-256), 4509 (Blake2s): the span that ends just before it, just behind it, inside the first round (< 256),
# inside a later chunk off every chunk and round boundary, and the full 64-bit span
@pytest.mark.parametrize("hash", ["sha256", "blake2s"])
@pytest.mark.parametrize("span", ["n", "n+1", 200, 3 * 4096 + 17, (1 << 64) - 1])
def test_span_edges(gp, hash, span):
    n = first_nonce(hash, 12)
    span = {"n": n, "n+1": n + 1}.get(span, span)
    work = work_words(gp)
    check(run(gp, hash, 12, span, work), expected(hash, 12, span))
    assert not work.any()


@pytest.mark.parametrize("span", [1 << 20, 4000])  # after a hit, after a miss
def test_work_words_clean_themselves(gp, span):
    work = work_words(gp)
    first = run(gp, "sha256", 12, span, work)
    check(first, expected("sha256", 12, span))
    assert not work.any()
    check(run(gp, "sha256", 12, span, work), first)  # (the same words again, never zeroed by the caller)
    assert not work.any()


def test_a_last_layer_that_is_not_constant_is_reported(gp):
    last = np.tile(np.array(LAST, np.uint32), (32, 1))
    last[29, 2] ^= 1
    want = expected("sha256", 12, 1 << 20)
    check(run(gp, "sha256", 12, 1 << 20, work_words(gp), last), want[:3] + (ERR_LAST_LAYER,))  # (the steps run all the same)


@pytest.mark.parametrize("bad", ["state", "last", "queries", "nonce", "err", "work", "last+4", "work+4", "span", "hash", "n_last"])
def test_refused_arguments_launch_nothing(gp, bad):
    buf = gp.torch.full((64,), FILL, dtype=gp.torch.int32, device=gp.dev)
    p = dict(state=buf.data_ptr(), last=buf[16:].data_ptr(), queries=buf[32:].data_ptr(), nonce=buf[44:].data_ptr(),
             err=buf[46:].data_ptr(), work=buf[48:].data_ptr())
    if bad in p:
        p[bad] = 0
    elif "+" in bad:
        p[bad[:-2]] += 4
    rc = gp.lib.ss_p_finish_grid_dev(gp.ver.ctx, 2 if bad == "hash" else 0, L, Q, 1 << 52, 0 if bad == "span" else 1 << 20,
                                     p["state"], p["last"], 0 if bad == "n_last" else 1, p["queries"], p["nonce"], p["err"],
                                     p["work"], gp._stream())
    gp.torch.cuda.synchronize(gp.dev)
    assert rc == binding.SS_ERR_ARG and bool((buf == FILL).all())


def small(**kw):
    return dict(n_cols=4, trace_log=4, log_blowup=1, n_queries=3, **kw)


@pytest.mark.parametrize("kw,transcript", [
    (small(pow_bits=5), "host"), (small(pow_bits=16), "device"), (small(pow_bits=16, hash="blake2s"), "device"),
    (dict(n_cols=4, trace_log=9, log_blowup=4, n_queries=16, pow_bits=5), "device"),  # proof.json
    (dict(n_cols=4, trace_log=9, log_blowup=4, n_queries=16, pow_bits=16), "host"),
], ids=lambda v: v if isinstance(v, str) else "log%d_pow%d_%s" % (v["trace_log"], v["pow_bits"], v.get("hash", "sha256")))
def test_records_with_grid_pow_equal_the_numpy_provers(gp, kw, transcript):
    proof = ss.stwo_from_json(stwo_prover.prove(seed=2, **kw))
    want = verifier.stwo_record(proof)
    out = gp.torch.full((want.size,), FILL, dtype=gp.torch.int32, device=gp.dev)
    got = gp.prove_record(out=out, transcript=transcript, grid_pow=True, seed=2, **kw)
    assert got is out and np.array_equal(got.cpu().numpy().view(np.uint32), want)
    if kw["pow_bits"] == 16:  # the one-workgroup search over a span that holds the nonce
        assert gp.torch.equal(got, gp.prove_record(transcript=transcript, pow_span=1 << 24, seed=2, **kw))
    batch = verifier.StwoDeviceBatch(gp.ver, gp.config(**kw), verifier.MODE_FIXTURE, got[None])
    batch.run()
    assert batch.status().tolist() == [0]
    want = verifier.stwo_minimal_record(formats.stwo_minimise(proof))
    got = gp.prove_minimal_record(transcript=transcript, grid_pow=True, seed=2, **kw)
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want)
