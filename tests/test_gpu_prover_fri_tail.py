"""ss_p_fri_tail_dev (include/ss_prover_fri.h): the FRI commit of every layer that fits in one workgroup, in one launch.
The kernel alone against hashlib and exact Python integers, word for word; records made with fri_tail=True against the
numpy prover's; the arguments it refuses."""
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
T = binding.lib().ss_p_fri_tail_log()
FILL = 0x5A5A5A5A


@pytest.fixture(scope="module")
def gp():
    return prover.GpuProver(verifier.Verifier(0))


def reference(H, state, layer, cinv, n_layers):
    """-> (arena words, roots, alphas, state) of n_layers commits and folds, in hashlib and Python integers"""
    words = lambda b: np.frombuffer(b, dtype=">u4").astype(np.uint32)  # noqa: E731
    ch = prover._Channel(H)
    ch.digest, ch.counter = prover._be(state[:8]), int(state[8])
    vals = [tuple(int(x) for x in row) for row in layer]
    arena, roots, alphas, off = [], [], [], 0
    for _ in range(n_layers):
        level = [H(prover._be(v)).digest() for v in vals]
        rows = list(level)
        while len(level) > 1:
            level = [H(level[2 * i] + level[2 * i + 1]).digest() for i in range(len(level) // 2)]
            rows += level
        ch.mix(level[0])
        alpha = ch.draw_qm31()
        half = len(vals) // 2
        vals = [prover.qadd(prover.qadd(vals[2 * i], vals[2 * i + 1]),
                            prover.qmul(prover.qmul(prover.qsub(vals[2 * i], vals[2 * i + 1]), (int(cinv[off + i]), 0, 0, 0)), alpha))
                for i in range(half)]
        off += half
        arena += [words(b"".join(rows)), np.full(8, FILL, np.uint32), np.array(vals, dtype=np.uint32).reshape(-1)]
        roots.append(words(level[0]))
        alphas.append(alpha)
    state = np.concatenate([words(ch.digest), [ch.counter]]).astype(np.uint32)
    return np.concatenate(arena), np.array(roots), np.array(alphas, dtype=np.uint32), state


@pytest.mark.parametrize("log_n,n_layers,hash", [
    (1, 1, "sha256"), (2, 2, "sha256"),            # the single pair
    (6, 6, "sha256"), (7, 3, "sha256"), (7, 3, "blake2s"), (8, 8, "sha256"),  # a wavefront of pairs: below, at, above
    (T - 1, 2, "sha256"), (T, 1, "sha256"),        # a pair per thread; more pairs than threads
    (T, T, "sha256"), (T, T, "blake2s"),           # the largest layer down to one value
])
def test_kernel_equals_hashlib_and_python_integers(gp, log_n, n_layers, hash):
    rng = np.random.default_rng(100 * log_n + n_layers)
    n = 1 << log_n
    layer = rng.integers(0, prover.P, size=(n, 4), dtype=np.uint32)
    cinv = rng.integers(1, prover.P, size=n, dtype=np.uint32)
    state = rng.integers(0, 1 << 32, size=9, dtype=np.uint32)
    state[8] = 3
    want = reference(prover.HASHES[hash], state, layer, cinv, n_layers)
    dev = lambda a: gp.torch.from_numpy(a.view(np.int32)).to(gp.dev)  # noqa: E731
    fill = lambda *shape: gp.torch.full(shape, FILL, dtype=gp.torch.int32, device=gp.dev)  # noqa: E731
    assert gp.lib.ss_p_fri_tail_words(log_n, n_layers) == want[0].size
    state_dev, layer_dev, cinv_dev = dev(state), dev(layer), dev(cinv)
    arena, roots, alphas = fill(want[0].size), fill(n_layers, 8), fill(n_layers, 4)
    gp._call("ss_p_fri_tail_dev", int(hash == "blake2s"), log_n, n_layers, state_dev.data_ptr(), layer_dev.data_ptr(),
             cinv_dev.data_ptr(), arena.data_ptr(), roots.data_ptr(), alphas.data_ptr())
    for name, got, ref in zip(("arena", "roots", "alphas", "state"), (arena, roots, alphas, state_dev), want):
        assert np.array_equal(got.cpu().numpy().view(np.uint32), ref), name  # (row 2n - 1 of every tree: still the poison)


def small(trace_log, **kw):
    return dict(n_cols=4, trace_log=trace_log, log_blowup=1, n_queries=3, pow_bits=3, **kw)


@pytest.mark.parametrize("kw,transcript", [
    (dict(n_cols=4, trace_log=2, log_blowup=1, n_queries=1, pow_bits=5), "device"),   # the whole commit in the kernel
    (dict(n_cols=4, trace_log=9, log_blowup=4, n_queries=16, pow_bits=5), "device"),  # proof.json
    (small(T), "device"), (small(T + 1), "device"),  # LDE 2^(T+1), 2^(T+2): one and two layers of the launch loop first
    (small(5, hash="blake2s"), "device"),
    (small(T), "host"),
], ids=lambda v: v if isinstance(v, str) else "log%d_%s" % (v["trace_log"], v.get("hash", "sha256")))
def test_record_with_fri_tail_equals_the_numpy_provers(gp, kw, transcript):
    want = verifier.stwo_record(ss.stwo_from_json(stwo_prover.prove(seed=3, **kw)))
    out = gp.torch.full((want.size,), FILL, dtype=gp.torch.int32, device=gp.dev)
    got = gp.prove_record(out=out, transcript=transcript, fri_tail=True, seed=3, **kw)
    assert got is out and np.array_equal(got.cpu().numpy().view(np.uint32), want)


def test_minimal_record_with_fri_tail_equals_the_definition(gp):
    kw = dict(n_cols=4, trace_log=9, log_blowup=4, n_queries=16, pow_bits=5)
    want = verifier.stwo_minimal_record(formats.stwo_minimise(ss.stwo_from_json(stwo_prover.prove(seed=1, **kw))))
    got = gp.prove_minimal_record(transcript="device", fri_tail=True, seed=1, **kw)
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want)


@pytest.mark.parametrize("hash,log_n,n_layers", [(0, 0, 1), (0, T + 1, 1), (0, 4, 0), (0, 4, 5), (2, 4, 2)])
def test_refused_arguments_launch_nothing(gp, hash, log_n, n_layers):
    arena = gp.torch.full((18 << 4,), FILL, dtype=gp.torch.int32, device=gp.dev)
    ins = gp._zeros(64 + 4 * (2 << T))
    rc = gp.lib.ss_p_fri_tail_dev(gp.ver.ctx, hash, log_n, n_layers, ins.data_ptr(), ins[16:].data_ptr(), ins[16:].data_ptr(),
                                  arena.data_ptr(), ins[32:].data_ptr(), ins[48:].data_ptr(), gp._stream())
    gp.torch.cuda.synchronize(gp.dev)
    assert rc == binding.SS_ERR_ARG and bool((arena == FILL).all())
