"""The transcript branches that depend on a hash output, on the device, against the restatement of test_rare_draws.py (hashlib
and Python integers; never prover._Channel, stwo_prover.Channel or the oracle as the reference):

  the redraw of channel_draw_qm31 at its three device sites -- Channel<HF>::draw_qm31 (csrc/ss_channel.h, through ss_selftest
  op 7), the verifier's transcript kernel (csrc/ss_stwo.hip), the FRI tail kernel's inlined loop (csrc/ss_prover_fri.hip) -- on
  the states of tests/golden/rare_draws.json;
  all 64 bits and the strictness of the proof-of-work compare -- Hasher<HF>::pow_value in the verifier and in the one-workgroup
  search, PowHash<HF>::value in the grid search (csrc/ss_prover_pow.hip) -- with targets at and next to the value itself;
  a nonce whose high word is not zero.

The shared and minimal record forms have no transcript kernel of their own (both end in stwo_transcript_kernel_*: csrc/ss_shared.hip
expands to per-query records, csrc/ss_minimal.hip writes the head words and launches the same kernel), so the verifier records run
as per-query records only."""
import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest
import torch  # noqa: F401  (before the library is loaded: it must bind the HIP runtime torch ships, binding.process_defaults)

import test_rare_draws as R

import stark_symphony_amd as ss
from stark_symphony_amd import formats, prover, verifier
from oracle import oracle as O

pytestmark = pytest.mark.gpu
FILL, ERR_POW_SPAN = 0x5A5A5A5A, 2
POW_CODE = verifier.stwo_code(4, 0, 0, 0)


@pytest.fixture(scope="module")
def ver():
    return verifier.Verifier(0)


@pytest.fixture(scope="module")
def gp(ver):
    return prover.GpuProver(ver)


# ------------------------------------------------------------------------------------------ C-GPU-1: Channel<HF>::draw_qm31
def test_selftest_draw_equals_the_restatement_on_unit_states(ver):
    cases, want = [], []
    for e in R.RARE["unit"]:
        H, digest = R.HASHES[e["hash"]], bytes.fromhex(e["digest"])
        value, after, attempts, first = R.draw(H, digest, e["counter"])
        assert e["word"] in first and attempts == (1 if e["word"] == 0xFFFFFFFD else 2)  # the branch, on the restatement alone
        cases.append([int(e["hash"] == "blake2s")] + R.words(digest) + [e["counter"]])
        want.append([1] + list(value) + [after])
    for i in range(8):  # ordinary states beside them: one attempt
        hash = ("sha256", "blake2s")[i % 2]
        digest = R.HASHES[hash](b"ordinary-%d" % i).digest()
        value, after, attempts, _ = R.draw(R.HASHES[hash], digest, 7 * i)
        assert attempts == 1
        cases.append([i % 2] + R.words(digest) + [7 * i])
        want.append([1] + list(value) + [after])
    assert {(c[0], w[5] - c[9]) for c, w in zip(cases, want)} == {(0, 1), (0, 2), (1, 1), (1, 2)}
    assert ver.selftest(7, np.array(cases, dtype=np.uint32)).tolist() == want


# --------------------------------------------------------------------------------- C-GPU-2: the verifier's transcript kernel
@pytest.mark.parametrize("mode", [verifier.MODE_FIXTURE, verifier.MODE_LITERAL])
@pytest.mark.parametrize("hash", ["sha256", "blake2s"])
def test_verifier_redraws_as_the_restatement(ver, hash, mode):
    entries = [e for e in R.RARE["verifier"] if e["hash"] == hash]
    assert sorted(e["field"] for e in entries) == ["fri_roots[0]", "roots[2]"]
    proofs = [R.smallest_proof(hash)] + [R.record_proof(e) for e in entries]
    refs = [R.transcript(p) for p in proofs]
    n_draws = 3 + proofs[0].cfg.n_layers + 1
    assert refs[0]["attempts"] == [1] * n_draws  # the branch, on the restatement alone: none, then one redraw each
    for e, ref in zip(entries, refs[1:]):
        assert ref["attempts"] == [2 if i == R.redrawn_ordinal(e) else 1 for i in range(n_draws)]
    b = ver.stwo_batch(proofs, mode)
    b.run()
    status = b.status().tolist()
    assert status == [O.stwo_verify(p, mode) for p in proofs]
    if mode == verifier.MODE_FIXTURE:
        assert status[0] == 0
    for e, st in zip(entries, status[1:]):
        assert st >> 24 != 1 and R.expected_record_status(e, mode, st), hex(st)
    for pi, ref in enumerate(refs):  # (proof 0, unmodified: the comparison itself works)
        got = b.intermediates(pi)
        assert got["oods_point"].tolist() == ref["oods_point"], pi
        assert got["fold_alphas"].tolist() == ref["fold_alphas"], pi
        assert got["queries"].tolist() == ref["queries"], pi


# ------------------------------------------------------------------------------------------- C-GPU-3: the FRI tail kernel
def tail_reference(H, state, layer, cinv, n_layers):
    """reference() of test_gpu_prover_fri_tail.py over the restated draw -> (arena, roots, alphas, state, attempts per layer)"""
    to_words = lambda b: np.frombuffer(b, dtype=">u4").astype(np.uint32)  # noqa: E731
    digest, counter = R.be(state[:8]), int(state[8])
    vals = [tuple(int(x) for x in row) for row in layer]
    arena, roots, alphas, attempts, off = [], [], [], [], 0
    for _ in range(n_layers):
        level = [H(R.be(v)).digest() for v in vals]
        rows = list(level)
        while len(level) > 1:
            level = [H(level[2 * i] + level[2 * i + 1]).digest() for i in range(len(level) // 2)]
            rows += level
        digest = H(digest + level[0]).digest()  # channel_mix_u256: the counter starts again at 0
        alpha, counter, n, _ = R.draw(H, digest, 0)
        attempts.append(n)
        half, nxt = len(vals) // 2, []
        for i in range(half):
            v0, v1 = vals[2 * i], vals[2 * i + 1]
            diff = tuple((a - b) * int(cinv[off + i]) % R.P for a, b in zip(v0, v1))
            nxt.append(tuple((a + b + c) % R.P for a, b, c in zip(v0, v1, R.qmul(diff, alpha))))
        vals, off = nxt, off + half
        arena += [to_words(b"".join(rows)), np.full(8, FILL, np.uint32), np.array(vals, dtype=np.uint32).reshape(-1)]
        roots.append(to_words(level[0]))
        alphas.append(alpha)
    state = np.concatenate([to_words(digest), [counter]]).astype(np.uint32)
    return np.concatenate(arena), np.array(roots), np.array(alphas, dtype=np.uint32), state, attempts


@pytest.mark.parametrize("e", R.TAILS)
def test_fri_tail_redraws_as_the_restatement(gp, e):
    log_n = n_layers = e["log_n"]  # (1, 1) and (2, 2)
    state, layer = np.array(e["state"], dtype=np.uint32), np.array(e["layer"], dtype=np.uint32)
    cinv = np.random.default_rng(log_n).integers(1, R.P, size=1 << log_n, dtype=np.uint32)
    want = tail_reference(R.HASHES[e["hash"]], state, layer, cinv, n_layers)
    assert want[4] == [2] + [1] * (n_layers - 1)  # the branch, on the restatement alone
    assert int(want[3][8]) == (2 if n_layers == 1 else 1)  # the counter after the last draw: 2 behind a redraw
    dev = lambda a: gp.torch.from_numpy(a.view(np.int32)).to(gp.dev)  # noqa: E731
    fill = lambda *shape: gp.torch.full(shape, FILL, dtype=gp.torch.int32, device=gp.dev)  # noqa: E731
    assert gp.lib.ss_p_fri_tail_words(log_n, n_layers) == want[0].size
    state_dev, layer_dev, cinv_dev = dev(state), dev(layer), dev(cinv)
    arena, roots, alphas = fill(want[0].size), fill(n_layers, 8), fill(n_layers, 4)
    gp._call("ss_p_fri_tail_dev", int(e["hash"] == "blake2s"), log_n, n_layers, state_dev.data_ptr(), layer_dev.data_ptr(),
             cinv_dev.data_ptr(), arena.data_ptr(), roots.data_ptr(), alphas.data_ptr())
    for name, got, ref in zip(("arena", "roots", "alphas", "state"), (arena, roots, alphas, state_dev), want):
        assert np.array_equal(got.cpu().numpy().view(np.uint32), ref), name


# ------------------------------------------------------------------------------ C-GPU-4: the verifier's proof-of-work compare
@pytest.mark.parametrize("which", ["small", "prod", "small-blake2s"])
def test_verifier_compares_all_64_bits_of_the_pow_value_strictly(ver, stwo_small, stwo_prod, which):
    base = {"small": stwo_small, "prod": stwo_prod}.get(which) or R.smallest_proof("blake2s")
    cases = R.pow_cases(base)
    assert [want for _, want in cases[:2]] == [POW_CODE, 0] and {want for _, want in cases} == {POW_CODE, 0}
    for target, want in cases:
        p = R.with_target(base, target)
        b = ver.stwo_batch([p], verifier.MODE_FIXTURE)
        assert b.cs.pow_target == target
        b.run()
        assert b.status().tolist() == [want] and O.stwo_verify(p, O.MODE_FIXTURE) == want, hex(target)


# -------------------------------------------------------------------------------- C-GPU-5: the provers' proof-of-work compare
SPAN, L, Q = 1 << 12, 13, 11


@functools.lru_cache(maxsize=None)
def pow_values(hash):
    """-> (digest after the last layer's mix, v(n) for n < SPAN) of STATE / LAST of test_gpu_prover_pow.py, by hashlib"""
    import test_gpu_prover_pow as TP
    H = R.HASHES[hash]
    digest = H(R.be(TP.STATE[:8]) + R.be(TP.LAST)).digest()
    return digest, [int.from_bytes(H(digest + n.to_bytes(8, "big")).digest()[24:], "little") for n in range(SPAN)]


def finish_expected(hash, target):
    """-> (state, queries, nonce hi lo or None, error bits) of the transcript's end over [0, SPAN) under `target`"""
    import test_gpu_prover_pow as TP
    H = R.HASHES[hash]
    digest, values = pow_values(hash)
    nonce = next((n for n, v in enumerate(values) if v < target), None)
    if nonce is None:
        return TP.STATE, np.zeros(Q, np.uint32), None, ERR_POW_SPAN
    digest = H(digest + nonce.to_bytes(8, "big")).digest()
    queries = [w & ((1 << L) - 1) for c in (0, 1) for w in R.words(H(digest + c.to_bytes(4, "big")).digest())][:Q]
    return np.array(R.words(digest) + [2], np.uint32), np.array(queries, np.uint32), np.array([nonce >> 32, nonce & 0xFFFFFFFF], np.uint32), 0


def finish(gp, entry, hash, target):
    """one launch of `entry` on fresh buffers -> (state, queries, nonce, error bits) as the device left them"""
    import test_gpu_prover_pow as TP
    dev = lambda a: gp.torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to(gp.dev)  # noqa: E731
    state, tail, err = dev(TP.STATE), dev(np.full(Q + 2, FILL, np.uint32)), gp._zeros(1)
    last = dev(np.tile(np.array(TP.LAST, np.uint32), (32, 1)))
    args = [int(hash == "blake2s"), L, Q, target, SPAN, state.data_ptr(), last.data_ptr(), last.shape[0], tail.data_ptr(),
            tail[Q:].data_ptr(), err.data_ptr()]
    work = TP.work_words(gp)
    gp._call(entry, *(args + [work.data_ptr()] if entry == "ss_p_finish_grid_dev" else args))
    host = lambda t: t.cpu().numpy().view(np.uint32)  # noqa: E731
    assert not work.any()
    return host(state), host(tail)[:Q], host(tail)[Q:], int(err.cpu()[0])


@pytest.mark.parametrize("hash", ["sha256", "blake2s"])
@pytest.mark.parametrize("entry", ["ss_p_finish_grid_dev", "ss_p_finish_dev"])
def test_prover_searches_compare_all_64_bits_strictly(gp, entry, hash):
    _, values = pow_values(hash)
    smallest = sorted(values)[:3]
    assert len(set(smallest)) == 3
    outcomes = set()
    for vk in smallest:
        for target in (vk + 1, vk):
            want = finish_expected(hash, target)
            # by arithmetic: v(k) + 1 admits v(k) itself, v(k) does not -- the smallest value of all admits nothing
            hits = [n for n, v in enumerate(values) if (v <= vk if target == vk + 1 else v < vk)]
            assert (want[2] is None) == (not hits) and (want[2] is None or int(want[2][1]) == hits[0])
            outcomes.add(want[3])
            state, queries, nonce, err = finish(gp, entry, hash, target)
            assert err == want[3] and np.array_equal(state, want[0]) and np.array_equal(queries, want[1]), (hex(target), err, nonce)
            if want[2] is not None:
                assert np.array_equal(nonce, want[2]), hex(target)
    assert outcomes == {0, ERR_POW_SPAN}


def prove_small(gp, kw, seed, target, span):
    """ss_p_prove_small_dev for one seed with the caller's own 64-bit target -> (row, error word)"""
    cs = verifier.stwo_cfg_struct(gp.config(**kw), verifier.MODE_FIXTURE)
    words = gp.lib.ss_stwo_record_words(C.byref(cs))
    rows = gp.torch.full((2, words), FILL, dtype=gp.torch.int32, device=gp.dev)
    err = gp.torch.full((2,), FILL, dtype=gp.torch.int32, device=gp.dev)
    arena = gp._empty(gp.lib.ss_p_small_arena_words(C.byref(cs), 1))
    n_log, l_log = kw["trace_log"], kw["trace_log"] + kw["log_blowup"]
    (_, itw_n, _), (tw_c, itw_c, hxhy_c), (tw_l, itw_l, hxhy_l) = gp.domain(n_log), gp.domain(n_log + 1), gp.domain(l_log)
    tables = prover.SmallTables(*[x.data_ptr() for x in (itw_n, tw_c, itw_c, hxhy_c, tw_l, itw_l, hxhy_l)])
    root = (C.c_uint32 * 8)(*R.words(R.HASHES[kw.get("hash", "sha256")](b"").digest()))
    seeds_dev = gp.torch.tensor([seed, 0], dtype=gp.torch.int64, device=gp.dev)
    gp._call("ss_p_prove_small_dev", C.byref(cs), target, span, seeds_dev.data_ptr(), 1, 1, C.byref(tables), root, arena.data_ptr(),
             arena.numel(), rows.data_ptr(), words, err.data_ptr())
    gp.torch.cuda.synchronize(gp.dev)
    host = rows.cpu().numpy().view(np.uint32)
    assert (host[1] == FILL).all() and int(err[1].cpu()) == FILL  # the guard row, the guard word
    return rows[:1], host[0], int(err[0].cpu())


@pytest.mark.parametrize("hash", ["sha256", "blake2s"])
def test_one_launch_prover_compares_all_64_bits_strictly(gp, hash):
    kw = dict(R.SMALLEST, hash=hash)
    proof, span = R.smallest_proof(hash), 1 << (kw["pow_bits"] + 8)
    ref = R.transcript(proof)
    H, v = R.HASHES[hash], ref["pow_value"]
    value = lambda n: int.from_bytes(H(ref["digest_before_nonce"] + n.to_bytes(8, "big")).digest()[24:], "little")  # noqa: E731
    assert value(proof.pow_nonce) == v and all(value(n) > v for n in range(proof.pow_nonce))
    # target v + 1: the numpy prover's nonce is the smallest that meets it, and the row is the numpy prover's record
    _, row, err = prove_small(gp, kw, 0, v + 1, span)
    assert err == 0 and np.array_equal(row, verifier.stwo_record(proof))
    # target v: that nonce no longer meets it -- a later one, or none in the span
    later = next((n for n in range(span) if value(n) < v), None)
    assert later is None or later > proof.pow_nonce
    rows, row, err = prove_small(gp, kw, 0, v, span)
    if later is None:
        assert err == ERR_POW_SPAN
    else:
        cfg = proof.cfg
        at = 24 + 4 * (cfg.n_cols + 16) + 8 * (cfg.n_layers + 1) + 4  # the record's nonce words: hi, lo
        assert err == 0 and row[at:at + 2].tolist() == [later >> 32, later & 0xFFFFFFFF]
        batch = verifier.StwoDeviceBatch(gp.ver, R.with_target(proof, v).cfg, verifier.MODE_FIXTURE, rows)
        batch.run()
        assert batch.status().tolist() == [0]


# ------------------------------------------------------------------------------------------- C-GPU-6: a high nonce word
@pytest.mark.parametrize("hash", ["sha256", "blake2s"])
def test_a_nonce_with_a_high_word_is_mixed_in_full(ver, hash):
    base = R.smallest_proof(hash)
    nonce = R.high_nonce(base)
    assert nonce >= 1 << 32 and nonce >> 32 != 0
    p = base.copy()
    p.pow_nonce = nonce
    ref = R.transcript(p)
    assert ref["pow_value"] < p.cfg.pow_target and ref["queries"] != [] and ref["digest_before_nonce"] == R.transcript(base)["digest_before_nonce"]
    b = ver.stwo_batch([base, p], verifier.MODE_FIXTURE)
    b.run()
    status = b.status().tolist()
    assert status == [0, O.stwo_verify(p, O.MODE_FIXTURE)] and status[1] != POW_CODE
    assert b.intermediates(1)["queries"].tolist() == ref["queries"]
    assert b.intermediates(0)["queries"].tolist() == R.transcript(base)["queries"]
