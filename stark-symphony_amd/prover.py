"""GPU wide-Fibonacci circle-STARK prover.

Chains the kernels of include/ss_prover.h into the protocol of the external stwo fork that made
the reference's proofs (stwo-verifier/tests/data/proof*.json): trace -> circle iFFT/LDE ->
Merkle commit -> composition polynomial in 16 partition columns -> OODS samples at P / 2P ->
two-batch DEEP quotients -> FRI commit -> proof of work -> queries -> decommit.  The
Fiat-Shamir channel (a few dozen hashes) and the O(columns) scalar QM31 algebra stay on the
host; everything proportional to the domain size runs in HIP kernels.

Output: the reference's `proof.json` schema (format C), byte for byte equal to
tools/stwo_prover.py -- and therefore to the reference's two fixtures
(tests/test_gpu_prover.py).  `prove_record` / `prove_records` give the same proof as the verifier's
per-query record (include/ss_verify.h) written by the GPU: after the FRI commit the transcript's tail
and the decommitment run in two kernels (include/ss_prover_record.h) and only an error word is read.
With transcript="device" the transcript before the FRI commit runs on the GPU as well
(include/ss_prover_transcript.h): the whole proof is enqueued without a host read.
`prove_minimal_record` / `prove_minimal_records` end the same way with the MINIMAL record (one sorted, deduplicated
decommitment per tree), whose layout the GPU plans from the queries (include/ss_prover_minimal.h).
"""
from __future__ import annotations

import ctypes as C
import hashlib
import time
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import binding as B

P = (1 << 31) - 1
Q4 = Tuple[int, int, int, int]
HASHES = {"sha256": hashlib.sha256, "blake2s": lambda b=b"": hashlib.blake2s(b, digest_size=32)}


# ------------------------------------------------------------- host QM31 scalars (Python ints)
def _cmul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def qmul(x: Q4, y: Q4) -> Q4:
    ac = _cmul(x[0:2], y[0:2])
    bd = _cmul(x[2:4], y[2:4])
    r = _cmul(bd, (2, 1))
    ad = _cmul(x[0:2], y[2:4])
    bc = _cmul(x[2:4], y[0:2])
    return ((ac[0] + r[0]) % P, (ac[1] + r[1]) % P, (ad[0] + bc[0]) % P, (ad[1] + bc[1]) % P)


def qadd(x: Q4, y: Q4) -> Q4:
    return tuple((a + b) % P for a, b in zip(x, y))


def qsub(x: Q4, y: Q4) -> Q4:
    return tuple((a - b) % P for a, b in zip(x, y))


def _cinv(a):
    n = pow((a[0] * a[0] + a[1] * a[1]) % P, P - 2, P)
    return (a[0] * n % P, (-a[1]) * n % P)


def qinv(x: Q4) -> Q4:
    a2 = _cmul(x[0:2], x[0:2])
    b2 = _cmul(x[2:4], x[2:4])
    t = _cmul(b2, (2, 1))
    den = ((a2[0] - t[0]) % P, (a2[1] - t[1]) % P)
    di = _cinv(den)
    re = _cmul(x[0:2], di)
    im = _cmul(((-x[2]) % P, (-x[3]) % P), di)
    return (re[0], re[1], im[0], im[1])


ONE: Q4 = (1, 0, 0, 0)
ZERO: Q4 = (0, 0, 0, 0)


def _interpolant(sp_y: Q4, value: Q4, alpha_i: Q4):
    """deep/quotients.simf:25-36 on canonical values."""
    a0 = (0, 0, (-2 * value[2]) % P, (-2 * value[3]) % P)
    b0 = (0, 0, (-2 * sp_y[2]) % P, (-2 * sp_y[3]) % P)
    c0 = qsub(qmul(b0, value), qmul(a0, sp_y))
    return qmul(alpha_i, a0), qmul(alpha_i, b0), qmul(alpha_i, c0)


class _Channel:
    """stwo-verifier/src/channel.simf:31-172 (host side of the Fiat-Shamir transcript)."""

    def __init__(self, h):
        self.h = h
        self.digest = bytes(32)
        self.counter = 0

    def mix(self, b: bytes) -> None:
        self.digest = self.h(self.digest + b).digest()
        self.counter = 0

    def draw_words(self) -> List[int]:
        d = self.h(self.digest + self.counter.to_bytes(4, "big")).digest()
        self.counter += 1
        return [int.from_bytes(d[4 * i:4 * i + 4], "big") for i in range(8)]

    def draw_qm31(self) -> Q4:
        while True:
            w = self.draw_words()
            if all(x < 4294967294 for x in w[:4]):
                return tuple(x % P for x in w[:4])


def _be(words: Sequence[int]) -> bytes:
    return b"".join(int(w).to_bytes(4, "big") for w in words)


class SmallTables(C.Structure):
    """ss_p_small_tables (include/ss_prover_small.h)"""
    _fields_ = [(k, C.c_void_p) for k in ("itw_n", "tw_c", "itw_c", "hxhy_c", "tw_l", "itw_l", "hxhy_l")]


class GpuProver:
    """Proves on one MI355X through the ss_p_* kernels.  `ver` is a verifier.Verifier (it owns
    the library context and the device)."""

    def __init__(self, ver):
        import torch
        self.torch = torch
        self.ver = ver
        self.dev = ver.device
        self.lib = B.lib()
        u32p, vp, sz = C.c_void_p, C.c_void_p, C.c_size_t
        L = self.lib

        def sig(name, *args):
            f = getattr(L, name)
            f.restype = C.c_int
            f.argtypes = [vp] + list(args) + [vp]
        sig("ss_p_trace", C.c_uint32, C.c_uint32, C.c_uint32, u32p)
        sig("ss_p_twiddles", C.c_uint32, u32p, u32p, u32p)
        sig("ss_p_fft", C.c_uint32, C.c_uint32, u32p, u32p, C.c_int)
        sig("ss_p_lde", C.c_uint32, C.c_uint32, C.c_uint32, u32p, u32p, u32p)
        sig("ss_p_hash_rows", C.c_uint32, sz, C.c_uint32, u32p, sz, u32p)
        sig("ss_p_hash_qm31", C.c_uint32, sz, u32p, u32p)
        sig("ss_p_merkle", C.c_uint32, sz, u32p)
        sig("ss_p_merkle_dup", C.c_uint32, sz, u32p, u32p)
        sig("ss_p_composition", C.c_uint32, C.c_uint32, u32p, u32p, u32p, u32p)
        sig("ss_p_eval_at_point", C.c_uint32, u32p, u32p, u32p, u32p)
        sig("ss_p_eval_at_point_batch", C.c_uint32, C.c_uint32, u32p, sz, u32p, u32p, u32p)
        sig("ss_p_channel_fri_layer", C.c_uint32, u32p, u32p, u32p, u32p)
        sig("ss_p_fri_fold_dev", sz, u32p, u32p, u32p, u32p)
        sig("ss_p_quotients", C.c_uint32, C.c_uint32, u32p, u32p, C.c_uint32, u32p, u32p, u32p, u32p, u32p, u32p)
        sig("ss_p_fri_fold", sz, u32p, u32p, u32p, u32p)
        sig("ss_p_pow", C.c_uint32, u32p, C.c_uint64, C.c_uint64, C.c_uint64, u32p)
        sig("ss_p_finish_dev", C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, u32p, u32p, sz, u32p, u32p, u32p)
        sig("ss_p_decommit_record", C.POINTER(B.StwoCfg), vp, u32p, u32p, u32p, u32p, u32p, u32p, u32p)
        # include/ss_prover_minimal.h
        sig("ss_p_decommit_minimal", C.POINTER(B.StwoCfg), vp, u32p, u32p, u32p, u32p, u32p, u32p, u32p, u32p)
        sig("ss_p_minimal_pack_dev", sz, u32p, sz, u32p, u32p, vp)
        # include/ss_prover_transcript.h
        sig("ss_p_channel_begin_dev", C.c_uint32, u32p, u32p, u32p, u32p, u32p)
        sig("ss_p_composition_dev", C.c_uint32, C.c_uint32, u32p, u32p, u32p, u32p)
        sig("ss_p_oods_point_dev", C.c_uint32, C.c_uint32, u32p, u32p, u32p, u32p, u32p, u32p)
        sig("ss_p_eval_at_point_dev", C.c_uint32, C.c_uint32, u32p, sz, u32p, u32p, u32p)
        sig("ss_p_deep_coeffs_dev", C.c_uint32, C.c_uint32, u32p, u32p, u32p, u32p, u32p, u32p)
        sig("ss_p_quotients_dev", C.c_uint32, C.c_uint32, u32p, u32p, C.c_uint32, u32p, u32p, u32p, u32p, u32p)
        # include/ss_prover_fri.h
        sig("ss_p_fri_tail_dev", C.c_uint32, C.c_uint32, C.c_uint32, u32p, u32p, u32p, u32p, u32p, u32p)
        L.ss_p_fri_tail_log.restype = C.c_uint32
        L.ss_p_fri_tail_log.argtypes = []
        L.ss_p_fri_tail_words.restype = sz
        L.ss_p_fri_tail_words.argtypes = [C.c_uint32, C.c_uint32]
        # include/ss_prover_pow.h
        sig("ss_p_finish_grid_dev", C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, u32p, u32p, sz, u32p, u32p, u32p, vp)
        # include/ss_prover_small.h
        sig("ss_p_prove_small_dev", C.POINTER(B.StwoCfg), C.c_uint64, C.c_uint64, vp, sz, sz, C.POINTER(SmallTables), u32p, vp, sz,
            vp, sz, vp)
        L.ss_p_small_limits.restype = None
        L.ss_p_small_limits.argtypes = [C.POINTER(C.c_uint32)] * 3
        L.ss_p_small_arena_words.restype = sz
        L.ss_p_small_arena_words.argtypes = [C.POINTER(B.StwoCfg), sz]
        L.ss_p_eval_scratch_words.restype = sz
        L.ss_p_eval_scratch_words.argtypes = [C.c_uint32, C.c_uint32]
        self._dom: Dict[int, tuple] = {}
        self._pow_work: Dict[int, object] = {}  # stream -> the three work words of ss_p_finish_grid_dev (zero between launches)
        self._workers: list = []  # (prover, stream) of prove_many
        self._pending = None  # (commit, record, error word, size word or None) of a prove_record / prove_minimal_record not yet checked
        self.record_words = None  # size of the last checked prove_minimal_record's record
        self.small_errors = None  # the SS_P_ERR_* words of the last prove_records(one_launch=True), as the kernel left them
        self.timings: Dict[str, float] = {}

    # -- small helpers ---------------------------------------------------------------------
    def _stream(self) -> int:
        return int(self.torch.cuda.current_stream(self.dev).cuda_stream)

    def _empty(self, *shape):
        return self.torch.empty(shape, dtype=self.torch.int32, device=self.dev)

    def _zeros(self, *shape):
        return self.torch.zeros(shape, dtype=self.torch.int32, device=self.dev)

    @staticmethod
    def _q(v: Q4):
        return (C.c_uint32 * 4)(*[int(x) for x in v])

    @staticmethod
    def _root_words(root: bytes):
        """A 32-byte root as the eight uint32 words the library takes."""
        return (C.c_uint32 * 8)(*np.frombuffer(root, dtype=">u4"))

    @staticmethod
    def _raise_errors(bits) -> None:
        """The SS_P_ERR_* bits of one proof, or of a batch, that have no other route: raises what prove_proof raises."""
        bits = np.asarray(bits)
        if (bits & 4).any():  # SS_P_ERR_TRANSCRIPT
            raise AssertionError("transcript: a draw ran out of tries, or 1 + t^2 has no inverse")
        if (bits & 1).any():  # SS_P_ERR_LAST_LAYER
            raise AssertionError("last FRI layer is not constant: the quotient is not low degree")

    def _set_timings(self, marks, t_start: float) -> None:
        """timings <- the time between consecutive marks, by name, and their total."""
        prev = t_start
        self.timings = {}
        for name, ts in marks:
            self.timings[name] = ts - prev
            prev = ts
        self.timings["total"] = prev - t_start

    def _call(self, name: str, *args) -> None:
        B.check(getattr(self.lib, name)(self.ver.ctx, *args, self._stream()))

    def _host(self, t) -> np.ndarray:
        return t.detach().cpu().numpy().view(np.uint32)

    def domain(self, m: int):
        """(tw, itw, hx_hy) of the canonic coset of log size m."""
        if m not in self._dom:
            tw, itw = self._empty(1 << m), self._empty(1 << m)
            hxhy = self._empty(1 << m)
            half = 1 << (m - 1)
            self._call("ss_p_twiddles", m, tw.data_ptr(), itw.data_ptr(), hxhy.data_ptr())
            hxhy[half:] = tw[:half]  # pair y = twiddle layer 0
            self._dom[m] = (tw, itw, hxhy)
        return self._dom[m]

    def fft(self, m: int, data, inverse: bool) -> None:
        tw, itw, _ = self.domain(m)
        self._call("ss_p_fft", m, data.shape[0], data.data_ptr(), (itw if inverse else tw).data_ptr(),
                   1 if inverse else 0)

    def extend(self, coefs, m: int, x_only: bool = False):
        """Coefficients [ncols, 2^k] -> evaluations on the canonic coset of log size m.
        x_only: the polynomials have no y term -- `coefs` holds the coefficients of x^k1 pi(x)^k2 ... only (the even
        positions of the full array) -- so the two points (x, +-y) of a storage pair get the same value: returns ONE
        value per pair, [ncols, 2^(m-1)].  That is the transform of size m - 1 run with the twiddles of layers 1.. of
        size m, which lie behind its first 2^(m-1) words (include/ss_prover.h, ss_p_twiddles)."""
        k = int(coefs.shape[1]).bit_length() - 1
        assert coefs.shape[1] == 1 << k and coefs.is_contiguous()
        tw = self.domain(m)[0]
        if x_only:
            tw, m = tw[1 << (m - 1):], m - 1
        out = self._empty(coefs.shape[0], 1 << m)
        # (ss_p_lde: the forward transform of the coefficients followed by zeros, without writing or reading the zeros)
        self._call("ss_p_lde", k, m, coefs.shape[0], coefs.data_ptr(), out.data_ptr(), tw.data_ptr())
        return out

    def merkle(self, hsel: int, leaves_fn, n: int):
        """levels[(2n - 1), 8]: leaves first, root last."""
        levels = self._empty(2 * n, 8)
        leaves_fn(levels)
        self._call("ss_p_merkle", hsel, n, levels.data_ptr())
        return levels

    def _root(self, levels, n: int) -> bytes:
        return self._host(levels[2 * n - 2]).astype(">u4").tobytes()

    @staticmethod
    def _path_rows(n: int, indices: Sequence[int], skip: int = 0) -> np.ndarray:
        """Rows of a tree's `levels` array holding the sibling hashes leaf -> root of every index at
        level `skip`, concatenated in query order.  Level j starts at row 2n - (2n >> j)."""
        h = n.bit_length() - 1
        if h <= skip or not len(indices):
            return np.zeros(0, dtype=np.int64)
        j = np.arange(skip, h, dtype=np.int64)
        idx = np.asarray(indices, dtype=np.int64)[:, None] >> (j - skip)[None, :]
        return ((2 * n - ((2 * n) >> j))[None, :] + (idx ^ 1)).reshape(-1)

    class _Gather:
        """Rows of several device arrays, fetched with ONE upload of all row indices and ONE
        download: requests are queued, `fetch()` uploads the concatenated indices, gathers on the
        device, concatenates and copies back (the decommitment used to cost a synchronising index
        upload and a synchronising download per tree and per layer)."""

        def __init__(self, prover):
            self.p, self.req = prover, []

        def rows(self, array, idxs) -> int:
            self.req.append((array, np.asarray(idxs, dtype=np.int64)))
            return len(self.req) - 1

        def take(self, tensor) -> int:
            self.req.append((tensor, None))
            return len(self.req) - 1

        def fetch(self) -> List[np.ndarray]:
            t = self.p.torch
            all_idx = np.concatenate([i for _, i in self.req if i is not None] or [np.zeros(0, np.int64)])
            dev_idx = t.from_numpy(all_idx).to(self.p.dev)
            parts, shapes, pos = [], [], 0
            for array, idx in self.req:
                if idx is None:
                    sel = array
                else:
                    sel = array[dev_idx[pos:pos + idx.size]]
                    pos += idx.size
                parts.append(sel.reshape(-1))
                shapes.append(tuple(sel.shape))
            flat = self.p._host(t.cat(parts)) if parts else np.zeros(0, np.uint32)
            out, pos = [], 0
            for shp in shapes:
                size = int(np.prod(shp))
                out.append(flat[pos:pos + size].reshape(shp))
                pos += size
            return out

    @staticmethod
    def _hash_rows_to_json(rows: np.ndarray) -> List[List[int]]:
        if rows.size == 0:
            return []
        return rows.reshape(-1, 8).astype(">u4").view(np.uint8).reshape(-1, 32).tolist()

    # -- the protocol ----------------------------------------------------------------------
    def _commit(self, n_cols: int = 4, trace_log: int = 9, log_blowup: int = 4, n_queries: int = 16,
                pow_bits: int = 5, seed: int = 0, hash: str = "sha256", transcript: str = "host", err=None,
                fri_tail: bool = False):
        """The protocol up to and including the FRI commit, shared by prove_proof and prove_record: everything the rest
        of a proof is made from, still on the device (trees, layers, samples, the channel state after the last fold).
        transcript="device" (prove_record only; `err` = its error word): the channel and the scalar QM31 algebra run in
        the kernels of include/ss_prover_transcript.h, and nothing here reads from the device or waits for it.
        fri_tail: from the first FRI layer of at most 2^ss_p_fri_tail_log() values on, that layer and every one after it
        are committed by ONE launch of one workgroup (include/ss_prover_fri.h) in place of four to six launches per layer;
        their trees and folds are then views of one arena.  The same bits either way."""
        import types
        torch = self.torch
        if transcript not in ("host", "device"):
            raise ValueError("transcript must be 'host' or 'device'")
        on_dev = transcript == "device"
        t_start = time.perf_counter()
        marks: List[Tuple[str, float]] = []

        def mark(name: str) -> None:
            if on_dev:  # no synchronisation between phases: timings carries the total only
                return
            torch.cuda.current_stream(self.dev).synchronize()  # this proof's stream only: others may be in flight (prove_many)
            marks.append((name, time.perf_counter()))
        n, L, N = trace_log, trace_log + log_blowup, n_cols
        K = L - 1 - log_blowup
        hsel = 1 if hash == "blake2s" else 0
        H = HASHES[hash]
        ch = _Channel(H)
        size_L = 1 << L

        # ---- trace, interpolation, LDE, commitment
        cols = self._empty(N, 1 << n)
        self._call("ss_p_trace", n, N, (seed * 0x9E3779B1) % P, cols.data_ptr())
        coefs = cols
        self.fft(n, coefs, True)
        lde = self.extend(coefs, L)
        trace_tree = self.merkle(hsel, lambda lv: self._call(
            "ss_p_hash_rows", hsel, size_L, N, lde.data_ptr(), size_L, lv.data_ptr()), size_L)
        const_root = H(b"").digest()
        trace_root = cp_root = oods_trace = oods_cp = None
        if on_dev:
            # channel[9], cp_alpha[4], points[16], sums + alpha^16 [20], fold factors of P [n][4] and of 2P [n - 1][4]
            tr = self._empty(52 + 8 * n)
            state, cp_alpha_dev, points, sums, fac = tr[:9], tr[12:16], tr[16:32], tr[32:52], tr[52:]
            self._call("ss_p_channel_begin_dev", hsel, self._root_words(const_root),
                       trace_tree[2 * size_L - 2].data_ptr(), state.data_ptr(), cp_alpha_dev.data_ptr(), err.data_ptr())
        else:
            trace_root = self._root(trace_tree, size_L)
            mark("trace commit")
            ch.mix(const_root)
            ch.mix(trace_root)
            cp_alpha = ch.draw_qm31()

        # ---- composition polynomial on the coset of log size n + 1, 16 partition columns
        ev = self.extend(coefs, n + 1)
        _, _, hxhy_c = self.domain(n + 1)
        F = self._empty(4, 1 << (n + 1))
        if on_dev:
            self._call("ss_p_composition_dev", n, N, ev.data_ptr(), hxhy_c.data_ptr(), cp_alpha_dev.data_ptr(), F.data_ptr())
        else:
            self._call("ss_p_composition", n, N, ev.data_ptr(), hxhy_c.data_ptr(), self._q(cp_alpha), F.data_ptr())
        self.fft(n + 1, F, True)
        # Partition 4c + part of coordinate c takes the coefficients whose two lowest index bits are `part` and is a
        # polynomial in x alone: in the basis of size n its coefficients sit at the even positions (no y term).  Kept
        # compact (2^(n-1) per column); its LDE has one value per storage pair, and the two leaves of a pair are equal.
        cp_coefs = self._empty(16, 1 << (n - 1))
        for c in range(4):
            for part in range(4):
                cp_coefs[4 * c + part] = F[c, part::4]
        cp_lde = self.extend(cp_coefs, L, x_only=True)  # [16, 2^(L-1)]: position i -> column value at i >> 1
        half_L = size_L >> 1

        # The two leaves of a storage pair are equal, so the 2^L leaf hashes are 2^(L-1) distinct ones and the first node
        # level is H(leaf || leaf): `cp_tree` holds the tree from that level up (its "leaves" are the level-1 nodes), the
        # duplicated leaf level exists nowhere (round 3 wrote it out: 0.8 GB of copies per proof).
        pair_leaf = self._empty(half_L, 8)
        self._call("ss_p_hash_rows", hsel, half_L, 16, cp_lde.data_ptr(), half_L, pair_leaf.data_ptr())
        cp_tree = self.merkle(hsel, lambda lv: self._call(
            "ss_p_merkle_dup", hsel, half_L, pair_leaf.data_ptr(), lv.data_ptr()), half_L)
        _, itw_L, hxhy_L = self.domain(L)
        layer = self._empty(size_L, 4)
        samples = self._empty(N + 16, 4)
        if on_dev:
            # ---- OODS point, samples, DEEP coefficients and quotients: six launches, every scalar stays in `tr`
            f1, f2x = fac[:4 * n], fac[4 * n:]
            self._call("ss_p_oods_point_dev", hsel, n, state.data_ptr(), cp_tree[2 * half_L - 2].data_ptr(), points.data_ptr(),
                       f1.data_ptr(), f2x.data_ptr() if n > 1 else None, err.data_ptr())
            scratch = self._empty(max(4, self.lib.ss_p_eval_scratch_words(n, max(N, 16))))
            self._call("ss_p_eval_at_point_dev", n, N, coefs.data_ptr(), 1 << n, f1.data_ptr(), scratch.data_ptr(), samples.data_ptr())
            if n > 1:
                self._call("ss_p_eval_at_point_dev", n - 1, 16, cp_coefs.data_ptr(), 1 << (n - 1), f2x.data_ptr(),
                           scratch.data_ptr(), samples[N:].data_ptr())
            else:  # a two-row trace: every partition is a constant
                samples[N:] = 0
                samples[N:, 0] = cp_coefs[:, 0]
            bcoef = self._empty(N + 16, 4)
            self._call("ss_p_deep_coeffs_dev", hsel, N, state.data_ptr(), samples.data_ptr(), points.data_ptr(),
                       bcoef.data_ptr(), sums.data_ptr(), err.data_ptr())
            self._call("ss_p_quotients_dev", L, N, lde.data_ptr(), cp_lde.data_ptr(), L - 1, hxhy_L.data_ptr(),
                       bcoef.data_ptr(), points.data_ptr(), sums.data_ptr(), layer.data_ptr())
        else:
            cp_root = self._root(cp_tree, half_L)
            mark("composition commit")
            ch.mix(cp_root)

            # ---- OODS point, samples
            t = ch.draw_qm31()
            t_sq = qmul(t, t)
            inv = qinv(qadd(ONE, t_sq))
            px, py = qmul(qsub(ONE, t_sq), inv), qmul(qadd(t, t), inv)
            p2x = qsub(qadd(qmul(px, px), qmul(px, px)), ONE)
            p2y = qadd(qmul(px, py), qmul(px, py))

            def factors(x: Q4, y: Q4, m: int) -> np.ndarray:
                f = [y, x]
                cur = x
                for _ in range(2, m):
                    cur = qsub(qadd(qmul(cur, cur), qmul(cur, cur)), ONE)
                    f.append(cur)
                return np.array(f[:m], dtype=np.uint32).reshape(-1)
            scratch = self._empty(max(N, 16) * (3 << n))
            f1, f2 = factors(px, py, n), factors(p2x, p2y, n)
            # all columns of a commitment are sampled at one point: one batched fold chain each
            self._call("ss_p_eval_at_point_batch", n, N, coefs.data_ptr(), 1 << n, f1.ctypes.data, scratch.data_ptr(),
                       samples.data_ptr())
            if n > 1:
                f2x = np.ascontiguousarray(f2[4:])  # no y term: the factors x, pi(x), ... over the compact coefficients
                self._call("ss_p_eval_at_point_batch", n - 1, 16, cp_coefs.data_ptr(), 1 << (n - 1), f2x.ctypes.data,
                           scratch.data_ptr(), samples[N:].data_ptr())
            else:  # a two-row trace: every partition is a constant
                samples[N:] = 0
                samples[N:, 0] = cp_coefs[:, 0]
            samp = self._host(samples).astype(np.int64)
            oods_trace = [tuple(int(x) for x in samp[k]) for k in range(N)]
            oods_cp = [tuple(int(x) for x in samp[N + k]) for k in range(16)]
            ch.mix(b"".join(_be(v) for v in oods_trace) + b"".join(_be(v) for v in oods_cp))
            deep_alpha = ch.draw_qm31()
            mark("oods")

            # ---- DEEP quotients (trace batch at P, composition batch at 2P)
            bco: List[Q4] = []
            sums: List[Q4] = []
            for sp_y, vals in ((py, oods_trace), (p2y, oods_cp)):
                A, Cc, alpha_i = ZERO, ZERO, deep_alpha
                for v in vals:
                    a, b, c = _interpolant(sp_y, v, alpha_i)
                    bco.append(b)
                    A, Cc = qadd(A, a), qadd(Cc, c)
                    alpha_i = qmul(alpha_i, deep_alpha)
                sums += [A, Cc]
            a16 = ONE
            for _ in range(16):
                a16 = qmul(a16, deep_alpha)
            bcoef = torch.from_numpy(np.array(bco, dtype=np.uint32).view(np.int32)).to(self.dev)
            pts = (C.c_uint32 * 8)(*px, *py)
            pts2 = (C.c_uint32 * 8)(*p2x, *p2y)
            sa = (C.c_uint32 * 20)(*[x for v in sums + [a16] for x in v])
            self._call("ss_p_quotients", L, N, lde.data_ptr(), cp_lde.data_ptr(), L - 1, hxhy_L.data_ptr(),
                       bcoef.data_ptr(), pts, pts2, sa, layer.data_ptr())
            mark("quotients")

        # ---- FRI commit (fri/commit.simf:70-85), channel included, without a host round trip: per
        # layer the Merkle tree, then one lane mixes the root and draws alpha ON THE DEVICE, then the
        # fold reads alpha from device memory.  One download at the end (roots, channel, last layer).
        if not on_dev:
            state = torch.from_numpy(np.concatenate([np.frombuffer(ch.digest, dtype=">u4").astype(np.uint32),
                                                     np.array([ch.counter], dtype=np.uint32)]).view(np.int32)).to(self.dev)
        roots_dev = self._empty(K + 1, 8)
        alphas_dev = self._empty(K + 1, 4)
        layers, trees = [], []
        tail_log = self.lib.ss_p_fri_tail_log() if fri_tail else 0
        for l in range(K + 1):
            size = size_L >> l
            if L - l <= tail_log:
                # layers l .. K in one launch; block j of the arena = tree [2 n_j][8] then fold [n_j / 2][4], n_j = size >> j
                off = size_L - (size_L >> l)
                arena = self._empty(self.lib.ss_p_fri_tail_words(L - l, K + 1 - l))
                self._call("ss_p_fri_tail_dev", hsel, L - l, K + 1 - l, state.data_ptr(), layer.data_ptr(), itw_L[off:].data_ptr(),
                           arena.data_ptr(), roots_dev[l:].data_ptr(), alphas_dev[l:].data_ptr())
                for j in range(K + 1 - l):
                    n_j, at = size >> j, 36 * (size - (size >> j))
                    layers.append(layer)
                    trees.append(arena[at:at + 16 * n_j].view(2 * n_j, 8))
                    layer = arena[at + 16 * n_j:at + 18 * n_j].view(n_j >> 1, 4)
                break
            layers.append(layer)
            cur = layer
            tree = self.merkle(hsel, lambda lv: self._call(
                "ss_p_hash_qm31", hsel, size, cur.data_ptr(), lv.data_ptr()), size)
            trees.append(tree)
            self._call("ss_p_channel_fri_layer", hsel, state.data_ptr(), tree[2 * size - 2].data_ptr(),
                       alphas_dev[l].data_ptr(), roots_dev[l].data_ptr())
            nxt = self._empty(size >> 1, 4)
            off = size_L - (size_L >> l)  # inverse twiddle layer l = 1 / fold coordinate
            self._call("ss_p_fri_fold_dev", size >> 1, layer.data_ptr(), itw_L[off:].data_ptr(),
                       alphas_dev[l].data_ptr(), nxt.data_ptr())
            layer = nxt
        return types.SimpleNamespace(
            N=N, n=n, L=L, K=K, Q=n_queries, pow_bits=pow_bits, hash=hash, hsel=hsel, ch=ch, mark=mark, marks=marks,
            t_start=t_start, const_root=const_root, trace_root=trace_root, cp_root=cp_root, oods_trace=oods_trace,
            oods_cp=oods_cp, samples=samples, lde=lde, cp_lde=cp_lde, trace_tree=trace_tree, pair_leaf=pair_leaf,
            cp_tree=cp_tree, layers=layers, trees=trees, state=state, roots_dev=roots_dev, last=layer, on_dev=on_dev)

    def _finish(self, c, target: int, span: int, tail, err, grid_pow: bool) -> None:
        """ss_p_finish_dev on the commit `c` (tail = queries, nonce hi, lo); grid_pow: ss_p_finish_grid_dev, the same
        words with the nonce searched by the whole device.  Its three work words are zeroed once per stream, here, and
        left zero by every launch, so proofs in flight on different streams never share them."""
        args = (c.hsel, c.L, c.Q, target, min(span, (1 << 64) - 1), c.state.data_ptr(), c.last.data_ptr(), c.last.shape[0], tail.data_ptr(),
                tail[c.Q:].data_ptr(), err.data_ptr())
        if not grid_pow:
            self._call("ss_p_finish_dev", *args)
            return
        stream = self._stream()
        if stream not in self._pow_work:
            self._pow_work[stream] = self.torch.zeros(3, dtype=self.torch.int64, device=self.dev)
        self._call("ss_p_finish_grid_dev", *args, self._pow_work[stream].data_ptr())

    def _host_tail(self, c, grid_pow: bool = False):
        """The end of the transcript on the host: one download (channel, FRI roots, last layer), the last layer's mix,
        the proof of work searched by ss_p_pow, the queries.  -> (roots, last, nonce, queries)
        grid_pow: ss_p_finish_grid_dev runs that end on the device over 2^(pow_bits + 8) nonces first, and the one
        download brings its nonce and queries along; should it find none, the search below takes over."""
        torch = self.torch
        ch, K, L, pow_bits, hsel, mark = c.ch, c.K, c.L, c.pow_bits, c.hsel, c.mark
        g = self._Gather(self)
        if grid_pow:
            tail, err = self._empty(c.Q + 2), self._zeros(1)
            self._finish(c, (1 << (64 - pow_bits)) - 1, 1 << (pow_bits + 8), tail, err, True)
            k_tail, k_err = g.take(tail), g.take(err)
        k_state, k_roots, k_last = g.take(c.state), g.take(c.roots_dev), g.take(c.last)
        got = g.fetch()
        if grid_pow and not int(got[k_err][0]) & 2:  # (bit 1, the last layer: raised below as ever)
            roots = [got[k_roots][l].astype(">u4").tobytes() for l in range(K + 1)]
            last_all = got[k_last]
            if not (last_all == last_all[0]).all():
                raise AssertionError("last FRI layer is not constant: the quotient is not low degree")
            mark("fri commit")
            mark("pow")
            t = [int(x) for x in got[k_tail]]
            return roots, tuple(int(x) for x in last_all[0]), (t[c.Q] << 32) | t[c.Q + 1], t[:c.Q]
        ch.digest = got[k_state][:8].astype(">u4").tobytes()
        ch.counter = int(got[k_state][8])
        roots = [got[k_roots][l].astype(">u4").tobytes() for l in range(K + 1)]
        last_all = got[k_last]
        if not (last_all == last_all[0]).all():
            raise AssertionError("last FRI layer is not constant: the quotient is not low degree")
        last = tuple(int(x) for x in last_all[0])
        ch.mix(_be(last))
        mark("fri commit")

        # ---- proof of work (pow.simf:22-36): smallest nonce, searched on the GPU
        target = (1 << (64 - pow_bits)) - 1
        dig = (C.c_uint32 * 8)(*np.frombuffer(ch.digest, dtype=">u4").astype(np.uint32))
        out = torch.zeros(2, dtype=torch.int32, device=self.dev)
        start, span = 0, 1 << min(22, pow_bits + 8)  # expected 2^pow_bits tries: rarely a second pass
        while True:
            self._call("ss_p_pow", hsel, dig, target, start, span, out.data_ptr())
            nonce = int(self._host(out).view(np.uint64)[0])
            if nonce != 0xFFFFFFFFFFFFFFFF:
                break
            start += span
            span = min(span * 4, 1 << 22)
        ch.mix(nonce.to_bytes(8, "big"))
        mark("pow")

        # ---- queries (fri/queries.simf:29-43) and decommitment
        mask = (1 << L) - 1
        queries: List[int] = []
        while len(queries) < c.Q:
            queries += [w & mask for w in ch.draw_words()]
        return roots, last, nonce, queries[:c.Q]

    def prove_proof(self, n_cols: int = 4, trace_log: int = 9, log_blowup: int = 4, n_queries: int = 16,
                    pow_bits: int = 5, seed: int = 0, hash: str = "sha256", fri_tail: bool = False, grid_pow: bool = False):
        """-> formats.StwoProof (arrays; what the verifier's record is made from).  fri_tail: see _commit.
        grid_pow: the proof of work is ground by ss_p_finish_grid_dev (include/ss_prover_pow.h) instead of ss_p_pow's
        spans of 2^22 with a download after each; the same proof."""
        c = self._commit(n_cols, trace_log, log_blowup, n_queries, pow_bits, seed, hash, fri_tail=fri_tail)
        N, n, L, K = c.N, c.n, c.L, c.K
        size_L, half_L = 1 << L, 1 << (L - 1)
        lde, cp_lde, trace_tree, pair_leaf, cp_tree, layers, trees = (c.lde, c.cp_lde, c.trace_tree, c.pair_leaf,
                                                                      c.cp_tree, c.layers, c.trees)
        const_root, trace_root, cp_root, oods_trace, oods_cp = c.const_root, c.trace_root, c.cp_root, c.oods_trace, c.oods_cp
        mark, marks, t_start = c.mark, c.marks, c.t_start
        roots, last, nonce, queries = self._host_tail(c, grid_pow)
        self.queries = list(queries)  # (of the last proof made by this call path; prove_minimal uses them)
        # every gather of the decommitment is enqueued first, then downloaded at once
        g = self._Gather(self)
        lde_t, cp_lde_t = lde.T, cp_lde.T  # views: row = LDE position
        k_tq, k_cq = g.rows(lde_t, queries), g.rows(cp_lde_t, [q >> 1 for q in queries])  # [Q, N], [Q, 16]
        k_thw = g.rows(trace_tree, self._path_rows(size_L, queries))
        # composition tree: the sibling of leaf q is the other leaf of its pair (the same hash); above it, the tree over the pairs
        k_chw0 = g.rows(pair_leaf, [q >> 1 for q in queries])
        k_chw = g.rows(cp_tree, self._path_rows(half_L, [q >> 1 for q in queries]))
        k_layers = []
        cur_q = list(queries)
        for l in range(K + 1):
            size = size_L >> l
            k_sib = g.rows(layers[l], [q ^ 1 for q in cur_q])
            k_hw = g.rows(trees[l], self._path_rows(size, [q >> 1 for q in cur_q], skip=1))
            k_layers.append((k_sib, k_hw))
            cur_q = [q >> 1 for q in cur_q]
        got = g.fetch()

        def hashes(rows: np.ndarray, *shape) -> np.ndarray:
            """stored words [.., 8] -> bytes [.., 32]"""
            return np.ascontiguousarray(rows).reshape(-1, 8).astype(">u4").view(np.uint8).reshape(*shape, 32)
        from .formats import StwoConfig, StwoProof
        Q = n_queries
        proof = StwoProof(
            StwoConfig(N, n, L, Q, K, pow_bits, hash),
            np.stack([np.frombuffer(r, dtype=np.uint8) for r in (const_root, trace_root, cp_root)]),
            np.array(oods_trace, dtype=np.uint32).reshape(N, 4), np.array(oods_cp, dtype=np.uint32).reshape(16, 4),
            got[k_tq].reshape(Q, N).copy(), got[k_cq].reshape(Q, 16).copy(),
            list(hashes(got[k_thw], Q, L)),
            list(hashes(np.concatenate([got[k_chw0].reshape(Q, 1, 8), got[k_chw].reshape(Q, L - 1, 8)], axis=1), Q, L)),
            np.stack([np.frombuffer(r, dtype=np.uint8) for r in roots]), np.array(last, dtype=np.uint32),
            np.stack([got[ks].reshape(Q, 4) for ks, _ in k_layers]),
            [list(hashes(got[kh], Q, L - 1 - l)) for l, (_, kh) in enumerate(k_layers)], nonce)
        mark("decommit")
        self._set_timings(marks, t_start)
        return proof

    # -- the proof as the verifier's record, in device memory ------------------------------------
    @staticmethod
    def config(n_cols: int = 4, trace_log: int = 9, log_blowup: int = 4, n_queries: int = 16, pow_bits: int = 5,
               seed: int = 0, hash: str = "sha256"):
        """The formats.StwoConfig of the proofs these arguments give: what a verifier of prove_record's output expects."""
        from .formats import StwoConfig
        return StwoConfig(n_cols, trace_log, trace_log + log_blowup, n_queries, trace_log - 1, pow_bits, hash)

    def _decommit_record(self, c, queries_dev, nonce_dev, out, words_out=None) -> None:
        """ss_p_decommit_record into `out`; with `words_out` (the size word) ss_p_decommit_minimal."""
        # one ss_p_tree (levels, values, leaf) per tree: trace, composition, FRI layers
        desc = [(c.trace_tree, c.lde, None), (c.cp_tree, c.cp_lde, c.pair_leaf)] + list(zip(c.trees, c.layers, [None] * (c.K + 1)))
        trees_dev = self.torch.tensor([[t.data_ptr() if t is not None else 0 for t in row] for row in desc], dtype=self.torch.int64)
        # (device transcript: from pinned memory, so that the upload does not wait for the stream)
        trees_dev = trees_dev.pin_memory().to(self.dev, non_blocking=True) if c.on_dev else trees_dev.to(self.dev)
        root = self._root_words(c.const_root)
        args = (C.byref(c.cs), trees_dev.data_ptr(), c.samples.data_ptr(), c.roots_dev.data_ptr(), c.last.data_ptr(),
                nonce_dev.data_ptr(), root, queries_dev.data_ptr(), out.data_ptr())
        if words_out is None:
            self._call("ss_p_decommit_record", *args)
        else:
            self._call("ss_p_decommit_minimal", *args, words_out.data_ptr())

    def _enqueue_record(self, minimal: bool, out, words_out, pow_span: Optional[int], transcript: str, grid_pow: bool, kw):
        """What prove_record and prove_minimal_record share: the protocol up to the FRI commit, ss_p_finish_dev, the
        decommitment into `out` (one record, or with `minimal` a row of ss_stwo_minimal_max_words words and the size
        word `words_out`), all enqueued and left pending for check()."""
        self.check()
        err = self._zeros(1) if transcript == "device" else None
        c = self._commit(transcript=transcript, err=err, **kw)
        from .verifier import MODE_FIXTURE, stwo_cfg_struct
        c.cs = stwo_cfg_struct(self.config(c.N, c.n, c.L - c.n, c.Q, c.pow_bits, 0, c.hash), MODE_FIXTURE)
        words = (self.lib.ss_stwo_minimal_max_words if minimal else self.lib.ss_stwo_record_words)(C.byref(c.cs))
        if out is None:
            out = self._empty(words)
        if out.dtype != self.torch.int32 or out.numel() != words or not out.is_contiguous() or out.device != c.state.device:
            raise ValueError("out must be %d contiguous int32 words on the prover's device" % words)
        if minimal:
            if words_out is None:
                words_out = self._empty(1)
            if words_out.dtype != self.torch.int32 or words_out.numel() != 1 or words_out.device != c.state.device:
                raise ValueError("words_out must be one int32 word on the prover's device")
        # (grid_pow: 2^(pow_bits + 8) nonces hold none with probability e^-256, and the whole device searches them)
        span = pow_span if pow_span is not None else 1 << (c.pow_bits + 8 if grid_pow else min(22, c.pow_bits + 8))
        if err is None:
            err = self._zeros(1)
        tail = self._empty(c.Q + 2)  # queries, nonce hi, lo
        self._finish(c, c.cs.pow_target, span, tail, err, grid_pow)
        self._decommit_record(c, tail, tail[c.Q:], out, words_out)
        self._pending = (c, out, err, words_out)
        return out

    def prove_record(self, out=None, pow_span: Optional[int] = None, check: bool = True, transcript: str = "host",
                     grid_pow: bool = False, **kw):
        """The proof of prove_proof(**kw) as the per-query record of include/ss_verify.h (verifier.stwo_record of it, word
        for word), written by the GPU into `out`: int32[record_words] on the device, e.g. a row of a caller's
        [n, record_words] tensor (allocated here when None; it may be uninitialised).  After the FRI commit nothing returns
        to the host but one error word: ss_p_finish_dev ends the transcript (last layer, proof of work over the first
        `pow_span` nonces -- default 2^min(22, pow_bits + 8), the first pass of prove_proof's search -- and queries),
        ss_p_decommit_record gathers the record.  check=False leaves that word unread: the record is then valid once
        check() has returned, and the caller runs no other proof on this prover before.
        transcript="device": the transcript before the FRI commit runs on the GPU too (include/ss_prover_transcript.h: the
        three draws, the OODS point and samples, the DEEP coefficients), so between the first launch and check() nothing
        is read from the device and nothing waits for it; `timings` then carries `total` only.  The same record.
        fri_tail=True (any entry of this class takes it): the FRI layers that fit in one workgroup are committed by one
        launch (include/ss_prover_fri.h) instead of four to six launches each.  The same record again.
        grid_pow=True (any entry of this class takes it): ss_p_finish_grid_dev (include/ss_prover_pow.h) takes the place
        of ss_p_finish_dev -- the nonce is searched by a grid of workgroups over the whole device instead of one, and
        the default `pow_span` is 2^(pow_bits + 8) with no cap, so a pow_bits of 20 to 30 stays on this route instead of
        falling back to the host in check().  The same record again."""
        out = self._enqueue_record(False, out, None, pow_span, transcript, grid_pow, kw)
        if check:
            self.check()
        return out

    def prove_minimal_record(self, out=None, words_out=None, pow_span: Optional[int] = None, check: bool = True,
                             transcript: str = "host", grid_pow: bool = False, **kw):
        """The proof of prove_proof(**kw) as the MINIMAL record of include/ss_verify_forms.h (verifier.stwo_minimal_record
        of formats.stwo_minimise of it, word for word), planned and gathered by the GPU (ss_p_decommit_minimal) behind the
        same _commit and ss_p_finish_dev as prove_record, with the same arguments.  A minimal record's size depends on the
        queries: `out` is a row of ss_stwo_minimal_max_words words (int32 on the device, allocated here when None, it may
        be uninitialised) of which the record fills the first `words`, and words_out (one int32 word on the device, e.g.
        an element of a caller's [n] tensor) receives that size; nothing behind the record is written.  check=True reads
        the size together with the error word -- still one synchronisation -- and returns out[:words]; check=False returns
        the whole row, and words_out (and `record_words`) are valid once check() has returned."""
        out = self._enqueue_record(True, out, words_out, pow_span, transcript, grid_pow, kw)
        if check:
            self.check()
            return out[:self.record_words]
        return out

    def check(self) -> None:
        """Waits for the last prove_record / prove_minimal_record of this prover (on the current stream) and reads its
        error word (and a minimal record's size with it, into `record_words`) -- the only host read after the FRI commit.
        SS_P_ERR_LAST_LAYER raises what prove_proof raises.  SS_P_ERR_POW_SPAN (no nonce in the span) redoes the tail on
        the host path of prove_proof and the decommitment with the queries and nonce uploaded: the same record."""
        pending, self._pending = self._pending, None
        if pending is None:
            return
        c, out, err, words = pending
        if words is None:
            bits = int(err.cpu()[0])
        else:
            bits, self.record_words = (int(x) for x in self.torch.cat([err, words.reshape(1)]).cpu())
        self._raise_errors(bits)
        if bits & 2:
            _, _, nonce, queries = self._host_tail(c)
            tail = self.torch.from_numpy(np.array(queries + [nonce >> 32, nonce & 0xFFFFFFFF], dtype=np.uint32).view(np.int32)).to(self.dev)
            self._decommit_record(c, tail, tail[c.Q:], out, words)
            self.torch.cuda.current_stream(self.dev).synchronize()
            if words is not None:  # (other queries: another size)
                self.record_words = int(words.cpu().reshape(1)[0])
        if c.on_dev:
            self.timings = {"total": time.perf_counter() - c.t_start}
            return
        c.mark("tail")
        self._set_timings(c.marks, c.t_start)

    def prove_records(self, seeds: Sequence[int], workers: int = 4, one_launch: bool = False, n_groups: int = 0, **kw):
        """prove_record for every seed of `seeds` (keywords, transcript= included, are passed on) on the schedule of
        prove_many (the same worker streams and threads):
        -> int32[len(seeds), record_words] on the device, row i = the record of seeds[i], every row checked and the
        device synchronised.  ss_stwo_pack_dev / Verifier.pack_stwo_records_dev take the tensor as it is.
        one_launch=True: the same tensor from ONE launch of ss_p_prove_small_dev (include/ss_prover_small.h), a workgroup
        per proof on `n_groups` workgroups (0: two per compute unit), for the shapes within small_limits() -- a shape outside
        them, or no seed at all, raises ValueError before anything is launched.  The seeds go up once and one error word
        per proof comes back once (kept in `small_errors`); a proof whose nonce lies outside `pow_span` is redone through
        prove_record.  `workers`, `transcript`, `fri_tail` and `grid_pow` choose among routes to the same words and mean
        nothing here."""
        if one_launch:
            return self._prove_records_small(list(seeds), n_groups, **kw)
        seeds = list(seeds)
        if not seeds:
            return self._empty(0, 0)
        t0 = time.perf_counter()
        first = self.prove_record(seed=seeds[0], **kw)  # also fills the twiddle cache every worker shares
        rows = self._empty(len(seeds), first.numel())
        rows[0] = first

        def one(gp, i):
            gp.prove_record(out=rows[i], seed=seeds[i], **kw)
        self._run_many(len(seeds), workers, one, t0)
        return rows

    def small_limits(self) -> Tuple[int, int, int]:
        """(lde_log, n_cols, n_queries): the largest that prove_records(one_launch=True) serves."""
        lim = [C.c_uint32() for _ in range(3)]
        self.lib.ss_p_small_limits(*[C.byref(x) for x in lim])
        return tuple(int(x.value) for x in lim)

    def _prove_records_small(self, seeds: List[int], n_groups: int = 0, pow_span: Optional[int] = None, n_cols: int = 4,
                             trace_log: int = 9, log_blowup: int = 4, n_queries: int = 16, pow_bits: int = 5,
                             hash: str = "sha256", transcript: str = "device", fri_tail: bool = False, grid_pow: bool = False):
        torch = self.torch
        from .verifier import MODE_FIXTURE, stwo_cfg_struct
        shape = dict(n_cols=n_cols, trace_log=trace_log, log_blowup=log_blowup, n_queries=n_queries, pow_bits=pow_bits, hash=hash)
        L = trace_log + log_blowup
        max_l, max_n, max_q = self.small_limits()
        if not (1 <= trace_log and 1 <= log_blowup and L <= max_l and 1 <= n_cols <= max_n and 1 <= n_queries <= max_q):
            raise ValueError("one_launch serves lde_log <= %d, n_cols <= %d, n_queries <= %d (got %d, %d, %d)"
                             % (max_l, max_n, max_q, L, n_cols, n_queries))
        n = len(seeds)
        if not n or hash not in HASHES or not 0 <= n_groups <= n or any(not 0 <= s < 1 << 63 for s in seeds):
            raise ValueError("one_launch needs at least one seed in [0, 2^63), a known hash and n_groups <= len(seeds)")
        t0 = time.perf_counter()
        cs = stwo_cfg_struct(self.config(**shape), MODE_FIXTURE)
        words = self.lib.ss_stwo_record_words(C.byref(cs))
        if not n_groups:
            n_groups = min(n, 2 * torch.cuda.get_device_properties(self.dev).multi_processor_count)
        arena_words = self.lib.ss_p_small_arena_words(C.byref(cs), n_groups)
        (_, itw_n, _), (tw_c, itw_c, hxhy_c), (tw_l, itw_l, hxhy_l) = self.domain(trace_log), self.domain(trace_log + 1), self.domain(L)
        tables = SmallTables(*[x.data_ptr() for x in (itw_n, tw_c, itw_c, hxhy_c, tw_l, itw_l, hxhy_l)])
        root = self._root_words(HASHES[hash](b"").digest())
        seeds_dev = torch.tensor(seeds, dtype=torch.int64).pin_memory().to(self.dev, non_blocking=True)
        arena, rows, err = self._empty(arena_words), self._empty(n, words), self._empty(n)
        span = pow_span if pow_span is not None else 1 << min(22, pow_bits + 8)
        self._call("ss_p_prove_small_dev", C.byref(cs), cs.pow_target, span, seeds_dev.data_ptr(), n, n_groups, C.byref(tables),
                   root, arena.data_ptr(), arena_words, rows.data_ptr(), words, err.data_ptr())
        self.small_errors = bits = self._host(err).copy()  # the one read: it waits for the launch
        self._raise_errors(bits)
        for i in np.flatnonzero(bits & 2):  # no nonce in the span: the existing route, whose check() searches on
            self.prove_record(out=rows[int(i)], seed=seeds[int(i)], pow_span=span, transcript="device", **shape)
        dt = time.perf_counter() - t0
        self.timings = {"total": dt, "proofs_per_s": n / dt, "groups": n_groups}
        return rows

    def prove_minimal_records(self, seeds: Sequence[int], workers: int = 4, **kw):
        """prove_minimal_record for every seed of `seeds` on the schedule of prove_records, then packed on the device
        (ss_p_minimal_pack_dev): every proof writes a row of an [n, max_words] tensor and a word of an [n] size tensor, a
        scan of the sizes gives the offsets and a copy lays the records back to back.
        -> (records, offs): int32[offs[n]] and int64[n + 1] on the device, record i = records[offs[i]:offs[i + 1]], every
        proof checked and the device synchronised.  verifier.StwoMinimalDeviceBatch takes the pair as it is.
        (There is no one_launch= here: the one-launch kernel of prove_records writes per-query records only.)"""
        torch = self.torch
        seeds = list(seeds)
        n = len(seeds)
        if not n:
            return self._empty(0), torch.zeros(1, dtype=torch.int64, device=self.dev)
        t0 = time.perf_counter()
        words = self._empty(n)
        first = self.prove_minimal_record(words_out=words[0:1], check=False, seed=seeds[0], **kw)  # also fills the twiddle cache
        self.check()
        rows = self._empty(n, first.numel())
        rows[0] = first

        def one(gp, i):
            gp.prove_minimal_record(out=rows[i], words_out=words[i:i + 1], seed=seeds[i], **kw)
        self._run_many(n, workers, one, t0)
        packed = self._empty(rows.numel())
        offs = torch.empty(n + 1, dtype=torch.int64, device=self.dev)
        self._call("ss_p_minimal_pack_dev", n, rows.data_ptr(), rows.shape[1], words.data_ptr(), packed.data_ptr(), offs.data_ptr())
        total = int(offs[n].cpu())  # the final synchronisation
        dt = time.perf_counter() - t0
        self.timings.update(total=dt, proofs_per_s=n / dt)
        return packed[:total], offs

    def prove_many(self, seeds: Sequence[int], workers: int = 4, **kw) -> list:
        """Proofs of the same configuration for every seed of `seeds`, `workers` of them in flight, each on its own
        HIP stream (and host thread).  A single proof leaves the GPU idle between its many dependent launches -- the
        small upper Merkle levels, the channel round trips -- and other proofs' kernels fill those gaps; nothing else
        changes, so every proof is byte-identical to `prove_proof(seed=...)`.  Returns the StwoProofs in seed order;
        `self.timings["proofs_per_s"]` is the rate of the call."""
        seeds = list(seeds)
        out: list = [None] * len(seeds)
        if not seeds:
            return out
        t0 = time.perf_counter()
        out[0] = self.prove_proof(seed=seeds[0], **kw)  # also fills the twiddle cache every worker shares

        def one(gp, i):
            out[i] = gp.prove_proof(seed=seeds[i], **kw)
        self._run_many(len(seeds), workers, one, t0)
        return out

    def _run_many(self, count: int, workers: int, one, t0: float) -> None:
        """The schedule of prove_many / prove_records: items 1 .. count-1 (item 0 is done: it filled the twiddle cache)
        through one(prover, i), `workers` of them in flight; t0 = when the caller began item 0."""
        import itertools
        import threading
        torch = self.torch
        nxt = itertools.count(1)
        errors: list = []

        # worker provers and their streams live as long as this prover: the caching allocator keeps a pool per
        # stream, so a fresh stream per call would start every call with gigabytes of hipMalloc
        while len(self._workers) < workers:
            self._workers.append((self if not self._workers else GpuProver(self.ver), torch.cuda.Stream(device=self.dev)))

        def work(w: int) -> None:
            gp, stream = self._workers[w]
            gp._dom = self._dom  # read-only from here on
            try:
                with torch.cuda.stream(stream):
                    while not errors:
                        i = next(nxt)
                        if i >= count:
                            return
                        one(gp, i)
            except BaseException as e:  # noqa: BLE001
                errors.append(e)
        threads = [threading.Thread(target=work, args=(w,)) for w in range(max(1, min(workers, count - 1)))]
        # A worker that wakes from a stream synchronisation needs the interpreter lock back; with CPython's default
        # 5 ms switch interval it can wait that long for a thread that is busy converting arrays, which is a third
        # of a whole proof.  Ask for the lock every 50 us while the workers run.
        import sys
        interval = sys.getswitchinterval()
        sys.setswitchinterval(5e-5)
        try:
            for t in threads:
                t.start()
            for t in threads:
                t.join()
        finally:
            sys.setswitchinterval(interval)
        if errors:
            raise errors[0]
        torch.cuda.synchronize(self.dev)
        dt = time.perf_counter() - t0
        self.timings = {"total": dt, "proofs_per_s": count / dt, "workers": len(threads)}

    def prove_minimal(self, **kw):
        """The proof with ONE decommitment per tree -- queries sorted and deduplicated, only the siblings and fold
        partners the verifier cannot compute (formats.StwoMinimalProof; what upstream stwo's prover sends, where the
        reference's format repeats a full path per query: fri/queries.simf:41, scripts/generate_wit.py:36-42).  The
        prover holds every node anyway, so this is prove_proof() minus what is not sent."""
        from .formats import stwo_minimise
        proof = self.prove_proof(**kw)
        return stwo_minimise(proof, self.queries)

    def prove(self, n_cols: int = 4, trace_log: int = 9, log_blowup: int = 4, n_queries: int = 16,
              pow_bits: int = 5, seed: int = 0, hash: str = "sha256", fri_tail: bool = False, grid_pow: bool = False) -> dict:
        """The same proof in the reference's `proof.json` schema (format C): `prove_proof` plus the
        conversion of 170 KB of hashes into JSON's lists of byte values (3-4 ms of pure Python at the
        2^20 shape, reported as timings["json"])."""
        from .formats import stwo_to_json
        proof = self.prove_proof(n_cols, trace_log, log_blowup, n_queries, pow_bits, seed, hash, fri_tail, grid_pow)
        t0 = time.perf_counter()
        out = stwo_to_json(proof)
        self.timings["json"] = time.perf_counter() - t0
        self.timings["total"] += self.timings["json"]
        return out
