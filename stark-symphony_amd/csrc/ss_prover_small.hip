// A batch of small proofs in one launch, one workgroup per proof (include/ss_prover_small.h).
//
// prover.py proves through about fifty launches, each waiting for the one before; at 2^9 rows x 4 columns the proof is
// those launches.  Here a workgroup of 512 threads stays resident over a WHOLE proof and walks the phases of _commit
// (device transcript), ss_p_finish_dev and ss_p_decommit_record with nothing but workgroup barriers between them;
// workgroup g proves g, g + gridDim, g + 2 gridDim, ... in arena slot g.  No workgroup reads another's memory or waits
// for it: no counter, no spin, no inter-workgroup atomic.
//
//   arena      what a later phase gathers from lives in the slot: trace coefficients, LDE columns, the composition's
//              compact coefficients and pair values, pair leaf hashes, every tree's levels, every FRI layer.  Each is
//              written once and read once or twice, by this workgroup only.
//   transforms one column at a time in LDS (a 2^13-word column is 32 KB): loaded once, two butterfly layers per barrier
//              (four values a thread, radix 4), stored once.  A low-degree extension starts from the coefficients
//              repeated down the column: the top layers of a zero-extended transform pair a value with zero, i.e. copy.
//              The sixteen x-only partitions of the composition are an index permutation on the way from LDS to the arena.
//   trees      a thread owns a pair of leaves: it hashes both and their parent from registers.  A level of at most 1024
//              nodes is handed down through two ping-ponged LDS buffers ([word][node]: conflict-free writes, one 8-byte read
//              per word and child pair) and stored to the arena as it is produced -- the column buffer is the larger of
//              the two: no transform runs while a tree is built.  Wider levels (2^13 leaves: 4096 and 2048 nodes) are
//              re-read from the arena lines just written.  From 64 nodes down the level lives in the registers of
//              wavefront 0 and a parent's children are two lane reads.
//   channel    Channel<HF> in the registers of wavefront 0 (all lanes the same words) from the first mix to the last
//              draw; what it draws reaches the others through LDS and the barrier that ends the phase.
//   hashing    the pair hash is ONE out-of-line copy (node_call), the leaf / channel / nonce hashes go through the
//              out-of-line compressions of ss_hash.h: inlining one per phase is 15 copies of 64 unrolled rounds.
//
// What a phase computes is not written here: every phase calls the step of ss_prover_dev.h that the kernels of
// ss_prover.hip and ss_prover_transcript.hip call for the same element, with the variable of its workgroup-stride loop
// as the index.  This file holds where the operands live and who waits for whom.
#include <hip/hip_runtime.h>

#include "../../include/ss_prover.h"
#include "ss_ctx.h"
#include "ss_prover_dev.h"

using namespace ss;

extern "C" int ss_internal_set_err(int code, const char *msg);

namespace ss {
namespace {

constexpr uint32_t kSmallLde = 13, kSmallCols = 32, kSmallQueries = kMaxQueries;
constexpr uint32_t kNT = 512, kWaves = kNT / 64;
constexpr uint32_t kGroupsPerCu = 2;  // n_groups = 0: what is resident at once (one workgroup a CU at 256 VGPRs) and as much behind it
constexpr uint32_t kPlaneA = 1024, kPlaneB = 512;  // nodes of the two LDS level buffers
constexpr uint32_t kMaxTraceLog = kSmallLde - 1, kMaxSamples = kSmallCols + kCp;
static_assert(8 * kPlaneA == 1u << kSmallLde, "the column buffer is the first level buffer");

// ---- a slot of the arena (word offsets, each a multiple of 4: rows move as uint4)
struct SmallSlot {
    uint32_t coefs, lde, ev, F, cp_coefs, cp_lde, pair_leaf, trace_tree, cp_tree, layers, fri_trees, total;
};
SS_HD inline SmallSlot small_slot(uint32_t N, uint32_t n, uint32_t L)
{
    SmallSlot s{};
    uint32_t o = 0;
    auto take = [&](uint32_t words) { const uint32_t at = o; o += (words + 3u) & ~3u; return at; };
    s.coefs = take(N << n);             // [N][2^n] trace values, then their coefficients
    s.lde = take(N << L);               // [N][2^L]
    s.ev = take(N << (n + 1));          // [N][2^(n+1)] the trace on the composition's coset
    s.F = take(4u << (n + 1));          // [4][2^(n+1)] the composition polynomial's coordinates
    s.cp_coefs = take(kCp << (n - 1));  // [16][2^(n-1)]
    s.cp_lde = take(kCp << (L - 1));    // [16][2^(L-1)] one value per storage pair
    s.pair_leaf = take(8u << (L - 1));  // [2^(L-1)][8]
    s.trace_tree = take(16u << L);      // [2 * 2^L][8]
    s.cp_tree = take(16u << (L - 1));   // [2 * 2^(L-1)][8]
    s.layers = take(8u << L);           // layer l at 4 (2^(L+1) - 2^(L+1-l)): [2^(L-l)][4], l = 0 .. n
    s.fri_trees = take(32u << L);       // tree l at 16 (2^(L+1) - 2^(L+1-l)): [2 * 2^(L-l)][8]
    s.total = o;
    return s;
}

struct SmallArgs {
    uint32_t N, n, L, Q, count;
    uint64_t target, span;
    Dig const_root;  // stored words
    const uint64_t *seeds;
    uint32_t *arena, *rec, *err;
    uint64_t row_stride;
    ss_p_small_tables tb;
};

// what the phases hand each other besides the arena
struct SmallShared {
    alignas(16) uint32_t samples[4 * kMaxSamples];
    alignas(16) uint32_t bcoef[4 * kMaxSamples];  // (quotients_pair reads a column's coefficient as one uint4)
    uint32_t cp_alpha[4], points[16], sums[20], alpha[4], last[4], nonce[2], dig[8];
    uint32_t f1[4 * kMaxTraceLog], f2x[4 * kMaxTraceLog];
    uint32_t troot[8], croot[8], roots[8 * kMaxTraceLog];  // stored words
    uint32_t queries[kSmallQueries];
    unsigned long long best;
    QM31 wave[2][kWaves];
};

// ------------------------------------------------------------------------------ hashing
template <int HF>
__device__ __noinline__ Dig node_call(Dig l, Dig r)
{
    Dig d;
    Hasher<HF>::template pair<true>(l.v, r.v, d.v);
    return d;
}

// The tree over n = 2^k >= 2 leaves into tree[2n][8] (ss_p_merkle's layout: leaves first, root in row 2n - 2).
// leaf(i) -> the hash of leaf i in native words.  -> the root (native) in every lane of wavefront 0.  Every thread of the
// workgroup calls it; the caller runs a barrier before either LDS buffer is written again.
template <int HF, class Leaf>
__device__ __forceinline__ Dig build_tree(uint32_t *tree, uint32_t n, Leaf leaf, uint32_t *lds_a, uint32_t *lds_b, uint32_t t)
{
    const uint32_t np = n >> 1;
    bool in_lds = np <= kPlaneA;
    for (uint32_t p = t; p < np; p += kNT) {
        const Dig l = leaf(2 * p), r = leaf(2 * p + 1);
        st_node<HF>(tree, 2 * p, l.v);
        st_node<HF>(tree, 2 * p + 1, r.v);
        const Dig d = node_call<HF>(l, r);
        st_node<HF>(tree, n + p, d.v);
        if (in_lds) {
#pragma unroll
            for (int k = 0; k < 8; k++) lds_a[k * kPlaneA + p] = d.v[k];
        }
    }
    __syncthreads();
    uint32_t cur = np, row = n;  // the level of `cur` nodes starts at row `row`
    uint32_t *src = lds_a, *dst = lds_b;
    uint32_t sp = kPlaneA, dp = kPlaneB;
    while (cur > 64) {
        const uint32_t par = cur >> 1;
        const bool out_lds = par <= kPlaneA;
        if (!in_lds) { dst = lds_a; dp = kPlaneA; }
        for (uint32_t i = t; i < par; i += kNT) {
            Dig l, r;
            if (in_lds) {
#pragma unroll
                for (int k = 0; k < 8; k++) {
                    const uint2 c = *reinterpret_cast<const uint2 *>(src + k * sp + 2 * i);
                    l.v[k] = c.x; r.v[k] = c.y;
                }
            } else {
                l = ld_node<HF>(tree, row + 2 * i);
                r = ld_node<HF>(tree, row + 2 * i + 1);
            }
            const Dig d = node_call<HF>(l, r);
            st_node<HF>(tree, row + cur + i, d.v);
            if (out_lds) {
#pragma unroll
                for (int k = 0; k < 8; k++) dst[k * dp + i] = d.v[k];
            }
        }
        __syncthreads();
        row += cur;
        cur = par;
        if (in_lds) {
            uint32_t *tp = src; src = dst; dst = tp;
            const uint32_t tq = sp; sp = dp; dp = tq;
        } else if (out_lds) {
            in_lds = true;
            src = lds_a; sp = kPlaneA; dst = lds_b; dp = kPlaneB;
        }
    }
    Dig root{};
    if (t < 64) {
        Dig h;
#pragma unroll
        for (int k = 0; k < 8; k++) h.v[k] = t < cur ? src[k * sp + t] : 0u;
        const uint32_t ln0 = (2u * t) & 63u, ln1 = ln0 + 1u;
        while (cur > 1) {
            const uint32_t par = cur >> 1;
            Dig l, r;
#pragma unroll
            for (int k = 0; k < 8; k++) {
                l.v[k] = (uint32_t)__shfl((int)h.v[k], (int)ln0);
                r.v[k] = (uint32_t)__shfl((int)h.v[k], (int)ln1);
            }
            h = node_call<HF>(l, r);
            if (t < par) st_node<HF>(tree, row + cur + t, h.v);
            row += cur;
            cur = par;
        }
#pragma unroll
        for (int k = 0; k < 8; k++) root.v[k] = (uint32_t)__shfl((int)h.v[k], 0);
    }
    return root;
}

// ------------------------------------------------------------------------------ transforms in LDS
// Layers 0 .. nl - 1 of the transform of 2^m words in buf (forward: nl - 1 down to 0), two layers per barrier; twiddle
// layer i at tw[2^m - 2^(m-i)] (ss_p_twiddles).  The caller has synchronised after filling buf; ends synchronised.
template <bool INV>
__device__ __forceinline__ void fft_lds(uint32_t *buf, uint32_t m, uint32_t nl, const uint32_t *__restrict__ tw, uint32_t t)
{
    auto TW = [&](uint32_t i, uint32_t h) { return tw[(1u << m) - (1u << (m - i)) + h]; };
    auto bfly = [&](uint32_t &v0, uint32_t &v1, uint32_t w) {
        if (INV) {
            const uint32_t sum = m31_add_c(v0, v1);
            v1 = m31_mul_c(m31_sub_c(v0, v1), w);
            v0 = sum;
        } else {
            const uint32_t x = m31_mul_c(v1, w);
            v1 = m31_sub_c(v0, x);
            v0 = m31_add_c(v0, x);
        }
    };
    for (uint32_t done = 0; done < nl;) {
        if (nl - done >= 2) {
            const uint32_t a = INV ? done : nl - 2 - done;  // layers a and a + 1
            for (uint32_t q = t; q < (1u << (m - 2)); q += kNT) {
                const uint32_t hq = q >> a, j0 = (hq << (a + 2)) | (q & ((1u << a) - 1));
                uint32_t *p0 = buf + j0, *p1 = p0 + (1u << a), *p2 = p0 + (2u << a), *p3 = p1 + (2u << a);
                uint32_t v0 = *p0, v1 = *p1, v2 = *p2, v3 = *p3;
                const uint32_t wa0 = TW(a, 2 * hq), wa1 = TW(a, 2 * hq + 1), wb = TW(a + 1, hq);
                if (INV) {
                    bfly(v0, v1, wa0); bfly(v2, v3, wa1);
                    bfly(v0, v2, wb);  bfly(v1, v3, wb);
                } else {
                    bfly(v0, v2, wb);  bfly(v1, v3, wb);
                    bfly(v0, v1, wa0); bfly(v2, v3, wa1);
                }
                *p0 = v0; *p1 = v1; *p2 = v2; *p3 = v3;
            }
            done += 2;
        } else {
            const uint32_t ip = INV ? done : 0;  // the odd layer: last (inverse) or lowest (forward)
            for (uint32_t b = t; b < (1u << (m - 1)); b += kNT) {
                const uint32_t h = b >> ip, j0 = (h << (ip + 1)) | (b & ((1u << ip) - 1));
                uint32_t v0 = buf[j0], v1 = buf[j0 + (1u << ip)];
                bfly(v0, v1, TW(ip, h));
                buf[j0] = v0; buf[j0 + (1u << ip)] = v1;
            }
            done += 1;
        }
        __syncthreads();
    }
}

// out[2^m] <- the evaluations of the polynomial of 2^k coefficients src (k <= m) on the coset whose twiddles are tw
__device__ __forceinline__ void lde_column(uint32_t *buf, const uint32_t *src, uint32_t k, uint32_t m,
                                           const uint32_t *__restrict__ tw, uint32_t *out, uint32_t t)
{
    for (uint32_t j = t; j < (1u << m); j += kNT) buf[j] = src[j & ((1u << k) - 1)];
    __syncthreads();
    fft_lds<false>(buf, m, k, tw, t);
    for (uint32_t j = t; j < (1u << m); j += kNT) out[j] = buf[j];
    __syncthreads();
}

// ------------------------------------------------------------------------------ the kernel
template <int HF>
__global__ void __launch_bounds__(kNT) p_prove_small_kernel(SmallArgs A)
{
    __shared__ __attribute__((aligned(16))) uint32_t s_col[1u << kSmallLde];  // a column; between transforms level buffer A
    __shared__ __attribute__((aligned(16))) uint32_t s_lvl[8 * kPlaneB];      // level buffer B
    __shared__ SmallShared S;
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const uint32_t N = A.N, n = A.n, L = A.L, Q = A.Q, K = n - 1;
    const uint32_t rows = 1u << n, size = 1u << L, half = size >> 1, csize = 2u << n;
    const SmallSlot sl = small_slot(N, n, L);
    uint32_t *const slot = A.arena + (size_t)blockIdx.x * sl.total;
    uint32_t *const coefs = slot + sl.coefs, *const lde = slot + sl.lde, *const ev = slot + sl.ev, *const F = slot + sl.F;
    uint32_t *const cp_coefs = slot + sl.cp_coefs, *const cp_lde = slot + sl.cp_lde, *const pair_leaf = slot + sl.pair_leaf;
    uint32_t *const trace_tree = slot + sl.trace_tree, *const cp_tree = slot + sl.cp_tree;
    auto layer_at = [&](uint32_t l) { return slot + sl.layers + 4 * ((2u << L) - ((2u << L) >> l)); };
    auto fri_tree_at = [&](uint32_t l) { return slot + sl.fri_trees + 16 * ((2u << L) - ((2u << L) >> l)); };

    for (uint32_t proof = blockIdx.x; proof < A.count; proof += gridDim.x) {
        uint32_t *const rec = A.rec + (size_t)proof * A.row_stride;
        Channel<HF> ch;  // wavefront 0 only
        uint32_t errbits = 0;

        // ---- trace
        {
            const uint32_t seed_term = (uint32_t)(((A.seeds[proof] % M31_P) * (0x9E3779B1ull % M31_P)) % M31_P);
            for (uint32_t r = t; r < rows; r += kNT) trace_row(r, seed_term, N, rows, coefs);
        }
        __syncthreads();

        // ---- per column: circle iFFT, LDE to L, extension to n + 1
        {
            const uint32_t scale = (1u << ((31 - (n % 31)) % 31)) % M31_P;  // 2^-n
            for (uint32_t k = 0; k < N; k++) {
                uint32_t *col = coefs + k * rows;
                for (uint32_t j = t; j < rows; j += kNT) s_col[j] = col[j];
                __syncthreads();
                fft_lds<true>(s_col, n, n, A.tb.itw_n, t);
                for (uint32_t j = t; j < rows; j += kNT) {
                    const uint32_t v = m31_mul_c(s_col[j], scale);
                    s_col[j] = v;
                    col[j] = v;
                }
                __syncthreads();
                // (the coefficients are in LDS already: repeat them down the column in place)
                for (uint32_t j = rows + t; j < size; j += kNT) s_col[j] = s_col[j & (rows - 1)];
                __syncthreads();
                fft_lds<false>(s_col, L, n, A.tb.tw_l, t);
                for (uint32_t j = t; j < size; j += kNT) lde[k * size + j] = s_col[j];
                __syncthreads();
                lde_column(s_col, col, n, n + 1, A.tb.tw_c, ev + k * csize, t);
            }
        }

        // ---- trace commitment; channel begin, cp_alpha
        {
            const Dig root = build_tree<HF>(trace_tree, size, [&](uint32_t i) {
                Dig d;
                Hasher<HF>::template stream<false, 0>(nullptr, [&](uint32_t k) { return lde[k * size + i]; }, N, d.v);
                return d;
            }, s_col, s_lvl, t);
            if (wave == 0) {
                uint32_t r[8];
#pragma unroll
                for (int k = 0; k < 8; k++) r[k] = Hasher<HF>::native(root.v[k]);
                ch.init();
                ch.mix(A.const_root.v);
                ch.mix(r);
                QM31 a;
                if (!ch.draw_qm31(a)) errbits |= SS_P_ERR_TRANSCRIPT;
                if (t == 0) {
                    stq(S.cp_alpha, a);
#pragma unroll
                    for (int k = 0; k < 8; k++) S.troot[k] = r[k];
                }
            }
        }
        __syncthreads();

        // ---- composition polynomial on the coset of log size n + 1
        {
            const QM31 alpha = ldq(S.cp_alpha);
            for (uint32_t i = t; i < csize; i += kNT) composition_point(i, n, N, ev, A.tb.hxhy_c, alpha, F);
            __syncthreads();
            // its iFFT; coefficient j of coordinate c goes to partition 4 c + (j & 3), place j >> 2
            const uint32_t scale = (1u << ((31 - ((n + 1) % 31)) % 31)) % M31_P;
            for (uint32_t c = 0; c < 4; c++) {
                for (uint32_t j = t; j < csize; j += kNT) s_col[j] = F[c * csize + j];
                __syncthreads();
                fft_lds<true>(s_col, n + 1, n + 1, A.tb.itw_c, t);
                for (uint32_t j = t; j < csize; j += kNT)
                    cp_coefs[((4 * c + (j & 3)) << (n - 1)) + (j >> 2)] = m31_mul_c(s_col[j], scale);
                __syncthreads();
            }
            // x-only LDE: the transform of size L - 1 with the twiddles of layers 1.. of size L
            for (uint32_t p = 0; p < kCp; p++)
                lde_column(s_col, cp_coefs + (p << (n - 1)), n - 1, L - 1, A.tb.tw_l + half, cp_lde + p * half, t);
        }

        // ---- composition commitment (pair leaves, the duplicate level, the tree over the pairs); OODS point
        {
            const Dig root = build_tree<HF>(cp_tree, half, [&](uint32_t i) {
                Dig a, b;
#pragma unroll
                for (uint32_t k = 0; k < 8; k++) {
                    a.v[k] = Hasher<HF>::native(cp_lde[k * half + i]);
                    b.v[k] = Hasher<HF>::native(cp_lde[(8 + k) * half + i]);
                }
                const Dig pl = node_call<HF>(a, b);
                st_node<HF>(pair_leaf, i, pl.v);
                return node_call<HF>(pl, pl);
            }, s_col, s_lvl, t);
            if (wave == 0) {
                uint32_t r[8];
#pragma unroll
                for (int k = 0; k < 8; k++) r[k] = Hasher<HF>::native(root.v[k]);
                if (!oods_point<HF>(ch, r, n, t == 0, S.points, S.f1, S.f2x)) errbits |= SS_P_ERR_TRANSCRIPT;
                if (t == 0) {
#pragma unroll
                    for (int k = 0; k < 8; k++) S.croot[k] = r[k];
                }
            }
        }
        __syncthreads();

        // ---- the N + 16 samples (p_eval_tile_kernel): 256 threads fold one column, two columns at a time
        {
            const uint32_t grp = t >> 8, tid = t & 255u;
            const uint32_t cols = n > 1 ? N + kCp : N;
            for (uint32_t base = 0, it = 0; base < cols; base += 2, it++) {
                const uint32_t c = base + grp;
                const bool live = c < cols, tr = c < N;
                const uint32_t lv = tr ? n : n - 1, n_tile = 1u << lv, e0 = tid * 16;
                const uint32_t *src = (tr ? coefs + c * rows : cp_coefs + ((c - N) << (n - 1))) + e0;
                const uint32_t *fac = tr ? S.f1 : S.f2x;
                QM31 r = qm31_zero();
                if (live) {
                    uint32_t cf[16];
#pragma unroll
                    for (uint32_t k = 0; k < 16; k++) cf[k] = e0 + k < n_tile ? src[k] : 0u;
                    r = eval_fold16(cf, fac, lv);
                }
                r = eval_fold_wave(r, fac, live ? lv : 0u);  // (whole wavefronts: a group is four of them)
                if (lane == 0) S.wave[it & 1][wave] = r;
                __syncthreads();
                if (live && tid == 0) stq(S.samples + 4 * c, eval_fold_waves(r, &S.wave[it & 1][4 * grp], fac, lv));
            }
            if (n == 1 && t < kCp) stq(S.samples + 4 * (N + t), QM31{cp_coefs[t], 0, 0, 0});  // every partition is a constant
        }
        __syncthreads();

        // ---- deep_alpha and the DEEP coefficients (p_deep_coeffs_kernel), wavefront 0: N + 16 <= 48 columns, a lane each
        if (wave == 0) {
            mix_stream<HF>(ch, S.samples, 4 * (N + kCp), CompressCall<HF>());
            QM31 pw;
            if (!ch.draw_qm31(pw)) errbits |= SS_P_ERR_TRANSCRIPT;
            pw = alpha_powers(pw, lane);
            const QM31 py = ldq(S.points + 4), p2y = ldq(S.points + 12);
            auto batch = [&](bool mine, QM31 sp_y, uint32_t k, uint32_t *sums_out) {
                QM31 a = qm31_zero(), b = a, c = a;
                if (mine) {
                    deep_interpolant(sp_y, ldq(S.samples + 4 * k), pw, a, b, c);
                    stq(S.bcoef + 4 * k, b);
                }
                wave_sum2(a, c);
                if (lane == 0) { stq(sums_out, a); stq(sums_out + 4, c); }
            };
            batch(lane < N, py, lane, S.sums);
            batch(lane < kCp, p2y, N + lane, S.sums + 8);
            if (lane == kCp - 1) stq(S.sums + 16, pw);  // alpha^16
        }
        __syncthreads();

        // ---- quotients: a thread = a storage pair; the composition columns hold one value per pair (log size L - 1)
        {
            const QuotArgs qa = quot_args(S.points, S.sums);
            for (uint32_t h = t; h < half; h += kNT)
                quotients_pair(h, L, N, lde, cp_lde, L - 1, A.tb.hxhy_l, A.tb.hxhy_l + half, S.bcoef, qa, layer_at(0));
        }
        __syncthreads();

        // ---- FRI commit: per layer leaf hashes and tree, mix, alpha, fold
        for (uint32_t l = 0; l <= K; l++) {
            const uint32_t ln = size >> l;
            const uint32_t *cur = layer_at(l);
            const Dig root = build_tree<HF>(fri_tree_at(l), ln, [&](uint32_t i) {
                const QM31 v = ldq4(cur + 4 * i);
                const uint32_t e[4] = {v.a, v.b, v.c, v.d};
                Dig d;
                Hasher<HF>::template block<false, 0, 4>(nullptr, e, d.v);
                return d;
            }, s_col, s_lvl, t);
            if (wave == 0) {
                uint32_t r[8];
#pragma unroll
                for (int k = 0; k < 8; k++) r[k] = Hasher<HF>::native(root.v[k]);
                ch.mix(r);
                QM31 a;
                if (!ch.draw_qm31(a)) errbits |= SS_P_ERR_TRANSCRIPT;
                if (t == 0) {
                    stq(S.alpha, a);
#pragma unroll
                    for (int k = 0; k < 8; k++) S.roots[8 * l + k] = r[k];
                }
            }
            __syncthreads();
            const QM31 alpha = ldq(S.alpha);
            const uint32_t *cinv = A.tb.itw_l + (size - ln);  // inverse twiddle layer l = 1 / fold coordinate
            uint32_t *nxt = layer_at(l + 1);
            for (uint32_t i = t; i < (ln >> 1); i += kNT)
                stq4(nxt + 4 * i, fri_fold(ldq4(cur + 8 * i), ldq4(cur + 8 * i + 4), cinv[i], alpha));
            __syncthreads();
        }

        // ---- the transcript's tail: last layer, proof of work, queries
        {
            const uint32_t *last = layer_at(K + 1);
            const int differs = last_layer_differs(last, size >> (K + 1), t, kNT);
            if (wave == 0) {
                const QM31 first = ldq4(last);
                const uint32_t lv[4] = {first.a, first.b, first.c, first.d};
                ch.mix_values(lv);
                if (t == 0) {
#pragma unroll
                    for (int k = 0; k < 8; k++) S.dig[k] = ch.dig.v[k];  // native words
                    stq(S.last, first);
                    S.best = ~0ull;
                }
            }
            if (__syncthreads_or(differs)) errbits |= SS_P_ERR_LAST_LAYER;
            uint32_t dig[8];
#pragma unroll
            for (int k = 0; k < 8; k++) dig[k] = S.dig[k];
            const unsigned long long nonce = pow_search_workgroup<HF, false>(dig, A.target, A.span, &S.best, t, kNT);
            if (nonce == ~0ull) errbits |= SS_P_ERR_POW_SPAN;
            if (wave == 0) {
                if (nonce != ~0ull) {
                    const uint32_t nv[2] = {(uint32_t)(nonce >> 32), (uint32_t)nonce};
                    ch.mix_values(nv);
                    draw_queries<HF, false>(ch, L, Q, t == 0, S.queries);
                    if (t == 0) { S.nonce[0] = nv[0]; S.nonce[1] = nv[1]; }
                } else {
                    if (t < Q) S.queries[t] = 0;  // (the row's content is unspecified; its gather stays inside the slot)
                    if (t == 0) { S.nonce[0] = 0; S.nonce[1] = 0; }
                }
                if (t == 0) A.err[proof] = errbits;
            }
        }
        __syncthreads();

        // ---- decommitment into the row: a wavefront per chain, all threads for head and trailer
        {
            const uint32_t kinds = K + 3, head = record_head_words(N, K), per_q = N + kCp + 16 * L;
            const RecordHead hd = {A.const_root, S.troot, S.croot, S.samples, S.roots, S.last, S.nonce};
            for (uint32_t w = t; w < head; w += kNT) rec[w] = record_head_word(w, hd, N, K);
            uint32_t *plen = rec + stwo_record_words(N, L, Q, K) - (uint64_t)kinds * Q;
            for (uint32_t i = t; i < kinds * Q; i += kNT) plen[i] = record_path_len(i, L, Q);
            // The chains are record_chain (ss_prover_dev.h) on 32-bit rows and the slot's own pointers, written out: through
            // an ss_p_tree and 64-bit rows the Blake2s instance takes 236 VGPRs where this takes 233.
            for (uint32_t chain = wave; chain < kinds * Q; chain += kWaves) {
                const uint32_t kind = chain / Q, q = chain - kind * Q, idx = S.queries[q];
                const uint32_t *levels, *leaf = nullptr;
                uint32_t m, p, len, *dst;
                int first_lvl;
                if (kind == 0) {
                    uint32_t *s = rec + head + (size_t)q * per_q;
                    for (uint32_t c = lane; c < N; c += 64) s[c] = lde[c * size + idx];
                    levels = trace_tree; m = L; p = idx; len = L; first_lvl = 0; dst = s + N + kCp;
                } else if (kind == 1) {
                    uint32_t *s = rec + head + (size_t)q * per_q + N;
                    if (lane < kCp) s[lane] = cp_lde[lane * half + (idx >> 1)];
                    levels = cp_tree; leaf = pair_leaf; m = L - 1; p = idx >> 1; len = L; first_lvl = -1; dst = s + kCp + 8 * L;
                } else {
                    const uint32_t l = kind - 2;
                    len = L - 1 - l;
                    const uint32_t before = Q * (4 * l + 8 * (l * (L - 1) - l * (l - 1) / 2));  // layers 0 .. l-1
                    uint32_t *s = rec + head + (size_t)Q * per_q + before + (size_t)q * (4 + 8 * len);
                    levels = fri_tree_at(l); m = L - l; p = idx >> l; first_lvl = 1; dst = s + 4;
                    if (lane == 0) move16(s, layer_at(l) + (size_t)(p ^ 1) * 4);
                }
                const uint32_t two_n = 2u << m;
                for (uint32_t s = lane >> 1; s < len; s += 32) {
                    const int j = (int)s + first_lvl;
                    const uint32_t *src = j < 0 ? leaf + (size_t)p * 8 : levels + (size_t)(two_n - (two_n >> j) + ((p >> j) ^ 1)) * 8;
                    move16(dst + s * 8 + (lane & 1) * 4, src + (lane & 1) * 4);
                }
            }
        }
        __syncthreads();  // (the slot and the shared words are the next proof's from here on)
    }
}

bool small_cfg_ok(const ss_stwo_cfg *c)
{
    return c && stwo_cfg_ok(c->n_cols, c->trace_log, c->lde_log, c->n_queries, c->n_layers, c->mode) && c->hash <= 1 &&
           c->lde_log <= kSmallLde && c->n_cols <= kSmallCols && c->n_queries <= kSmallQueries && c->trace_log < c->lde_log &&
           c->n_layers + 1 == c->trace_log;
}

}  // namespace
}  // namespace ss

extern "C" void ss_p_small_limits(uint32_t *lde_log_out, uint32_t *n_cols_out, uint32_t *n_queries_out)
{
    if (lde_log_out) *lde_log_out = kSmallLde;
    if (n_cols_out) *n_cols_out = kSmallCols;
    if (n_queries_out) *n_queries_out = kSmallQueries;
}

extern "C" size_t ss_p_small_arena_words(const ss_stwo_cfg *cfg, size_t n_groups)
{
    if (!small_cfg_ok(cfg) || !n_groups) return 0;
    return (size_t)small_slot(cfg->n_cols, cfg->trace_log, cfg->lde_log).total * n_groups;
}

extern "C" int ss_p_prove_small_dev(ss_ctx *ctx, const ss_stwo_cfg *cfg, uint64_t pow_target, uint64_t pow_span,
                                    const uint64_t *seeds_dev, size_t n, size_t n_groups, const ss_p_small_tables *tables,
                                    const uint32_t const_root[8], uint32_t *arena_dev, size_t arena_words, uint32_t *records_out_dev,
                                    size_t row_stride_words, uint32_t *err_dev, void *stream)
{
    SS_DEVICE_GUARD(ctx);
    if (!small_cfg_ok(cfg))
        return ss_internal_set_err(SS_ERR_ARG, "ss_p_prove_small_dev: the shape is outside ss_p_small_limits");
    if (!n || n > 0x7fffffffu || n_groups > n || !pow_span || !seeds_dev || !tables || !const_root || !arena_dev ||
        !records_out_dev || !err_dev || ((uintptr_t)arena_dev & 15u) || ((uintptr_t)records_out_dev & 3u) ||
        row_stride_words < stwo_record_words(cfg->n_cols, cfg->lde_log, cfg->n_queries, cfg->n_layers) || !tables->itw_n ||
        !tables->tw_c || !tables->itw_c || !tables->hxhy_c || !tables->tw_l || !tables->itw_l || !tables->hxhy_l)
        return ss_internal_set_err(SS_ERR_ARG, "ss_p_prove_small_dev: bad argument");
    const size_t slot_words = small_slot(cfg->n_cols, cfg->trace_log, cfg->lde_log).total;
    if (!n_groups) n_groups = std::min(std::min<size_t>(n, kGroupsPerCu * (size_t)std::max(ctx->cus, 1)), arena_words / slot_words);
    if (!n_groups || arena_words / slot_words < n_groups)
        return ss_internal_set_err(SS_ERR_ARG, "ss_p_prove_small_dev: the arena is smaller than n_groups slots");
    SmallArgs a;
    a.N = cfg->n_cols; a.n = cfg->trace_log; a.L = cfg->lde_log; a.Q = cfg->n_queries; a.count = (uint32_t)n;
    a.target = pow_target; a.span = pow_span;
    for (int i = 0; i < 8; i++) a.const_root.v[i] = const_root[i];
    a.seeds = seeds_dev; a.arena = arena_dev; a.rec = records_out_dev; a.err = err_dev;
    a.row_stride = row_stride_words;
    a.tb = *tables;
    if (cfg->hash)
        hipLaunchKernelGGL(p_prove_small_kernel<1>, dim3((unsigned)n_groups), dim3(kNT), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(p_prove_small_kernel<0>, dim3((unsigned)n_groups), dim3(kNT), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return SS_OK;
}
