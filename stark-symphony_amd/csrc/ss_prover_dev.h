// The prover's protocol steps as device functions: the ONE definition of each, for every kernel that runs it.
//
// A step takes the index of its element as an argument.  A grid kernel (ss_prover.hip, ss_prover_transcript.hip) passes
// blockIdx.x * blockDim.x + threadIdx.x after its bounds check; the one-launch kernel (ss_prover_small.hip) passes the
// variable of its workgroup-stride loop; the resident FRI and proof-of-work kernels use the helpers.  Where the step
// runs and where its operands live (HBM, LDS, registers) is the caller's business; what it computes is here.
// All arithmetic is exact M31 / QM31 on canonical words, so any evaluation order gives the bits of tools/stwo_prover.py.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ss_prover.h"
#include "ss_channel.h"
#include "ss_fields.h"
#include "ss_hash.h"
#include "ss_layout.h"

namespace ss {

// ---------------------------------------------------------------------------------- words, lanes
__device__ __forceinline__ QM31 ldq(const uint32_t *p) { return QM31{p[0], p[1], p[2], p[3]}; }
__device__ __forceinline__ void stq(uint32_t *p, QM31 v) { p[0] = v.a; p[1] = v.b; p[2] = v.c; p[3] = v.d; }
// the same through one 16-byte access: p is 16-byte aligned
__device__ __forceinline__ QM31 ldq4(const uint32_t *p)
{
    const uint4 v = *reinterpret_cast<const uint4 *>(p);
    return QM31{v.x, v.y, v.z, v.w};
}
__device__ __forceinline__ void stq4(uint32_t *p, QM31 v) { *reinterpret_cast<uint4 *>(p) = make_uint4(v.a, v.b, v.c, v.d); }

// 16 bytes from an aligned source to a slot of a record, which is aligned or not as a whole
__device__ __forceinline__ void move16(uint32_t *dst, const uint32_t *src)
{
    const uint4 v = *reinterpret_cast<const uint4 *>(src);
    if (((uintptr_t)dst & 15) == 0) {
        *reinterpret_cast<uint4 *>(dst) = v;
    } else {
        dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; dst[3] = v.w;
    }
}

__device__ __forceinline__ QM31 q_shfl_down(QM31 v, uint32_t d)
{
    return {__shfl_down(v.a, d, 64), __shfl_down(v.b, d, 64), __shfl_down(v.c, d, 64), __shfl_down(v.d, d, 64)};
}
__device__ __forceinline__ QM31 q_shfl_up(QM31 v, uint32_t d)
{
    return {__shfl_up(v.a, d, 64), __shfl_up(v.b, d, 64), __shfl_up(v.c, d, 64), __shfl_up(v.d, d, 64)};
}
__device__ __forceinline__ QM31 lane_q(QM31 v, uint32_t src)
{
    return QM31{(uint32_t)__shfl((int)v.a, (int)src), (uint32_t)__shfl((int)v.b, (int)src),
                (uint32_t)__shfl((int)v.c, (int)src), (uint32_t)__shfl((int)v.d, (int)src)};
}
// a value that is the same in every lane, moved to a scalar register
__device__ __forceinline__ uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

// ---------------------------------------------------------------------------------- tree nodes
// a node in the hash's native words -> row `row` of a tree, in stored words; and back
template <int HF>
__device__ __forceinline__ void st_node(uint32_t *tree, size_t row, const uint32_t (&d)[8])
{
    uint4 *o = reinterpret_cast<uint4 *>(tree + row * 8);
    o[0] = make_uint4(Hasher<HF>::native(d[0]), Hasher<HF>::native(d[1]), Hasher<HF>::native(d[2]), Hasher<HF>::native(d[3]));
    o[1] = make_uint4(Hasher<HF>::native(d[4]), Hasher<HF>::native(d[5]), Hasher<HF>::native(d[6]), Hasher<HF>::native(d[7]));
}
template <int HF>
__device__ __forceinline__ Dig ld_node(const uint32_t *tree, size_t row)
{
    const uint4 *c = reinterpret_cast<const uint4 *>(tree + row * 8);
    const uint4 a = c[0], b = c[1];
    return Dig{{Hasher<HF>::native(a.x), Hasher<HF>::native(a.y), Hasher<HF>::native(a.z), Hasher<HF>::native(a.w),
                Hasher<HF>::native(b.x), Hasher<HF>::native(b.y), Hasher<HF>::native(b.z), Hasher<HF>::native(b.w)}};
}

// ---------------------------------------------------------------------------------- channel state
// state = 8 STORED digest words + the draw counter, in device memory between two kernels
template <int HF>
__device__ __forceinline__ void channel_load(Channel<HF> &ch, const uint32_t *state)
{
#pragma unroll
    for (int i = 0; i < 8; i++) ch.dig.v[i] = Hasher<HF>::native(state[i]);
    ch.ctr = state[8];
}
template <int HF>
__device__ __forceinline__ void channel_store(const Channel<HF> &ch, uint32_t *state)
{
#pragma unroll
    for (int i = 0; i < 8; i++) state[i] = Hasher<HF>::native(ch.dig.v[i]);
    state[8] = ch.ctr;
}

// The compression of mix_stream: inlined where one kernel has one stream hash, the out-of-line copy of ss_hash.h where
// a kernel holds many hashes and code size counts.  The choice is the kernel's.
template <int HF>
struct CompressInline {
    __device__ __forceinline__ void operator()(Dig &st, W16 &w, uint32_t blk, uint32_t nblk, uint32_t total) const
    {
        Hasher<HF>::compress(st, w, blk, nblk, total);
    }
};
template <int HF>
struct CompressCall {
    __device__ __forceinline__ void operator()(Dig &st, W16 &w, uint32_t blk, uint32_t nblk, uint32_t total) const
    {
        if (HF) {
            const bool last = blk + 1 == nblk;
            st = b2s_compress_call(st, w, last ? 4u * total : 64u * (blk + 1), last);
        } else {
            st = sha_compress_call(st, w);
        }
    }
};
// channel_mix_oods_evals (deep/oods.simf:23-39): digest <- H(digest || words[0 .. count)) for a message of any length,
// a runtime-length stream hash around one compression; then num_sent = 0
template <int HF, class Compress>
__device__ __forceinline__ void mix_stream(Channel<HF> &ch, const uint32_t *words, uint32_t count, Compress compress)
{
    const uint32_t total = 8 + count, nblk = Hasher<HF>::n_blocks(total);
    Dig st;
    Hasher<HF>::iv(st.v);
    for (uint32_t blk = 0; blk < nblk; blk++) {
        W16 w;
        Hasher<HF>::fill(w, blk, nblk, total, ch.dig.v, [&](int, uint32_t i) { return words[i]; });
        compress(st, w, blk, nblk, total);
    }
    ch.dig = st;
    ch.ctr = 0;
}

// ---------------------------------------------------------------------------------- trace
// row r of the wide-Fibonacci trace into out[n_cols][rows]: 1, r + seed term, c_k = c_{k-1}^2 + c_{k-2}^2
__device__ __forceinline__ void trace_row(uint32_t r, uint32_t seed_term, uint32_t n_cols, uint32_t rows, uint32_t *__restrict__ out)
{
    uint32_t a = 1, b = m31_add(m31_red(r), seed_term);
    out[r] = a;
    if (n_cols > 1) out[(size_t)rows + r] = b;
    for (uint32_t k = 2; k < n_cols; k++) {
        const uint32_t c = m31_add(m31_sqr(b), m31_sqr(a));
        out[(size_t)k * rows + r] = c;
        a = b;
        b = c;
    }
}

// ---------------------------------------------------------------------------------- composition
// point i of the composition polynomial on the coset of log size n_log + 1: ev[n_cols][size] -> out[4][size]
__device__ __forceinline__ void composition_point(uint32_t i, uint32_t n_log, uint32_t n_cols, const uint32_t *__restrict__ ev,
                                                  const uint32_t *__restrict__ hx, QM31 alpha, uint32_t *__restrict__ out)
{
    const uint32_t size = 1u << (n_log + 1);
    uint32_t van = hx[i >> 1];
    for (uint32_t k = 1; k < n_log; k++) van = m31_dbl_x(van);
    uint32_t van_inv;
    m31_inv(van, van_inv);
    QM31 acc = qm31_zero();
    uint32_t a = ev[i], b = n_cols > 1 ? ev[(size_t)size + i] : 0;
    for (uint32_t k = 2; k < n_cols; k++) {
        const uint32_t c = ev[(size_t)k * size + i];
        const uint32_t cons = m31_sub(c, m31_add(m31_sqr(b), m31_sqr(a)));
        acc = qm31_mul(acc, alpha);
        acc.a = m31_add(acc.a, cons);
        a = b;
        b = c;
    }
    out[i] = m31_mul(acc.a, van_inv);
    out[(size_t)size + i] = m31_mul(acc.b, van_inv);
    out[(size_t)2 * size + i] = m31_mul(acc.c, van_inv);
    out[(size_t)3 * size + i] = m31_mul(acc.d, van_inv);
}

// ---------------------------------------------------------------------------------- OODS point and fold factors
// One lane's work: mix the composition root (stored words), channel_draw_qm31_point (channel.simf:143-151), then the
// factor chains x -> pi(x) = 2 x^2 - 1 of P (behind y) and of 2P (no y: the composition columns are held compact).
// A lane with `store` writes points[16] = px, py, p2x, p2y, fp[trace_log][4] and f2p[trace_log - 1][4].  -> drawn?
template <int HF>
__device__ __forceinline__ bool oods_point(Channel<HF> &ch, const uint32_t (&cp_root)[8], uint32_t trace_log, bool store,
                                           uint32_t *points, uint32_t *fp, uint32_t *f2p)
{
    ch.mix(cp_root);
    QM31 t, inv;
    bool ok = ch.draw_qm31(t);
    const QM31 t_sq = qm31_mul(t, t);
    ok &= qm31_inv(qm31_add(qm31_one(), t_sq), inv);
    const QM31 px = qm31_mul(qm31_sub(qm31_one(), t_sq), inv), py = qm31_mul(qm31_add(t, t), inv);
    const QM31 p2x = qm31_dbl_x(px), pxy = qm31_mul(px, py), p2y = qm31_add(pxy, pxy);
    if (store) {
        stq(points, px); stq(points + 4, py); stq(points + 8, p2x); stq(points + 12, p2y);
        stq(fp, py);
        QM31 cur = px;
        for (uint32_t i = 1; i < trace_log; i++) { stq(fp + 4 * i, cur); cur = qm31_dbl_x(cur); }
        cur = p2x;
        for (uint32_t i = 0; i + 1 < trace_log; i++) { stq(f2p + 4 * i, cur); cur = qm31_dbl_x(cur); }
    }
    return ok;
}

// ---------------------------------------------------------------------------------- evaluation at a point, tiled
// A column's value at the point is the fold of its coefficients: level l replaces the pairs (v[2j], v[2j+1]) by
// v[2j] + f_l v[2j+1], f_l = fac[4 l ..].  A tile of 2^lv <= 2^12 elements is folded by 256 lanes, 16 elements each:
// levels 0..3 in registers, 4..9 between the lanes of a wavefront, 10 and 11 across the four wavefronts.  Levels at
// and above lv are skipped (their factors do not exist); the elements past the tile are zeros.
__device__ __forceinline__ QM31 fold_q(QM31 even, QM31 odd, QM31 f) { return qm31_add_c(even, qm31_mul_c(odd, f)); }

// levels 1..3: eight QM31 -> one
__device__ __forceinline__ QM31 eval_fold8(QM31 (&v)[8], const uint32_t *fac, uint32_t lv)
{
#pragma unroll
    for (uint32_t s = 1; s < 4; s++) {
        if (s < lv) {
            const QM31 f = ldq(fac + 4 * s);
#pragma unroll
            for (uint32_t j = 0; j < (8u >> s); j++) v[j] = fold_q(v[2 * j], v[2 * j + 1], f);
        }
    }
    return v[0];
}
// levels 0..3: sixteen M31 words -> one QM31 (level 0 is M31 x QM31-factor)
__device__ __forceinline__ QM31 eval_fold16(const uint32_t (&c)[16], const uint32_t *fac, uint32_t lv)
{
    const QM31 f0 = ldq(fac);
    QM31 v[8];
#pragma unroll
    for (uint32_t j = 0; j < 8; j++) {
        const uint32_t o = c[2 * j + 1];
        v[j] = QM31{m31_add_c(m31_mul_c(f0.a, o), c[2 * j]), m31_mul_c(f0.b, o), m31_mul_c(f0.c, o), m31_mul_c(f0.d, o)};
    }
    return eval_fold8(v, fac, lv);
}
// levels 4..9: lane i takes lane i + 2^s's value; after level 4 + s only the lanes that are multiples of 2^(s+1) hold
// live values (the others compute on, unread), so lane 0 ends with the wavefront's 1024 elements.  Whole wavefronts
// call it, with one lv.
__device__ __forceinline__ QM31 eval_fold_wave(QM31 r, const uint32_t *fac, uint32_t lv)
{
#pragma unroll
    for (uint32_t s = 0; s < 6; s++) {
        const QM31 up = q_shfl_down(r, 1u << s);
        if (4 + s < lv) r = fold_q(r, up, ldq(fac + 4 * (4 + s)));
    }
    return r;
}
// levels 10, 11: r = lane 0's value of the tile's first wavefront, w[1..3] = those of the others
__device__ __forceinline__ QM31 eval_fold_waves(QM31 r, const QM31 *w, const uint32_t *fac, uint32_t lv)
{
    if (lv > 10) {
        const QM31 f10 = ldq(fac + 40);
        r = fold_q(r, w[1], f10);
        if (lv > 11) r = fold_q(r, fold_q(w[2], w[3], f10), ldq(fac + 44));
    }
    return r;
}

// ---------------------------------------------------------------------------------- DEEP coefficients
// deep/quotients.simf:25-36 on canonical values: a0 = -2 Im(v) u, b0 = -2 Im(y) u, c0 = b0 v - a0 y, times alpha^i
__device__ __forceinline__ void deep_interpolant(QM31 sp_y, QM31 v, QM31 alpha_i, QM31 &a, QM31 &b, QM31 &c)
{
    auto neg2 = [](uint32_t x) { return m31_sub_c(0, m31_add_c(x, x)); };
    const CM31 a0 = {neg2(v.c), neg2(v.d)}, b0 = {neg2(sp_y.c), neg2(sp_y.d)};
    const QM31 c0 = qm31_sub(qm31_mul_im_c(v, b0), qm31_mul_im_c(sp_y, a0));
    a = qm31_mul_im_c(alpha_i, a0);
    b = qm31_mul_im_c(alpha_i, b0);
    c = qm31_mul_c(alpha_i, c0);
}
// every lane of a wavefront holds alpha -> lane i holds alpha^(i + 1): an inclusive prefix product in six doubling steps
__device__ __forceinline__ QM31 alpha_powers(QM31 pw, uint32_t lane)
{
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const QM31 below = q_shfl_up(pw, d);
        if (lane >= d) pw = qm31_mul_c(pw, below);
    }
    return pw;
}
// a, c <- their sums over the wavefront, in lane 0
__device__ __forceinline__ void wave_sum2(QM31 &a, QM31 &c)
{
#pragma unroll
    for (uint32_t d = 32; d; d >>= 1) {
        a = qm31_add_c(a, q_shfl_down(a, d));
        c = qm31_add_c(c, q_shfl_down(c, d));
    }
}

// ---------------------------------------------------------------------------------- quotients
struct QuotArgs {
    QM31 px, py, p2x, p2y, a1, c1, a2, c2, alpha16;
};
// points: px, py, p2x, p2y as oods_point writes them; sums: A1, C1, A2, C2, alpha^16.  The 36 addresses do not depend
// on the lane.
__device__ __forceinline__ QuotArgs quot_args(const uint32_t *points, const uint32_t *sums)
{
    QuotArgs q;
    q.px = ldq(points); q.py = ldq(points + 4); q.p2x = ldq(points + 8); q.p2y = ldq(points + 12);
    q.a1 = ldq(sums); q.c1 = ldq(sums + 4); q.a2 = ldq(sums + 8); q.c2 = ldq(sums + 12); q.alpha16 = ldq(sums + 16);
    return q;
}

// The DEEP quotients of the storage pair (2h, 2h+1): the two positions share x and have y, -y.  The column sums are
// open 64-bit multiply-accumulates (one v_mad_u64_u32 per product, folded every third product, reduced once per word);
// the four DEEP denominators (two sample points x two positions) share ONE M31 inversion.  All operands are canonical
// field elements, so every re-association gives the bits of the straightforward evaluation (which
// tools/stwo_prover.py performs).  bcoef[n_cols + 16][4] is 16-byte aligned; out[2^lde_log][4].
__device__ __forceinline__ void
quotients_pair(size_t h, uint32_t lde_log, uint32_t n_cols, const uint32_t *__restrict__ trace_lde,
               const uint32_t *__restrict__ cp_lde, uint32_t cp_log, const uint32_t *__restrict__ hx,
               const uint32_t *__restrict__ hy, const uint32_t *__restrict__ bcoef, const QuotArgs &q,
               uint32_t *__restrict__ out)
{
    const size_t size = (size_t)1 << lde_log;
    const uint32_t x = hx[h], y0 = hy[h];
    const uint32_t ys[2] = {y0, m31_sub_c(0, y0)};
    // s[batch][position] = sum_k b_k v_k
    // (pairs = false: a column that depends on x only holds ONE value per storage pair, stride size / 2)
    auto dot = [&](const uint32_t *lde, const uint32_t *coef, uint32_t count, bool pairs, QM31 (&res)[2]) {
        uint64_t acc[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
        uint32_t open = 0;
        for (uint32_t k = 0; k < count; k++) {
            uint2 v;
            if (pairs) v = *reinterpret_cast<const uint2 *>(lde + (size_t)k * size + 2 * h);
            else v.x = v.y = lde[(size_t)k * (size >> 1) + h];
            const uint4 c = *reinterpret_cast<const uint4 *>(coef + 4 * k);
            acc[0][0] = m31_mac(acc[0][0], c.x, v.x); acc[0][1] = m31_mac(acc[0][1], c.y, v.x);
            acc[0][2] = m31_mac(acc[0][2], c.z, v.x); acc[0][3] = m31_mac(acc[0][3], c.w, v.x);
            if (pairs) {  // (one value per pair: the second sum is the first)
                acc[1][0] = m31_mac(acc[1][0], c.x, v.y); acc[1][1] = m31_mac(acc[1][1], c.y, v.y);
                acc[1][2] = m31_mac(acc[1][2], c.z, v.y); acc[1][3] = m31_mac(acc[1][3], c.w, v.y);
            }
            if (++open == 3) {
#pragma unroll
                for (int p = 0; p < 2; p++)
#pragma unroll
                    for (int w = 0; w < 4; w++) acc[p][w] = m31_fold62(acc[p][w]);
                open = 0;
            }
        }
#pragma unroll
        for (int p = 0; p < 2; p++)
            res[p] = QM31{m31_red64(acc[p][0]), m31_red64(acc[p][1]), m31_red64(acc[p][2]), m31_red64(acc[p][3])};
        if (!pairs) res[1] = res[0];
    };
    QM31 s1[2], s2[2];
    dot(trace_lde, bcoef, n_cols, true, s1);
    dot(cp_lde, bcoef + 4 * n_cols, kCp, cp_log == lde_log, s2);
    // deep_quotient_denominator_inverse (deep/quotients.simf:15-22) for (P, 2P) x (y, -y)
    CM31 d[4];
    uint32_t nrm[4], pre[4];
    uint32_t run = 1;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const QM31 sx = j < 2 ? q.px : q.p2x, sy = j < 2 ? q.py : q.p2y;
        const CM31 dx = cm31_sub_m31(q_re(sx), x), dy = cm31_sub_m31(q_re(sy), ys[j & 1]);
        d[j] = cm31_sub(cm31_mul(dx, q_im(sy)), cm31_mul(dy, q_im(sx)));
        nrm[j] = m31_add(m31_sqr(d[j].a), m31_sqr(d[j].b));
        pre[j] = run;
        run = m31_mul(run, nrm[j] ? nrm[j] : 1u);  // a zero norm inverts to 0, as cm31_inv gives
    }
    uint32_t inv;
    m31_inv(run, inv);
    CM31 dinv[4];
#pragma unroll
    for (int j = 3; j >= 0; j--) {
        const uint32_t ni = nrm[j] ? m31_mul(inv, pre[j]) : 0u;
        inv = m31_mul(inv, nrm[j] ? nrm[j] : 1u);
        dinv[j] = cm31_mul_m31(CM31{d[j].a, m31_neg(d[j].b)}, ni);
    }
    const QM31 a1y = qm31_mul_m31(q.a1, y0), a2y = qm31_mul_m31(q.a2, y0);
#pragma unroll
    for (int p = 0; p < 2; p++) {
        // a * (-y) = -(a * y)
        const QM31 t1 = p ? qm31_sub(q.c1, a1y) : qm31_add(a1y, q.c1);
        const QM31 t2 = p ? qm31_sub(q.c2, a2y) : qm31_add(a2y, q.c2);
        const QM31 b1 = qm31_mul_cm31(qm31_sub(s1[p], t1), dinv[p]);
        const QM31 b2 = qm31_mul_cm31(qm31_sub(s2[p], t2), dinv[2 + p]);
        stq(out + 4 * (2 * h + p), qm31_add(qm31_mul(b1, q.alpha16), b2));
    }
}

// ---------------------------------------------------------------------------------- FRI fold
__device__ __forceinline__ QM31 fri_fold(QM31 v0, QM31 v1, uint32_t cinv, QM31 alpha)
{
    const QM31 f0 = qm31_add(v0, v1);
    const QM31 f1 = qm31_mul_m31(qm31_sub(v0, v1), cinv);
    return qm31_add(f0, qm31_mul(f1, alpha));
}

// ---------------------------------------------------------------------------------- the transcript's tail
// thread t of nt: does any of its rows of last[n_last][4] (16-byte aligned) differ from row 0?  (the caller ORs the threads)
__device__ __forceinline__ int last_layer_differs(const uint32_t *last, size_t n_last, uint32_t t, uint32_t nt)
{
    const QM31 first = ldq4(last);
    int differs = 0;
    for (size_t i = t; i < n_last; i += nt) differs |= !qm31_eq(ldq4(last + 4 * i), first);
    return differs;
}

// The smallest nonce in [0, span) with pow_value(H(dig || be8(nonce))) < target, or ~0, by a workgroup of nt threads
// (every one calls it, with the same native digest): thread t tries base + t, one block of nt nonces per round.  The
// smallest hit of a round is taken by a 64-bit min in LDS (*best = ~0 before the call, and a barrier behind that);
// rounds are tried in ascending order, so the first round with a hit holds the smallest nonce of all.
// INL: the block hash inlined, or through the out-of-line compressions of ss_hash.h.
template <int HF, bool INL>
__device__ __forceinline__ unsigned long long pow_search_workgroup(const uint32_t (&dig)[8], uint64_t target, uint64_t span,
                                                                   unsigned long long *best, uint32_t t, uint32_t nt)
{
    unsigned long long nonce = ~0ull;
    for (uint64_t base = 0; base < span; base += nt) {
        const uint64_t cand = base + t;
        if (cand < span) {
            const uint32_t m[2] = {(uint32_t)(cand >> 32), (uint32_t)cand};
            uint32_t d[8];
            Hasher<HF>::template block<INL, 8, 2>(dig, m, d);
            if (Hasher<HF>::pow_value(d) < target) atomicMin(best, (unsigned long long)cand);
        }
        __syncthreads();
        nonce = *best;
        __syncthreads();  // (nobody enters the next round's atomicMin before everybody has read this round's result)
        if (nonce != ~0ull) break;
    }
    return nonce;
}

// the n_queries positions of lde_log bits, eight per draw; a lane with `store` writes them
template <int HF, bool INL>
__device__ __forceinline__ void draw_queries(Channel<HF> &ch, uint32_t lde_log, uint32_t n_queries, bool store, uint32_t *queries)
{
    const uint32_t mask = (uint32_t)(((uint64_t)1 << lde_log) - 1);
    for (uint32_t got = 0; got < n_queries; got += 8) {
        uint32_t w[8];
        if (INL) {  // Channel<HF>::draw_words around an inlined block hash
            const uint32_t m[1] = {ch.ctr};
            Hasher<HF>::template block<true, 8, 1>(ch.dig.v, m, w);
            ch.ctr = ch.ctr + 1;
#pragma unroll
            for (int i = 0; i < 8; i++) w[i] = Hasher<HF>::native(w[i]);
        } else {
            ch.draw_words(w);
        }
        if (store) {
#pragma unroll
            for (uint32_t k = 0; k < 8; k++)
                if (got + k < n_queries) queries[got + k] = w[k] & mask;
        }
    }
}

// ---------------------------------------------------------------------------------- the record
// A record is head | per query: trace values, composition values, two chains | per FRI layer and query: the fold
// partner and a chain | the path_len trailer (ss_layout.h).
struct RecordHead {
    Dig const_root;  // stored words
    const uint32_t *troot, *croot, *samples, *fri_roots, *last, *nonce;
};
__device__ __forceinline__ uint32_t record_head_words(uint32_t N, uint32_t K) { return 24 + 4 * (N + kCp) + 8 * (K + 1) + 6; }
// word w of the head: roots, samples, FRI roots, last layer, nonce
__device__ __forceinline__ uint32_t record_head_word(uint32_t w, const RecordHead &src, uint32_t N, uint32_t K)
{
    const uint32_t oods = 4 * (N + kCp);
    uint32_t v = 0, r = w;
    if (r < 8) {
#pragma unroll
        for (uint32_t k = 0; k < 8; k++)  // (a kernel argument: selected, not indexed)
            if (r == k) v = src.const_root.v[k];
    }
    else if ((r -= 8) < 8) v = src.troot[r];
    else if ((r -= 8) < 8) v = src.croot[r];
    else if ((r -= 8) < oods) v = src.samples[r];
    else if ((r -= oods) < 8 * (K + 1)) v = src.fri_roots[r];
    else if ((r -= 8 * (K + 1)) < 4) v = src.last[r];
    else v = src.nonce[r - 4];
    return v;
}
// entry i of the path_len trailer [K + 3][Q]
__device__ __forceinline__ uint32_t record_path_len(uint32_t i, uint32_t L, uint32_t Q)
{
    const uint32_t kind = i / Q;
    return kind < 2 ? L : L + 1 - kind;
}
// One wavefront moves the authentication chain of tree `kind` (0 trace, 1 composition, 2 + l FRI layer l, described by
// `tree`) at query q, position idx, and the chain's queried values (kind 0: the N trace columns at idx, strided over
// the lanes; kind 1: the 16 composition values of idx's pair; FRI: the 4-word fold partner).  A chain is at most L
// siblings of 32 bytes, and a lane owns half a sibling: lane 2 * level + half computes its source row from the query
// (level j of a tree of n leaves starts at row 2n - (2n >> j), the sibling of position p there is (p >> j) ^ 1) and
// moves one uint4.  64 lanes = 32 levels >= the layout's bound of 31, so the level loop runs once.
__device__ __forceinline__ void record_chain(uint32_t kind, uint32_t q, uint32_t idx, uint32_t lane, const ss_p_tree &tree,
                                             uint32_t N, uint32_t L, uint32_t Q, uint32_t K, uint32_t *rec)
{
    const uint32_t head = record_head_words(N, K), per_q = N + kCp + 16 * L;
    // the chain's tree has 2^m leaves, the chain enters it at position p, and its sibling s is tree level s + first
    // (composition: sibling 0 is the pair's other leaf, the same hash, and the tree over the pairs starts above it)
    uint32_t m, p, len, *dst;
    int first;
    if (kind == 0) {
        uint32_t *slot = rec + head + (size_t)q * per_q;
        for (uint32_t c = lane; c < N; c += 64) slot[c] = tree.values[((size_t)c << L) + idx];
        m = L; p = idx; len = L; first = 0; dst = slot + N + kCp;
    } else if (kind == 1) {
        uint32_t *slot = rec + head + (size_t)q * per_q + N;
        if (lane < kCp) slot[lane] = tree.values[((size_t)lane << (L - 1)) + (idx >> 1)];
        m = L - 1; p = idx >> 1; len = L; first = -1; dst = slot + kCp + 8 * L;
    } else {
        const uint32_t l = kind - 2;
        len = L - 1 - l;
        // layers 0 .. l-1 hold Q (4 + 8 (L - 1 - l')) words each
        const uint32_t before = Q * (4 * l + 8 * (l * (L - 1) - l * (l - 1) / 2));
        uint32_t *slot = rec + head + (size_t)Q * per_q + before + (size_t)q * (4 + 8 * len);
        m = L - l; p = idx >> l; first = 1; dst = slot + 4;
        if (lane == 0) move16(slot, tree.values + (size_t)(p ^ 1) * 4);
    }
    const uint64_t two_n = (uint64_t)2 << m;
    for (uint32_t s = lane >> 1; s < len; s += 32) {
        const int j = (int)s + first;
        const uint32_t *src = j < 0 ? tree.leaf + (size_t)p * 8 : tree.levels + (two_n - (two_n >> j) + ((p >> j) ^ 1)) * 8;
        move16(dst + s * 8 + (lane & 1) * 4, src + (lane & 1) * 4);
    }
}

}  // namespace ss
