// The prover's Fiat-Shamir transcript up to the FRI commit, on the device (include/ss_prover_transcript.h).
//
// prover.py used to leave HIP three times before the FRI commit: to draw cp_alpha, to draw the OODS point and prepare
// the fold factors of the samples, and to draw deep_alpha and compute the DEEP line coefficients.  The kernels here do
// that work where the data is: two single-lane channel steps (the pattern of p_channel_fri_layer_kernel), the tiled
// evaluation of all columns at the OODS point, and one workgroup for the O(columns) QM31 algebra of the quotients.
// All arithmetic is exact M31 / QM31 on canonical words, so any evaluation order gives the bits of the host route.
#include <hip/hip_runtime.h>

#include "../../include/ss_prover.h"
#include "ss_ctx.h"
#include "ss_prover_dev.h"

using namespace ss;

extern "C" int ss_internal_set_err(int code, const char *msg);

namespace ss {
namespace {

// ------------------------------------------------------------------------ 1. begin: roots, cp_alpha
// evals_commit (evals/commit.simf:20-35) by one lane: two mixes and a draw are three to four dependent compressions.
template <int HF>
__global__ void p_channel_begin_kernel(Dig const_root, const uint32_t *__restrict__ trace_root, uint32_t *__restrict__ state,
                                       uint32_t *__restrict__ alpha_out, uint32_t *__restrict__ err)
{
    if (blockIdx.x || threadIdx.x) return;
    Channel<HF> ch;
    ch.init();
    ch.mix(const_root.v);
    uint32_t r[8];
    for (int i = 0; i < 8; i++) r[i] = trace_root[i];
    ch.mix(r);
    QM31 a;
    if (!ch.draw_qm31(a)) atomicOr(err, SS_P_ERR_TRANSCRIPT);
    stq(alpha_out, a);
    channel_store(ch, state);
}

// ------------------------------------------------------------------------ 3. OODS point and fold factors
// One lane runs oods_point (ss_prover_dev.h).
template <int HF>
__global__ void p_oods_point_kernel(uint32_t trace_log, uint32_t *__restrict__ state, const uint32_t *__restrict__ cp_root,
                                    uint32_t *__restrict__ points, uint32_t *__restrict__ fp, uint32_t *__restrict__ f2p,
                                    uint32_t *__restrict__ err)
{
    if (blockIdx.x || threadIdx.x) return;
    Channel<HF> ch;
    channel_load(ch, state);
    uint32_t r[8];
    for (int i = 0; i < 8; i++) r[i] = cp_root[i];
    if (!oods_point<HF>(ch, r, trace_log, true, points, fp, f2p)) atomicOr(err, SS_P_ERR_TRANSCRIPT);
    channel_store(ch, state);
}

// ------------------------------------------------------------------------ 4. evaluation at a point, tiled
// A column's value at the point is the fold of its 2^m coefficients: level l replaces the pairs (v[2j], v[2j+1]) by
// v[2j] + f_l v[2j+1].  The chain of ss_p_eval_at_point_batch runs one launch per level over 3 * 2^m words of scratch per
// column; here a workgroup owns a contiguous TILE of 2^T elements of one column (T = 12: 16 KB of coefficients; grid =
// tiles x columns) and folds it to one QM31 without leaving the CU:
//   levels 0..3   in registers: a lane loads 16 consecutive elements (four uint4 of M31 words) and folds them to one
//                 QM31 -- level 0 is M31 x QM31-factor, the rest QM31 x QM31;
//   levels 4..9   between the lanes of the wavefront: lane i takes lane i + 2^s's value by a ds_bpermute-style
//                 exchange (__shfl_down); after level 4 + s only the lanes that are multiples of 2^(s+1) hold live
//                 values (the others compute on, unread), so lane 0 ends with the wavefront's 1024 elements;
//   levels 10, 11 across the four wavefronts through 64 bytes of LDS, by thread 0.
// The tile's QM31 goes to scratch and a second launch of the SAME kernel in QM31-input mode (QIN) folds the 2^(m-T)
// partials with the factors T.. (and a third one beyond m = 24): ceil(m / T) launches where there were m, and
// ncols * 2^(m-T) QM31 of scratch.  A tile of fewer than 2^T elements (m <= T, or the last launch) is zero-filled and
// its levels at and above `lv` are skipped: their factors do not exist.
// Every operand is a canonical field element and every helper returns the canonical word of the exact field result, so
// this association gives the bits that ss_p_eval_at_point_batch (and tools/stwo_prover.py) give.
constexpr uint32_t kEvalT = SS_P_EVAL_TILE_LOG, kEvalThreads = 256, kEvalPerLane = 16;
static_assert(kEvalThreads * kEvalPerLane == 1u << kEvalT, "a lane holds 16 elements of the tile");

template <bool QIN>
__global__ void __launch_bounds__(kEvalThreads)
p_eval_tile_kernel(uint32_t lv, const uint32_t *__restrict__ in, size_t in_stride, const uint32_t *__restrict__ factors,
                   uint32_t *__restrict__ out, size_t out_stride)
{
    __shared__ QM31 s_wave[kEvalThreads / 64];
    const uint32_t tid = threadIdx.x, n_tile = 1u << lv, e0 = tid * kEvalPerLane;
    QM31 r;  // (factor addresses do not depend on the lane: uniform loads)
    if (QIN) {
        const QM31 f0 = ldq(factors);
        const uint32_t *src = in + (size_t)blockIdx.y * in_stride + (((size_t)blockIdx.x << lv) + e0) * 4;
        QM31 v[8];
#pragma unroll
        for (uint32_t j = 0; j < 8; j++) {
            const bool live = e0 + 2 * j + 1 < n_tile;  // n_tile is even: a pair is inside or outside as a whole
            v[j] = live ? fold_q(ldq4(src + 8 * j), ldq4(src + 8 * j + 4), f0) : qm31_zero();
        }
        r = eval_fold8(v, factors, lv);
    } else {
        const uint32_t *src = in + (size_t)blockIdx.y * in_stride + ((size_t)blockIdx.x << lv) + e0;
        uint32_t c[kEvalPerLane];
        if (e0 + kEvalPerLane <= n_tile && ((uintptr_t)src & 15) == 0) {
#pragma unroll
            for (uint32_t k = 0; k < 4; k++) {
                const uint4 w = reinterpret_cast<const uint4 *>(src)[k];
                c[4 * k] = w.x; c[4 * k + 1] = w.y; c[4 * k + 2] = w.z; c[4 * k + 3] = w.w;
            }
        } else {
#pragma unroll
            for (uint32_t k = 0; k < kEvalPerLane; k++) c[k] = e0 + k < n_tile ? src[k] : 0u;
        }
        r = eval_fold16(c, factors, lv);
    }
    r = eval_fold_wave(r, factors, lv);
    if ((tid & 63) == 0) s_wave[tid >> 6] = r;
    __syncthreads();
    if (tid) return;
    stq(out + (size_t)blockIdx.y * out_stride + 4 * (size_t)blockIdx.x, eval_fold_waves(r, s_wave, factors, lv));
}

// ------------------------------------------------------------------------ 5. deep_alpha and the DEEP coefficients
// One workgroup.  The channel is a dependent chain with nothing to share out, so wavefront 0 alone runs it (its lanes
// in lockstep on the same words): the mix of the 4 (N + 16) sample words is a runtime-length stream hash around one
// inlined compression, as the verifier's transcript kernel does for channel_mix_oods_evals.  deep_alpha reaches the
// other wavefronts through LDS; no other wavefront touches `state`, which lane 0 rewrites.
// Column k of a batch needs alpha^(k+1).  Lane i gets alpha^(i+1) from an inclusive prefix PRODUCT of 256 copies of
// alpha: six doubling steps inside the wavefront (__shfl_up), then the totals of the wavefronts below it from LDS --
// 6 + 3 dependent QM31 products instead of 256.  A batch wider than the workgroup (wide256: 272 columns) goes in chunks
// of 256 columns with the running power alpha^(256 chunk) carried along; the second batch restarts at alpha^1, and
// lane 15's power is alpha^16.  The sums A = sum a_k and C = sum c_k are workgroup reductions (__shfl_down, then LDS).
constexpr uint32_t kDeepThreads = 256;

template <int HF>
__global__ void __launch_bounds__(kDeepThreads)
p_deep_coeffs_kernel(uint32_t N, uint32_t *__restrict__ state, const uint32_t *__restrict__ samples,
                     const uint32_t *__restrict__ points, uint32_t *__restrict__ bcoef, uint32_t *__restrict__ sums,
                     uint32_t *__restrict__ err)
{
    constexpr uint32_t kWaves = kDeepThreads / 64;
    __shared__ QM31 s_alpha, s_total[kWaves], s_step, s_sum[2][2][kWaves];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // ---- channel_mix_oods_evals (deep/oods.simf:23-39), draw deep_alpha: wavefront 0
    if (wave == 0) {
        Channel<HF> ch;
        channel_load(ch, state);
        mix_stream<HF>(ch, samples, 4 * (N + kCp), CompressInline<HF>());
        QM31 drawn;
        const bool ok = ch.draw_qm31(drawn);
        if (tid == 0) {  // (every lane of this wavefront has read `state`: they run in lockstep, the loads come first)
            if (!ok) atomicOr(err, SS_P_ERR_TRANSCRIPT);
            channel_store(ch, state);
            s_alpha = drawn;
        }
    }
    __syncthreads();
    // ---- pw = alpha^(tid + 1)
    QM31 pw = alpha_powers(s_alpha, lane);
    if (lane == 63) s_total[wave] = pw;
    __syncthreads();
    for (uint32_t w = 0; w < wave; w++) pw = qm31_mul_c(pw, s_total[w]);
    if (tid == kDeepThreads - 1) s_step = pw;  // alpha^256: what a chunk multiplies the running power by
    __syncthreads();
    const QM31 step = s_step;
    // the sums of a batch over the workgroup -> sums_out[0..4) = A, [4..8) = C
    auto reduce = [&](uint32_t batch, QM31 A, QM31 C, uint32_t *sums_out) {
        wave_sum2(A, C);
        if (lane == 0) { s_sum[batch][0][wave] = A; s_sum[batch][1][wave] = C; }
        __syncthreads();
        if (tid < 2) {
            QM31 t = s_sum[batch][tid][0];
            for (uint32_t w = 1; w < kWaves; w++) t = qm31_add_c(t, s_sum[batch][tid][w]);
            stq(sums_out + 4 * tid, t);
        }
    };
    // ---- batch 1: the N trace columns at P
    const QM31 py = ldq(points + 4), p2y = ldq(points + 12);
    QM31 A = qm31_zero(), C = qm31_zero(), carry = qm31_one();
    for (uint32_t base = 0; base < N; base += kDeepThreads) {
        const uint32_t k = base + tid;
        if (k < N) {
            QM31 a, b, c;
            deep_interpolant(py, ldq(samples + 4 * (size_t)k), base ? qm31_mul_c(pw, carry) : pw, a, b, c);
            stq(bcoef + 4 * (size_t)k, b);
            A = qm31_add_c(A, a);
            C = qm31_add_c(C, c);
        }
        carry = qm31_mul_c(carry, step);
    }
    reduce(0, A, C, sums);
    // ---- batch 2: the 16 composition columns at 2P, powers from alpha^1 again
    A = qm31_zero();
    C = qm31_zero();
    if (tid < kCp) {
        QM31 b;
        deep_interpolant(p2y, ldq(samples + 4 * (size_t)(N + tid)), pw, A, b, C);
        stq(bcoef + 4 * (size_t)(N + tid), b);
    }
    reduce(1, A, C, sums + 8);
    if (tid == kCp - 1) stq(sums + 16, pw);  // alpha^16
}

}  // namespace
}  // namespace ss

// =============================================================================== C ABI
extern "C" int ss_p_channel_begin_dev(ss_ctx *ctx, uint32_t hash, const uint32_t const_root[8], const uint32_t *trace_root_dev,
                                      uint32_t *state_dev, uint32_t *cp_alpha_out_dev, uint32_t *err_dev, void *stream)
{
    SS_DEVICE_GUARD(ctx);
    if (!const_root || !trace_root_dev || !state_dev || !cp_alpha_out_dev || !err_dev || hash > 1)
        return ss_internal_set_err(SS_ERR_ARG, "ss_p_channel_begin_dev: bad argument");
    Dig root;
    for (int i = 0; i < 8; i++) root.v[i] = const_root[i];
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, root, trace_root_dev, state_dev, cp_alpha_out_dev,
                           err_dev);
    };
    if (hash) launch(p_channel_begin_kernel<1>);
    else launch(p_channel_begin_kernel<0>);
    HIP_TRY(hipGetLastError());
    return SS_OK;
}

extern "C" int ss_p_oods_point_dev(ss_ctx *ctx, uint32_t hash, uint32_t trace_log, uint32_t *state_dev,
                                   const uint32_t *cp_root_dev, uint32_t *points_out_dev, uint32_t *factors_p_out_dev,
                                   uint32_t *factors_2p_out_dev, uint32_t *err_dev, void *stream)
{
    SS_DEVICE_GUARD(ctx);
    if (!state_dev || !cp_root_dev || !points_out_dev || !factors_p_out_dev || (!factors_2p_out_dev && trace_log > 1) ||
        !err_dev || hash > 1 || trace_log < 1 || trace_log > 28)
        return ss_internal_set_err(SS_ERR_ARG, "ss_p_oods_point_dev: bad argument");
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, trace_log, state_dev, cp_root_dev, points_out_dev,
                           factors_p_out_dev, factors_2p_out_dev, err_dev);
    };
    if (hash) launch(p_oods_point_kernel<1>);
    else launch(p_oods_point_kernel<0>);
    HIP_TRY(hipGetLastError());
    return SS_OK;
}

// every launch but the last leaves ncols * tiles QM31 partials; the launches' regions follow each other
extern "C" size_t ss_p_eval_scratch_words(uint32_t m, uint32_t ncols)
{
    size_t words = 0;
    for (uint32_t rem = m; rem > kEvalT && rem <= 28; rem -= kEvalT) words += ((size_t)ncols << (rem - kEvalT)) * 4;
    return words;
}

extern "C" int ss_p_eval_at_point_dev(ss_ctx *ctx, uint32_t m, uint32_t ncols, const uint32_t *coeffs, size_t col_stride,
                                      const uint32_t *factors_dev, uint32_t *scratch_dev, uint32_t *out, void *stream)
{
    SS_DEVICE_GUARD(ctx);
    if (!coeffs || !factors_dev || !out || m < 1 || m > 28 || !ncols || ncols > 65535 || col_stride < ((size_t)1 << m) ||
        (m > kEvalT && (!scratch_dev || ((uintptr_t)scratch_dev & 15))))
        return ss_internal_set_err(SS_ERR_ARG, "ss_p_eval_at_point_dev: bad argument");
    const uint32_t *src = coeffs, *f = factors_dev;
    size_t sstride = col_stride;
    uint32_t *sc = scratch_dev;
    bool qin = false;
    for (uint32_t rem = m;;) {
        const uint32_t lv = rem < kEvalT ? rem : kEvalT, tiles = 1u << (rem - lv);  // (tiles <= 2^16)
        const bool last = tiles == 1;
        uint32_t *dst = last ? out : sc;
        const size_t dstride = last ? 4 : (size_t)tiles * 4;
        const dim3 grid(tiles, ncols);
        if (qin)
            hipLaunchKernelGGL(p_eval_tile_kernel<true>, grid, dim3(kEvalThreads), 0, (hipStream_t)stream, lv, src, sstride, f, dst, dstride);
        else
            hipLaunchKernelGGL(p_eval_tile_kernel<false>, grid, dim3(kEvalThreads), 0, (hipStream_t)stream, lv, src, sstride, f, dst, dstride);
        if (last) break;
        src = sc;
        sstride = dstride;
        sc += (size_t)ncols * dstride;
        f += 4 * lv;
        rem -= lv;
        qin = true;
    }
    HIP_TRY(hipGetLastError());
    return SS_OK;
}

extern "C" int ss_p_deep_coeffs_dev(ss_ctx *ctx, uint32_t hash, uint32_t n_cols, uint32_t *state_dev, const uint32_t *samples_dev,
                                    const uint32_t *points_dev, uint32_t *bcoef_out_dev, uint32_t *sums_alpha16_out_dev,
                                    uint32_t *err_dev, void *stream)
{
    SS_DEVICE_GUARD(ctx);
    if (!state_dev || !samples_dev || !points_dev || !bcoef_out_dev || !sums_alpha16_out_dev || !err_dev || hash > 1 ||
        !n_cols || n_cols > 65535)
        return ss_internal_set_err(SS_ERR_ARG, "ss_p_deep_coeffs_dev: bad argument");
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(1), dim3(kDeepThreads), 0, (hipStream_t)stream, n_cols, state_dev, samples_dev, points_dev,
                           bcoef_out_dev, sums_alpha16_out_dev, err_dev);
    };
    if (hash) launch(p_deep_coeffs_kernel<1>);
    else launch(p_deep_coeffs_kernel<0>);
    HIP_TRY(hipGetLastError());
    return SS_OK;
}
