// The end of the transcript with the proof of work ground by the whole GPU, in one launch (include/ss_prover_pow.h,
// DESIGN.md 7).  Everything p_finish_kernel (ss_prover.hip) does, and the same words; what differs is who searches.
//
//   work split  [0, span) is cut into chunks of kChunk = 256 * kRounds consecutive nonces.  A grid of persistent
//               workgroups claims chunk indices 0, 1, 2, ... from ONE 64-bit counter in device memory: lane 0 does the
//               atomicAdd and the index reaches the other lanes through LDS.
//   a chunk     rounds ascend, lane `tid` tries base + round * 256 + tid.  A round ends in ONE __syncthreads_or of
//               (this lane hit) | (lane 0 saw best < the round's base); when it is set the lanes that hit fold their
//               nonce into the 64-bit `best` in device memory and the workgroup leaves the chunk: later rounds hold
//               larger nonces.  Lane 0 loads `best` before the hash and looks at it after, so the latency is hidden, and
//               since the decision goes through the barrier's OR every wavefront takes the same branch.
//   leaving     a workgroup stops claiming when its chunk starts at or above span, or above the `best` it read with
//               the claim.  NO workgroup ever waits for another: no spin loop, no grid barrier, no cooperative launch.
//   the tail    every leaving workgroup fences and counts itself out; the one that counts gridDim.x - 1 others is the
//               last, reads `best` and finishes as p_finish_kernel does (mix the nonce, draw the queries, write the
//               channel, or on no hit leave the channel and write zero queries), then puts the three work words back
//               to zero for the next launch: nobody else is left to read them.
//
// Why `best` ends as the SMALLEST nonce below the target.  (1) Claims are the consecutive integers from 0.  (2) A
// workgroup stops only on a chunk that starts above the `best` it saw (or past span).  (3) `best` only decreases, so
// the `best` any workgroup saw is never below the final one.  Hence every chunk that starts at or below the final `best`
// was claimed by a workgroup that went INTO it; inside, that workgroup left a round unsearched only after a hit in that
// round or an earlier one of the same chunk, or after seeing best < that round's base -- and by (3) every round it
// skipped then lies wholly above the final `best` or above a hit that was folded into it.  So every nonce below the
// final `best` was hashed and missed, and `best` itself was hashed and hit.
//
// The word in memory holds ~best: zero then means "no hit" (a nonce is < span <= 2^64 - 1, so ~nonce >= 1), the
// caller's zeroing is the initial value, and atomicMax on the complement is atomicMin on the nonce.
//
// The last-layer scan (all n_last values equal) and the mix of last[0] are done by EVERY workgroup, redundantly, as
// every lane of p_finish_kernel does: the layer is 2^(blowup + 1) values, and every workgroup needs the mixed digest.
//
// Hashing.  The block is digest || be8(nonce) || padding.  SHA-256: the state after rounds 0..7 and the parts of the
// schedule words 16..22 that depend on the digest alone are computed once per workgroup, round 8 (its message word is
// the nonce's high half) and the rest of word 23 once per chunk -- a chunk never straddles a multiple of 2^32 -- and
// both live in scalar registers; a nonce costs rounds 9..63 and, of the digest, only words 6 and 7.  The additions are
// those of sha256_compress regrouped, exact modulo 2^32: bit for bit Hasher<0>::block<true, 8, 2>.  Blake2s has no
// midstate (the nonce enters round 0 already); it calls Hasher<1>::block itself with the digest in scalar registers.
#include <hip/hip_runtime.h>

#include "../../include/ss_prover.h"
#include "ss_ctx.h"
#include "ss_prover_dev.h"

using namespace ss;

extern "C" int ss_internal_set_err(int code, const char *msg);

namespace ss {
namespace {

constexpr uint32_t kPowThreads = 256;
// Measured on one MI355X with nothing hitting: one claim per 2^10 or 2^11 nonces holds the grid at 14 and
// 21 G compressions/s -- the one counter is the bottleneck -- 2^12 reaches 33 to 36 G/s, and 2^13 / 2^14 add 2 % at 2^28
// nonces but make every search of up to 2^20 nonces 30 to 100 % longer, since a chunk's rounds run one after the other.
constexpr uint32_t kRounds = 16;
constexpr uint64_t kChunk = (uint64_t)kPowThreads * kRounds;
static_assert((kChunk & (kChunk - 1)) == 0 && kChunk <= ((uint64_t)1 << 32), "a chunk keeps the nonce's high word fixed");
// Workgroups per compute unit: four wavefronts per SIMD, which the SHA-256 variant's 108 VGPRs just allow.  Two are
// within the spread up to 2^26 nonces and 9 % slower at 2^28 (32.96 against 36.05 G/s); one loses 20 %.
constexpr uint32_t kGridPerCu = 4;

template <int HF>
struct PowHash;

template <>
struct PowHash<0> {
    uint32_t mid[8];  // a..h after rounds 0..7
    uint32_t p[8];    // the digest-only part of schedule word 16 + i
    uint32_t st[8];   // a..h after round 8          | per chunk
    uint32_t p23;     // p[7] + s0(hi) + s1(w21)     |

    __device__ __forceinline__ void init(const uint32_t (&dig)[8])
    {
        uint32_t a, b, c, d, e, f, g, h;
        {
            uint32_t iv[8];
            sha_iv(iv);
            a = iv[0]; b = iv[1]; c = iv[2]; d = iv[3]; e = iv[4]; f = iv[5]; g = iv[6]; h = iv[7];
        }
        SS_SHA_ROUND(a, b, c, d, e, f, g, h, kK.k[0] + dig[0]);
        SS_SHA_ROUND(h, a, b, c, d, e, f, g, kK.k[1] + dig[1]);
        SS_SHA_ROUND(g, h, a, b, c, d, e, f, kK.k[2] + dig[2]);
        SS_SHA_ROUND(f, g, h, a, b, c, d, e, kK.k[3] + dig[3]);
        SS_SHA_ROUND(e, f, g, h, a, b, c, d, kK.k[4] + dig[4]);
        SS_SHA_ROUND(d, e, f, g, h, a, b, c, kK.k[5] + dig[5]);
        SS_SHA_ROUND(c, d, e, f, g, h, a, b, kK.k[6] + dig[6]);
        SS_SHA_ROUND(b, c, d, e, f, g, h, a, kK.k[7] + dig[7]);
        const uint32_t m[8] = {a, b, c, d, e, f, g, h};
#pragma unroll
        for (int i = 0; i < 8; i++) mid[i] = uni(m[i]);
        // w[r] = w[r-16] + s0(w[r-15]) + w[r-7] + s1(w[r-2]) with w8 = hi, w9 = lo, w10 = 0x80000000, w11..14 = 0, w15 = 320
        const uint32_t w17 = dig[1] + sha_s0(dig[2]) + 0x80000000u + sha_s1(320u);
        const uint32_t w19 = dig[3] + sha_s0(dig[4]) + sha_s1(w17);
        const uint32_t w21 = dig[5] + sha_s0(dig[6]) + sha_s1(w19);
        p[0] = uni(dig[0] + sha_s0(dig[1]));         // + lo
        p[1] = uni(w17);
        p[2] = uni(dig[2] + sha_s0(dig[3]));         // + s1(w16)
        p[3] = uni(w19);
        p[4] = uni(dig[4] + sha_s0(dig[5]));         // + s1(w18)
        p[5] = uni(w21);
        p[6] = uni(dig[6] + sha_s0(dig[7]) + 320u);  // + s1(w20)
        p[7] = uni(dig[7] + sha_s1(w21));            // + s0(hi) + w16
    }
    __device__ __forceinline__ void chunk(uint32_t hi)
    {
        uint32_t a = mid[0], b = mid[1], c = mid[2], d = mid[3], e = mid[4], f = mid[5], g = mid[6], h = mid[7];
        SS_SHA_ROUND(a, b, c, d, e, f, g, h, kK.k[8] + hi);
        const uint32_t m[8] = {a, b, c, d, e, f, g, h};
#pragma unroll
        for (int i = 0; i < 8; i++) st[i] = uni(m[i]);
        p23 = uni(p[7] + sha_s0(hi));
    }
    // pow_value of H(digest || hi || lo)
    __device__ __forceinline__ uint64_t value(uint32_t hi, uint32_t lo) const
    {
        uint32_t a = st[0], b = st[1], c = st[2], d = st[3], e = st[4], f = st[5], g = st[6], h = st[7];
        SS_SHA_ROUND(h, a, b, c, d, e, f, g, kK.k[9] + lo);
        SS_SHA_ROUND(g, h, a, b, c, d, e, f, kK.k[10] + 0x80000000u);
        SS_SHA_ROUND(f, g, h, a, b, c, d, e, kK.k[11]);
        SS_SHA_ROUND(e, f, g, h, a, b, c, d, kK.k[12]);
        SS_SHA_ROUND(d, e, f, g, h, a, b, c, kK.k[13]);
        SS_SHA_ROUND(c, d, e, f, g, h, a, b, kK.k[14]);
        SS_SHA_ROUND(b, c, d, e, f, g, h, a, kK.k[15] + 320u);
        // the rolling window as sha256_compress holds it before round 24: w[i] = word 16 + i (i < 8), words 8..15 above
        uint32_t w[16];
        w[0] = p[0] + lo;
        w[1] = p[1];
        w[2] = p[2] + sha_s1(w[0]);
        w[3] = p[3];
        w[4] = p[4] + sha_s1(w[2]);
        w[5] = p[5];
        w[6] = p[6] + sha_s1(w[4]);
        w[7] = p23 + w[0];
        w[8] = hi; w[9] = lo; w[10] = 0x80000000u; w[11] = 0; w[12] = 0; w[13] = 0; w[14] = 0; w[15] = 320u;
#pragma unroll
        for (int i = 16; i < 64; i += 8) {
            if (i >= 24) {
#pragma unroll
                for (int j = 0; j < 8; j++) {
                    const int r = i + j;
                    w[r & 15] += sha_s0(w[(r + 1) & 15]) + w[(r + 9) & 15] + sha_s1(w[(r + 14) & 15]);
                }
            }
            SS_SHA_ROUND(a, b, c, d, e, f, g, h, kK.k[i + 0] + w[(i + 0) & 15]);
            SS_SHA_ROUND(h, a, b, c, d, e, f, g, kK.k[i + 1] + w[(i + 1) & 15]);
            SS_SHA_ROUND(g, h, a, b, c, d, e, f, kK.k[i + 2] + w[(i + 2) & 15]);
            SS_SHA_ROUND(f, g, h, a, b, c, d, e, kK.k[i + 3] + w[(i + 3) & 15]);
            SS_SHA_ROUND(e, f, g, h, a, b, c, d, kK.k[i + 4] + w[(i + 4) & 15]);
            SS_SHA_ROUND(d, e, f, g, h, a, b, c, kK.k[i + 5] + w[(i + 5) & 15]);
            SS_SHA_ROUND(c, d, e, f, g, h, a, b, kK.k[i + 6] + w[(i + 6) & 15]);
            SS_SHA_ROUND(b, c, d, e, f, g, h, a, kK.k[i + 7] + w[(i + 7) & 15]);
        }
        const uint32_t d6 = 0x1f83d9abu + g, d7 = 0x5be0cd19u + h;  // IV words 6, 7 (sha_iv)
        return ((uint64_t)__builtin_bswap32(d7) << 32) | __builtin_bswap32(d6);
    }
};

template <>
struct PowHash<1> {
    uint32_t dig[8];
    __device__ __forceinline__ void init(const uint32_t (&d)[8])
    {
#pragma unroll
        for (int i = 0; i < 8; i++) dig[i] = uni(d[i]);
    }
    __device__ __forceinline__ void chunk(uint32_t) {}
    __device__ __forceinline__ uint64_t value(uint32_t hi, uint32_t lo) const
    {
        const uint32_t m[2] = {hi, lo};
        uint32_t d[8];
        Hasher<1>::block<true, 8, 2>(dig, m, d);
        return Hasher<1>::pow_value(d);
    }
};

__device__ __forceinline__ unsigned long long load_word(const unsigned long long *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Channel<HF>::mix_values with the compression inlined: the out-of-line calls of ss_channel.h pass their blocks through
// scratch memory, and this kernel has none.
template <int HF, int NV>
__device__ __forceinline__ void mix_values(Channel<HF> &ch, const uint32_t (&vals)[NV])
{
    Hasher<HF>::template block<true, 8, NV>(ch.dig.v, vals, ch.dig.v);
    ch.ctr = 0;
}

template <int HF>
__global__ void __launch_bounds__(kPowThreads)
p_finish_grid_kernel(uint32_t *__restrict__ state, const uint32_t *__restrict__ last, size_t n_last, uint64_t target,
                     uint64_t span, uint32_t lde_log, uint32_t n_queries, uint32_t *__restrict__ queries,
                     uint32_t *__restrict__ nonce_out, uint32_t *__restrict__ err, unsigned long long *work)
{
    __shared__ unsigned long long s_claim, s_best;
    __shared__ uint32_t s_last;
    constexpr unsigned long long kNone = ~0ull;
    unsigned long long *claim_w = work, *best_w = work + 1, *gone_w = work + 2;  // best_w holds ~best
    const uint32_t tid = threadIdx.x;
    const int differs = last_layer_differs(last, n_last, tid, kPowThreads);
    const QM31 first = ldq4(last);
    Channel<HF> ch;
    channel_load(ch, state);
    const int bad_layer = __syncthreads_or(differs);
    const uint32_t lv[4] = {first.a, first.b, first.c, first.d};
    mix_values<HF>(ch, lv);
    PowHash<HF> ph;
    ph.init(ch.dig.v);

    const uint64_t n_chunks = (span - 1) / kChunk + 1;  // (span >= 1: the entry point refuses 0)
    for (;;) {
        if (tid == 0) {
            s_claim = atomicAdd(claim_w, 1ull);
            s_best = ~load_word(best_w);
        }
        __syncthreads();
        const uint64_t chunk = s_claim, seen = s_best;
        __syncthreads();  // (lane 0 writes the next claim only after everybody has read this one)
        if (chunk >= n_chunks) break;
        const uint64_t base = chunk * kChunk;  // < span: no overflow
        if (base > seen) break;
        const uint32_t hi = uni((uint32_t)(base >> 32));
        ph.chunk(hi);
        for (uint32_t round = 0; round < kRounds; round++) {
            const uint64_t rbase = base + (uint64_t)round * kPowThreads;
            if (rbase >= span) break;  // (uniform)
            const uint64_t best = tid == 0 ? ~load_word(best_w) : kNone;  // one load per workgroup and round, not one per wavefront
            const uint64_t cand = rbase + tid;
            const bool hit = cand < span && ph.value(hi, (uint32_t)cand) < target;
            if (__syncthreads_or((int)hit | (int)(best < rbase))) {
                if (hit) atomicMax(best_w, ~(unsigned long long)cand);
                break;
            }
        }
    }

    // out: this workgroup's atomics are performed before it is counted as gone
    __threadfence();
    __syncthreads();
    if (tid == 0) {
        const bool is_last = atomicAdd(gone_w, 1ull) == (unsigned long long)gridDim.x - 1;
        if (is_last) {
            __threadfence();
            s_best = ~load_word(best_w);
            *claim_w = 0;  // every other workgroup has made its last access: ready for the next launch
            *best_w = 0;
            *gone_w = 0;
        }
        s_last = is_last;
    }
    __syncthreads();
    if (!s_last) return;

    const unsigned long long nonce = s_best;
    if (nonce != kNone) {
        const uint32_t nv[2] = {(uint32_t)(nonce >> 32), (uint32_t)nonce};
        mix_values<HF>(ch, nv);
        draw_queries<HF, true>(ch, lde_log, n_queries, tid == 0, queries);  // (inlined, as mix_values above)
        if (tid == 0) {
            channel_store(ch, state);
            nonce_out[0] = nv[0];
            nonce_out[1] = nv[1];
        }
    } else {
        for (uint32_t i = tid; i < n_queries; i += kPowThreads) queries[i] = 0;  // defined positions for the decommitment behind
    }
    const uint32_t bits = (bad_layer ? SS_P_ERR_LAST_LAYER : 0u) | (nonce == kNone ? SS_P_ERR_POW_SPAN : 0u);
    if (tid == 0 && bits) atomicOr(err, bits);
}

}  // namespace
}  // namespace ss

extern "C" int ss_p_finish_grid_dev(ss_ctx *ctx, uint32_t hash, uint32_t lde_log, uint32_t n_queries, uint64_t pow_target,
                                    uint64_t span, uint32_t *state_dev, const uint32_t *last_dev, size_t n_last,
                                    uint32_t *queries_out_dev, uint32_t *nonce_out_dev, uint32_t *err_dev,
                                    uint64_t *work_dev, void *stream)
{
    SS_DEVICE_GUARD(ctx);
    // (the two sizes this call depends on, by the layout's own rule, as ss_p_finish_dev checks them)
    if (!stwo_cfg_ok(1, 1, lde_log, n_queries, 0, 0) || hash > 1 || !span || !state_dev || !last_dev || !n_last ||
        !queries_out_dev || !nonce_out_dev || !err_dev || !work_dev)
        return ss_internal_set_err(SS_ERR_ARG, "ss_p_finish_grid_dev: bad argument");
    if (((uintptr_t)last_dev & 15u) != 0 || ((uintptr_t)work_dev & 7u) != 0 ||
        (((uintptr_t)state_dev | (uintptr_t)queries_out_dev | (uintptr_t)nonce_out_dev | (uintptr_t)err_dev) & 3u) != 0)
        return ss_internal_set_err(SS_ERR_ARG, "ss_p_finish_grid_dev: last_dev needs 16-byte, work_dev 8-byte alignment");
    // never more workgroups than chunks; the all-ones span must be refused by no sum that wraps
    const uint64_t n_chunks = (span - 1) / kChunk + 1;
    const uint64_t want = (uint64_t)kGridPerCu * (uint64_t)(ctx->cus > 0 ? ctx->cus : 1);
    const uint32_t grid = (uint32_t)(n_chunks < want ? n_chunks : want);
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(kPowThreads), 0, (hipStream_t)stream, state_dev, last_dev, n_last,
                           pow_target, span, lde_log, n_queries, queries_out_dev, nonce_out_dev, err_dev,
                           (unsigned long long *)work_dev);
    };
    if (hash) launch(p_finish_grid_kernel<1>);
    else launch(p_finish_grid_kernel<0>);
    HIP_TRY(hipGetLastError());
    return SS_OK;
}
