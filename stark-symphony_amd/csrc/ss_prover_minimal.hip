// The decommitment as a minimal record, planned and gathered on the device, and the packing of a batch of them
// (include/ss_prover_minimal.h; the form is defined in include/ss_verify_forms.h and csrc/ss_minimal.h).
//
// p_decommit_record_kernel (ss_prover.hip) gathers a fixed shape: one wavefront per authentication chain.  Here the
// shape is data.  With s = the Q masked positions in ascending order, the nodes of absolute level a are the runs of
// equal s[i] >> a (sorting survives the shift), so one lane per sorted query and two ballots per level give
//   nodes[a]  bit i: sorted lane i is the first of its run -- the node s[i] >> a of Nodes(a)
//   lone[a]   bit i: ... and its sibling (s[i] >> a) ^ 1 is not a node; that sibling could only be the run before
//             (odd node) or the run after (even node), so it is one compare with a neighbouring run
// and everything the layout needs after that is a popcount: |Lone(a)| = popc(lone[a]), the place of lane i's node in
// its level's list = popc(lone[a] & lanes below i), the list lengths and bases two wavefront scans over <= 64 lanes
// (31 levels; 2 K + 4 <= 64 lists).  Every workgroup recomputes that plan -- wavefront 0: a rank sort of 64 broadcasts,
// then two shuffles and two ballots per level -- and shares it through LDS: cheaper than a second launch, and nothing
// goes through global memory.
// Lanes talk through shuffles and ballots only; LDS is written before a workgroup barrier and read after it.
//
// The gather is one wavefront per LIST PIECE, lane = sorted query: (tree, level) moves the siblings of Lone(level),
// (layer) the fold partners of Lone(layer), (sorted query, commitment) the queried values of a distinct position with
// the lanes striding over the columns.  One more workgroup writes the head, the list lengths and the size.
#include <hip/hip_runtime.h>

#include "../../include/ss_prover.h"
#include "ss_ctx.h"
#include "ss_minimal.h"
#include "ss_prover_dev.h"

using namespace ss;

extern "C" int ss_internal_set_err(int code, const char *msg);

namespace ss {
namespace {

constexpr uint32_t kMinThreads = 256, kMinWaves = kMinThreads / 64;
constexpr uint32_t kMinLists = 2 * kMaxList + 2;  // fri_wit[K + 1] then hash_wit[K + 3], K <= 30: at most 64, a lane each

struct MinDecommitArgs {
    uint32_t N, L, Q, K;
    uint32_t const_root[8];  // stored words
};

// The plan of one proof, in LDS.
struct MinPlanDev {
    uint32_t s[kMaxQueries];     // the masked positions, ascending; entries >= Q hold 0xFFFFFFFF
    uint64_t nodes[kMaxList];    // per absolute level, see above
    uint64_t lone[kMaxList];
    uint32_t cum[kMaxList + 1];  // cum[a] = |Lone(0)| + .. + |Lone(a - 1)|, a = 0 .. L
    uint32_t len[kMinLists];     // n_fw[K + 1], n_hw[K + 3]: the record's own order
    uint32_t base[kMinLists];    // first word of each of those lists
    uint32_t n_vals, words;      // |Nodes(0)|; the record's size
};

__device__ __forceinline__ uint32_t wave_scan(uint32_t v, uint32_t lane)  // inclusive
{
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t t = __shfl_up(v, d, 64);
        if (lane >= d) v += t;
    }
    return v;
}

// Both halves are called by every wavefront of the workgroup (wavefront 0 works) with a barrier between and after.
__device__ __forceinline__ void min_plan_sort(MinPlanDev &p, const uint32_t *__restrict__ queries, uint32_t L, uint32_t Q,
                                              uint32_t lane)
{
    // rank sort: 64 broadcasts, ties broken by lane, so the ranks are a permutation; the padding sorts last (a
    // position has at most 31 bits)
    const uint32_t q = lane < Q ? queries[lane] & (uint32_t)(((uint64_t)1 << L) - 1) : 0xFFFFFFFFu;
    uint32_t rank = 0;
#pragma unroll
    for (uint32_t j = 0; j < 64; j++) {
        const uint32_t qj = __shfl(q, j, 64);
        rank += (qj < q) | ((qj == q) & (j < lane));
    }
    p.s[rank] = q;
}

__device__ __forceinline__ void min_plan_lists(MinPlanDev &p, const MinMap &m, uint32_t lane)
{
    const uint32_t L = m.L, Q = m.Q, K = m.K;
    const uint32_t sv = p.s[lane];
    const uint64_t bit = (uint64_t)1 << lane, below = bit - 1;
    uint32_t cnt = 0;  // lane a: |Lone(a)|
    uint64_t nodes0 = 0;
    for (uint32_t a = 0; a < L; a++) {
        const uint32_t x = sv >> a, px = __shfl_up(x, 1, 64);
        const bool head = lane < Q && (lane == 0 || px != x);
        const uint64_t nodes = __ballot(head);
        // a head's previous run ends in the lane below it; its next run starts at the first head above it
        const uint64_t above = nodes & ~(below | bit);
        const uint32_t nx = __shfl(x, above ? (uint32_t)__ffsll((unsigned long long)above) - 1 : lane, 64);
        const bool paired = (x & 1) ? (lane > 0 && px == (x ^ 1)) : (above != 0 && nx == (x ^ 1));
        const uint64_t lone = __ballot(head && !paired);
        if (lane == 0) {
            p.nodes[a] = nodes;
            p.lone[a] = lone;
        }
        if (lane == a) cnt = (uint32_t)__popcll(lone);
        if (a == 0) nodes0 = nodes;
    }
    const uint32_t inc = wave_scan(cnt, lane), cum = inc - cnt, total = __shfl(inc, 63, 64);
    if (lane <= L) p.cum[lane] = cum;  // (lanes >= L count nothing: cum[L] = total)
    // list `lane`: fri_wit[lane] = Lone(lane); hash_wit[t], t = lane - (K + 1): Lone(first) .. Lone(L - 1)
    const uint32_t t = lane - (K + 1);
    const uint32_t cum_first = __shfl(cum, lane > K && lane < 2 * K + 4 ? min_tree_shift(t) : 0, 64);
    const uint32_t len = lane <= K ? cnt : lane < 2 * K + 4 ? total - cum_first : 0;
    const uint32_t size = lane <= K ? 4 * len : 8 * len;
    const uint32_t n_vals = (uint32_t)__popcll(nodes0), lists = m.data + n_vals * (m.N + kCp);
    const uint32_t end = wave_scan(size, lane);
    if (lane < 2 * K + 4) {
        p.len[lane] = len;
        p.base[lane] = lists + end - size;
    }
    if (lane == 63) {
        p.n_vals = n_vals;
        p.words = lists + end;
    }
}

__global__ void __launch_bounds__(kMinThreads)
p_decommit_minimal_kernel(MinDecommitArgs a, const ss_p_tree *__restrict__ trees_dev, const uint32_t *__restrict__ samples,
                          const uint32_t *__restrict__ fri_roots, const uint32_t *__restrict__ last,
                          const uint32_t *__restrict__ nonce, const uint32_t *__restrict__ queries, uint32_t *__restrict__ out,
                          uint32_t *__restrict__ words_out)
{
    __shared__ ss_p_tree trees[kMaxList + 3];
    __shared__ MinPlanDev p;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t N = a.N, L = a.L, Q = a.Q, K = a.K, kinds = K + 3;
    const MinMap m = min_map(N, L, Q, K);
    for (uint32_t i = tid; i < kinds; i += kMinThreads) trees[i] = trees_dev[i];
    if (wave == 0) min_plan_sort(p, queries, L, Q, lane);
    __syncthreads();
    if (wave == 0) min_plan_lists(p, m, lane);
    __syncthreads();

    if (blockIdx.x == gridDim.x - 1) {
        // ---- head, list lengths, size
        const uint32_t *troot = trees[0].levels + (((uint64_t)2 << L) - 2) * 8;
        const uint32_t *croot = trees[1].levels + (((uint64_t)1 << L) - 2) * 8;  // (tree over the 2^(L-1) pairs)
        const uint32_t oods = 4 * (N + kCp);
        for (uint32_t w = tid; w < m.data; w += kMinThreads) {
            uint32_t v = 0, r = w;
            if (r < 8) {
#pragma unroll
                for (uint32_t k = 0; k < 8; k++)  // (a kernel argument: selected, not indexed)
                    if (r == k) v = a.const_root[k];
            }
            else if ((r -= 8) < 8) v = troot[r];
            else if ((r -= 8) < 8) v = croot[r];
            else if ((r -= 8) < oods) v = samples[r];
            else if ((r -= oods) < 8 * (K + 1)) v = fri_roots[r];
            else if ((r -= 8 * (K + 1)) < 4) v = last[r];
            else if ((r -= 4) < 2) v = nonce[r];
            else if ((r -= 2) < 2) v = p.n_vals;
            else v = p.len[r - 2];
            out[w] = v;
        }
        if (tid == 0) *words_out = p.words;
        return;
    }

    // ---- one wavefront per list piece
    uint32_t item = blockIdx.x * kMinWaves + wave;
    const uint64_t below = ((uint64_t)1 << lane) - 1;
    if (item < kinds * L) {
        // siblings of Lone(lvl) in tree t, whose leaves sit at absolute level `leaf` (composition: the tree over the
        // pairs starts at 1, and the sibling of a leaf is the other leaf of its pair -- the same hash)
        const uint32_t t = item / L, lvl = item - t * L, first = min_tree_shift(t);
        const uint64_t lone = p.lone[lvl];
        if (lvl < first || !((lone >> lane) & 1)) return;
        const uint32_t x = p.s[lane] >> lvl;
        const ss_p_tree tr = trees[t];
        uint32_t *dst = out + p.base[K + 1 + t] + 8 * (size_t)(p.cum[lvl] - p.cum[first] + (uint32_t)__popcll(lone & below));
        const uint32_t *src;
        if (t == 1 && lvl == 0) {
            src = tr.leaf + (size_t)(x >> 1) * 8;
        } else {
            const uint32_t leaf = t < 2 ? t : t - 2, j = lvl - leaf;
            const uint64_t two_n = (uint64_t)2 << (L - leaf);
            src = tr.levels + (two_n - (two_n >> j) + (x ^ 1)) * 8;
        }
        move16(dst, src);
        move16(dst + 4, src + 4);
        return;
    }
    item -= kinds * L;
    if (item <= K) {
        // fold partners of Lone(l) in layer l
        const uint64_t lone = p.lone[item];
        if (!((lone >> lane) & 1)) return;
        const uint32_t x = p.s[lane] >> item;
        move16(out + p.base[item] + 4 * (size_t)__popcll(lone & below), trees[2 + item].values + (size_t)(x ^ 1) * 4);
        return;
    }
    item -= K + 1;
    if (item < 2 * Q) {
        // queried values of the distinct position that sorted query i heads, lanes over the columns
        const uint32_t i = item >> 1;
        const uint64_t nodes = p.nodes[0];
        if (!((nodes >> i) & 1)) return;
        const uint32_t x = p.s[i], v = (uint32_t)__popcll(nodes & (((uint64_t)1 << i) - 1));
        if (item & 1) {
            uint32_t *dst = out + m.data + (size_t)p.n_vals * N + (size_t)v * kCp;
            if (lane < kCp) dst[lane] = trees[1].values[((size_t)lane << (L - 1)) + (x >> 1)];
        } else {
            uint32_t *dst = out + m.data + (size_t)v * N;
            for (uint32_t c = lane; c < N; c += 64) dst[c] = trees[0].values[((size_t)c << L) + x];
        }
    }
}

// ------------------------------------------------------------------------------ packing a batch
constexpr uint32_t kPackThreads = 256;

// offs[p] = sum of min(words[i], cap) over i < p, p = 0 .. n: one workgroup, 256 sizes per round, carry between rounds
__global__ void __launch_bounds__(kPackThreads)
p_minimal_offs_kernel(size_t n, const uint32_t *__restrict__ words, uint32_t cap, uint64_t *__restrict__ offs)
{
    __shared__ unsigned long long wsum[kPackThreads / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned long long carry = 0;
    for (size_t base = 0; base < n; base += kPackThreads) {
        const size_t i = base + tid;
        uint32_t v = i < n ? words[i] : 0;
        v = v < cap ? v : cap;
        unsigned long long inc = v;
#pragma unroll
        for (uint32_t d = 1; d < 64; d <<= 1) {
            const unsigned long long t = __shfl_up(inc, d, 64);
            if (lane >= d) inc += t;
        }
        if (lane == 63) wsum[wave] = inc;
        __syncthreads();
        unsigned long long before = carry, all = 0;
#pragma unroll
        for (uint32_t w = 0; w < kPackThreads / 64; w++) {
            if (w < wave) before += wsum[w];
            all += wsum[w];
        }
        if (i < n) offs[i] = before + inc - v;
        carry += all;
        __syncthreads();  // (wsum is written again in the next round)
    }
    if (tid == 0) offs[n] = carry;
}

// grid = (chunk, record): a workgroup copies every gridDim.x-th run of 256 words of its records
__global__ void __launch_bounds__(kPackThreads)
p_minimal_pack_kernel(size_t n, const uint32_t *__restrict__ rows, size_t stride, const uint64_t *__restrict__ offs,
                      uint32_t *__restrict__ packed)
{
    for (size_t p = blockIdx.y; p < n; p += gridDim.y) {
        const uint64_t o = offs[p];
        const uint32_t size = (uint32_t)(offs[p + 1] - o);  // (<= stride: p_minimal_offs_kernel caps it)
        const uint32_t *src = rows + p * stride;
        uint32_t *dst = packed + o;
        for (uint32_t w = blockIdx.x * kPackThreads + threadIdx.x; w < size; w += gridDim.x * kPackThreads) dst[w] = src[w];
    }
}

}  // namespace
}  // namespace ss

// =============================================================================== C ABI
extern "C" int ss_p_decommit_minimal(ss_ctx *ctx, const ss_stwo_cfg *cfg, const ss_p_tree *trees_dev,
                                     const uint32_t *samples_dev, const uint32_t *fri_roots_dev, const uint32_t *last_dev,
                                     const uint32_t *nonce_dev, const uint32_t const_root[8], const uint32_t *queries_dev,
                                     uint32_t *minimal_out_dev, uint32_t *words_out_dev, void *stream)
{
    SS_DEVICE_GUARD(ctx);
    if (!cfg || !stwo_cfg_ok(cfg->n_cols, cfg->trace_log, cfg->lde_log, cfg->n_queries, cfg->n_layers, cfg->mode) ||
        !trees_dev || !samples_dev || !fri_roots_dev || !last_dev || !nonce_dev || !const_root || !queries_dev ||
        !minimal_out_dev || ((uintptr_t)minimal_out_dev & 3) || !words_out_dev || ((uintptr_t)words_out_dev & 3))
        return ss_internal_set_err(SS_ERR_ARG, "ss_p_decommit_minimal: bad argument");
    MinDecommitArgs a;
    a.N = cfg->n_cols; a.L = cfg->lde_log; a.Q = cfg->n_queries; a.K = cfg->n_layers;
    for (int i = 0; i < 8; i++) a.const_root[i] = const_root[i];
    const uint32_t items = (a.K + 3) * a.L + (a.K + 1) + 2 * a.Q;
    hipLaunchKernelGGL(p_decommit_minimal_kernel, dim3((items + kMinWaves - 1) / kMinWaves + 1), dim3(kMinThreads), 0,
                       (hipStream_t)stream, a, trees_dev, samples_dev, fri_roots_dev, last_dev, nonce_dev, queries_dev,
                       minimal_out_dev, words_out_dev);
    HIP_TRY(hipGetLastError());
    return SS_OK;
}

extern "C" int ss_p_minimal_pack_dev(ss_ctx *ctx, size_t n, const uint32_t *rows_dev, size_t row_stride_words,
                                     const uint32_t *words_dev, uint32_t *packed_out_dev, uint64_t *offs_out_dev, void *stream)
{
    SS_DEVICE_GUARD(ctx);
    if (!rows_dev || !words_dev || !packed_out_dev || !offs_out_dev || !row_stride_words || row_stride_words > 0xFFFFFFFFu ||
        ((uintptr_t)offs_out_dev & 7))
        return ss_internal_set_err(SS_ERR_ARG, "ss_p_minimal_pack_dev: bad argument");
    hipLaunchKernelGGL(p_minimal_offs_kernel, dim3(1), dim3(kPackThreads), 0, (hipStream_t)stream, n, words_dev,
                       (uint32_t)row_stride_words, offs_out_dev);
    HIP_TRY(hipGetLastError());
    if (!n) return SS_OK;
    // four words per thread and pass at the longest record; the y dimension loops past its limit
    const dim3 grid((unsigned)((row_stride_words + 4 * kPackThreads - 1) / (4 * kPackThreads)), (unsigned)(n < 65535 ? n : 65535));
    hipLaunchKernelGGL(p_minimal_pack_kernel, grid, dim3(kPackThreads), 0, (hipStream_t)stream, n, rows_dev, row_stride_words,
                       offs_out_dev, packed_out_dev);
    HIP_TRY(hipGetLastError());
    return SS_OK;
}
