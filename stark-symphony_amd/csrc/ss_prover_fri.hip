// The FRI commit of every layer that fits in one workgroup, in one launch (include/ss_prover_fri.h).
//
// The launch loop of prover.py runs, per layer, ss_p_hash_qm31 -> ss_p_merkle (a launch per wide level + the tail)
// -> ss_p_channel_fri_layer -> ss_p_fri_fold_dev, each waiting for the one before.  Below a few thousand values that
// chain is dispatch latency and nothing else.  Here ONE workgroup stays resident over all those layers:
//
//   values     never touch LDS as a layer.  A thread OWNS a storage pair (2i, 2i+1) -- two at 2^kTailLog, where
//              a thread's two folds are the next layer's pair already -- loads it once (layer 0) and keeps it in
//              registers: it hashes the two leaves and their parent from registers, and after alpha folds them into
//              out[i].  The next layer's pair k is (out[2k], out[2k+1]): 16 bytes per thread through a word-major LDS
//              tile while a layer is wider than a wavefront, two lane reads (ds_bpermute) once it is not.
//   tree       level 1 (and level 2 at 2^kTailLog) is hashed from registers.  A level with more than 64 nodes is
//              handed down through LDS, ping-ponged between two buffers so that ONE workgroup barrier per level
//              suffices; nodes lie word-major ([word][node]), so the writes are consecutive lanes -> consecutive banks
//              and the read of a node's two children is one 8-byte access per word, conflict-free as well.
//              From 64 nodes down the level lives in the registers of wavefront 0 and a parent's children are two lane
//              reads: no LDS, no barrier.
//   channel    every lane of wavefront 0 runs the same Channel<HF> state on the root broadcast from lane 0 (uniform, no
//              divergence; kept in scalar registers), from state_dev read once to state_dev written once.  Its mix is
//              the last turn of the tree's level loop and its draw one inlined block hash: Channel<HF>'s own methods
//              call out-of-line compressions, which cost scratch.  The other wavefronts get alpha through four LDS
//              words and one barrier; wavefront 0 needs neither.
//   wave stage once a layer has at most 64 pairs the other wavefronts return, and the rest of the chain (half of the
//              layers of a 2^11 start) runs in wavefront 0 with no barrier and no LDS at all.
//   prefetch   a layer's coord_inv words are loaded before its tree is hashed and used after alpha is drawn.
//
// Every hash, the draw and the fold are the code of p_hash_qm31_kernel, merkle_parent, p_channel_fri_layer_kernel and
// p_fri_fold_dev_kernel (ss_prover.hip): Hasher<HF>::block<.., 0, 4> / pair, Channel<HF>::mix / draw_qm31, and
// (v0 + v1) + alpha * ((v0 - v1) * coord_inv).  All of it is exact integer arithmetic on canonical words.
#include <hip/hip_runtime.h>

#include "../../include/ss_prover.h"
#include "ss_ctx.h"
#include "ss_prover_dev.h"

using namespace ss;

extern "C" int ss_internal_set_err(int code, const char *msg);

namespace ss {
namespace {

// 2^11 values = 1024 pairs = two per thread of a workgroup of 512.  What bounds it is the register file, not LDS
// (24 KB of the CU's 160 KB): the unrolled SHA-256 compression inside the level loop wants about 150 VGPRs (its round
// constants are hoisted out of the loop), which 16 wavefronts (128 VGPRs each) cannot have without scratch and 8 can.
// Nothing is lost with 8: the hashes are dependent VALU chains, which one wavefront per SIMD already issues back to back.
// Four pairs a thread (2^12) would hold 32 value words and four node hashes over the tree: scratch again.
constexpr uint32_t kTailLog = 11;
constexpr uint32_t kTailThreads = 512;
constexpr uint32_t kPlaneA = kTailThreads;      // nodes of the widest level that goes through LDS
constexpr uint32_t kPlaneB = kTailThreads / 2;  // ... and of the level after it; as a value tile: [4][kTailThreads]
static_assert((1u << kTailLog) == 4 * kTailThreads, "a thread owns at most two storage pairs");
static_assert(8 * kPlaneB == 4 * kTailThreads, "the value tile shares the second node buffer");

template <int HF>
__global__ void __launch_bounds__(kTailThreads)
p_fri_tail_kernel(uint32_t log_n, uint32_t n_layers, uint32_t *__restrict__ state, const uint32_t *__restrict__ layer,
                  const uint32_t *__restrict__ cinv, uint32_t *__restrict__ arena, uint32_t *__restrict__ roots_out,
                  uint32_t *__restrict__ alphas_out)
{
    __shared__ __attribute__((aligned(16))) uint32_t lds_a[8 * kPlaneA];  // [word][node]
    __shared__ __attribute__((aligned(16))) uint32_t lds_b[8 * kPlaneB];  // [word][node]; between two trees the value tile [word][pair]
    __shared__ uint32_t lds_alpha[4];
    const uint32_t t = threadIdx.x, lane = t & 63u, nt = blockDim.x;
    const uint32_t ln0 = (2u * lane) & 63u, ln1 = ln0 + 1u;  // the lanes of a node's children / a pair's values

    // The channel: the same in every lane of wavefront 0 (and unused in the others), so it is read through
    // readfirstlane and lives in scalar registers, native digest words + num_sent.
    Channel<HF> ch;
    channel_load(ch, state);
#pragma unroll
    for (int i = 0; i < 8; i++) ch.dig.v[i] = uni(ch.dig.v[i]);
    ch.ctr = uni(ch.ctr);

    uint32_t n = 1u << log_n;
    // The thread's pair.  With two pairs a thread (layer 0 of a 2^kTailLog start) they are read where they are used,
    // for the leaves and again for the fold: input words, still in L2, and eight registers fewer over the tree.
    QM31 v0 = qm31_zero(), v1 = v0;
    if ((n >> 1) <= nt && t < (n >> 1)) { v0 = ldq4(layer + 8 * t); v1 = ldq4(layer + 8 * t + 4); }

    uint32_t *tree = arena;
    for (uint32_t j = 0; j < n_layers; j++) {
        const uint32_t np = n >> 1;   // pairs = nodes of level 1 = values of the next layer
        const bool two = np > nt;     // (layer 0 of a 2^kTailLog start only)
        if (np <= 64 && t >= 64) return;  // the wave stage: no barrier is reached from here on (all are behind "> 64")
        uint32_t *fold = tree + 16 * (size_t)n;

        // ---- this layer's coord_inv, in flight while the tree is hashed
        uint32_t c0 = 0, c1 = 0;
        if (two) { c0 = cinv[2 * t]; c1 = cinv[2 * t + 1]; }
        else if (t < np) c0 = cinv[t];

        // ---- leaves and level 1 from registers
        uint32_t h[8] = {0, 0, 0, 0, 0, 0, 0, 0}, hr[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // native words
        const uint32_t mine = two ? 2u : (t < np ? 1u : 0u);
#pragma unroll 1
        for (uint32_t p = 0; p < mine; p++) {
            const uint32_t pair = two ? 2 * t + p : t;
            uint32_t l[8], r[8];
#pragma unroll 1
            for (uint32_t s = 0; s < 2; s++) {  // (one inlined leaf hash, not two)
                QM31 v = s ? v1 : v0;
                if (two) v = ldq4(layer + 4 * (size_t)(2 * pair + s));
                const uint32_t e[4] = {v.a, v.b, v.c, v.d};
                uint32_t d[8];
                Hasher<HF>::template block<true, 0, 4>(nullptr, e, d);
                st_node<HF>(tree, 2 * pair + s, d);
#pragma unroll
                for (int k = 0; k < 8; k++) { if (s) r[k] = d[k]; else l[k] = d[k]; }
            }
            uint32_t d[8];
            Hasher<HF>::template pair<true>(l, r, d);
            st_node<HF>(tree, n + pair, d);
#pragma unroll
            for (int k = 0; k < 8; k++) { if (p) hr[k] = d[k]; else h[k] = d[k]; }
        }

        // ---- the levels above, and the channel's mix as the last turn of the same loop (digest <- H(digest || root) is
        // one more pair hash: one inlined copy serves both).  Thread t < cur holds node t of the level of `cur` nodes at
        // row `row` in h -- or, with have_lr, thread t < cur / 2 holds the two children of ITS parent already (h, hr).
        uint32_t cur = np, row = n;
        bool have_lr = two, flip = false;
        for (;;) {
            const bool mix = cur == 1;  // thread 0 holds the root
            const uint32_t par = cur >> 1;
            uint32_t l[8], r[8];
            if (mix) {
#pragma unroll
                for (int k = 0; k < 8; k++) { l[k] = ch.dig.v[k]; r[k] = (uint32_t)__shfl((int)h[k], 0); }
                if (t == 0) st_node<HF>(roots_out, j, r);
            } else if (have_lr) {
#pragma unroll
                for (int k = 0; k < 8; k++) { l[k] = h[k]; r[k] = hr[k]; }
            } else if (cur > 64) {
                uint32_t *buf = flip ? lds_b : lds_a;
                const uint32_t plane = flip ? kPlaneB : kPlaneA;
                if (t < cur) {
#pragma unroll
                    for (int k = 0; k < 8; k++) buf[k * plane + t] = h[k];
                }
                __syncthreads();
#pragma unroll
                for (int k = 0; k < 8; k++) {
                    const uint2 c = t < par ? *reinterpret_cast<const uint2 *>(buf + k * plane + 2 * t) : make_uint2(0, 0);
                    l[k] = c.x; r[k] = c.y;
                }
                flip = !flip;
            } else {
#pragma unroll
                for (int k = 0; k < 8; k++) {
                    l[k] = (uint32_t)__shfl((int)h[k], (int)ln0);
                    r[k] = (uint32_t)__shfl((int)h[k], (int)ln1);
                }
            }
            have_lr = false;
            row += cur;
            if (mix ? t < 64 : t < par) {
                uint32_t d[8];
                Hasher<HF>::template pair<true>(l, r, d);
#pragma unroll
                for (int k = 0; k < 8; k++) h[k] = d[k];
                if (!mix) st_node<HF>(tree, row + t, h);
            }
            if (mix) break;
            cur = par;
        }

        // ---- the rest of fri_layer_commit (channel_mix_u256 resets num_sent; channel_draw_qm31 as Channel<HF> has it,
        // with the one-block hash inlined), then alpha to the other wavefronts
        QM31 alpha = qm31_zero();
        if (t < 64) {
#pragma unroll
            for (int k = 0; k < 8; k++) ch.dig.v[k] = uni(h[k]);
            ch.ctr = 0;
#pragma unroll 1
            for (int it = 0; it < 256; it++) {
                const uint32_t m[1] = {ch.ctr};
                uint32_t d[8];
                Hasher<HF>::template block<true, 8, 1>(ch.dig.v, m, d);
                ch.ctr = ch.ctr + 1;
                const uint32_t w0 = Hasher<HF>::native(d[0]), w1 = Hasher<HF>::native(d[1]), w2 = Hasher<HF>::native(d[2]),
                               w3 = Hasher<HF>::native(d[3]);
                if (w0 < 4294967294u && w1 < 4294967294u && w2 < 4294967294u && w3 < 4294967294u) {
                    alpha = {m31_red(w0), m31_red(w1), m31_red(w2), m31_red(w3)};
                    break;
                }
            }
            if (t == 0) {
                stq4(alphas_out + 4 * j, alpha);
                if (np > 64) { lds_alpha[0] = alpha.a; lds_alpha[1] = alpha.b; lds_alpha[2] = alpha.c; lds_alpha[3] = alpha.d; }
            }
        }
        if (np > 64) {
            __syncthreads();
            alpha = QM31{lds_alpha[0], lds_alpha[1], lds_alpha[2], lds_alpha[3]};
        }

        // ---- fold, and hand the folds over as the next layer's pairs
        if (two) {
            const uint32_t *in = layer + 16 * (size_t)t;
            const QM31 o0 = fri_fold(ldq4(in), ldq4(in + 4), c0, alpha), o1 = fri_fold(ldq4(in + 8), ldq4(in + 12), c1, alpha);
            stq4(fold + 8 * t, o0);
            stq4(fold + 8 * t + 4, o1);
            v0 = o0; v1 = o1;  // pair t of the next layer
        } else {
            QM31 o = qm31_zero();
            if (t < np) {
                o = fri_fold(v0, v1, c0, alpha);
                stq4(fold + 4 * t, o);
            }
            if (j + 1 < n_layers) {
                if (np > 64) {
                    uint32_t *tile = lds_b;  // (its last reader as a node buffer is behind the alpha barrier)
                    if (t < np) {
                        tile[0 * kTailThreads + t] = o.a; tile[1 * kTailThreads + t] = o.b;
                        tile[2 * kTailThreads + t] = o.c; tile[3 * kTailThreads + t] = o.d;
                    }
                    __syncthreads();
                    if (t < (np >> 1)) {
                        const uint2 a = *reinterpret_cast<const uint2 *>(tile + 0 * kTailThreads + 2 * t);
                        const uint2 b = *reinterpret_cast<const uint2 *>(tile + 1 * kTailThreads + 2 * t);
                        const uint2 c = *reinterpret_cast<const uint2 *>(tile + 2 * kTailThreads + 2 * t);
                        const uint2 d = *reinterpret_cast<const uint2 *>(tile + 3 * kTailThreads + 2 * t);
                        v0 = QM31{a.x, b.x, c.x, d.x};
                        v1 = QM31{a.y, b.y, c.y, d.y};
                    }
                } else {
                    v0 = lane_q(o, ln0);
                    v1 = lane_q(o, ln1);
                }
            }
        }
        tree += 18 * (size_t)n;
        cinv += np;
        n = np;
    }

    if (t == 0) channel_store(ch, state);
}

}  // namespace
}  // namespace ss

extern "C" uint32_t ss_p_fri_tail_log(void) { return kTailLog; }

extern "C" size_t ss_p_fri_tail_words(uint32_t log_n, uint32_t n_layers)
{
    if (log_n < 1 || log_n > kTailLog || n_layers < 1 || n_layers > log_n) return 0;
    const size_t n0 = (size_t)1 << log_n, n_last = n0 >> (n_layers - 1);
    return 36 * (n0 - n_last) + 18 * n_last;
}

extern "C" int ss_p_fri_tail_dev(ss_ctx *ctx, uint32_t hash, uint32_t log_n, uint32_t n_layers, uint32_t *state_dev,
                                 const uint32_t *layer_dev, const uint32_t *coord_inv_dev, uint32_t *arena_dev,
                                 uint32_t *roots_out_dev, uint32_t *alphas_out_dev, void *stream)
{
    SS_DEVICE_GUARD(ctx);
    if (!state_dev || !layer_dev || !coord_inv_dev || !arena_dev || !roots_out_dev || !alphas_out_dev || hash > 1 ||
        log_n < 1 || log_n > kTailLog || n_layers < 1 || n_layers > log_n)
        return ss_internal_set_err(SS_ERR_ARG, "ss_p_fri_tail_dev: bad argument");
    // values, nodes, roots and alphas move as 16-byte words
    if ((((uintptr_t)layer_dev | (uintptr_t)arena_dev | (uintptr_t)roots_out_dev | (uintptr_t)alphas_out_dev) & 15u) != 0)
        return ss_internal_set_err(SS_ERR_ARG, "ss_p_fri_tail_dev: layer, arena, roots and alphas need 16-byte alignment");
    const uint32_t pairs = 1u << (log_n - 1);
    const uint32_t threads = pairs >= kTailThreads ? kTailThreads : (pairs + 63u) / 64u * 64u;  // a pair each, whole wavefronts
    if (hash)
        hipLaunchKernelGGL(p_fri_tail_kernel<1>, dim3(1), dim3(threads), 0, (hipStream_t)stream, log_n, n_layers, state_dev,
                           layer_dev, coord_inv_dev, arena_dev, roots_out_dev, alphas_out_dev);
    else
        hipLaunchKernelGGL(p_fri_tail_kernel<0>, dim3(1), dim3(threads), 0, (hipStream_t)stream, log_n, n_layers, state_dev,
                           layer_dev, coord_inv_dev, arena_dev, roots_out_dev, alphas_out_dev);
    HIP_TRY(hipGetLastError());
    return SS_OK;
}
