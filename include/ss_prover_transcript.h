/*
 * ss_prover_transcript.h -- the Fiat-Shamir transcript of a proof on the GPU from its first mix up to the FRI commit:
 * the three places where a caller of ss_prover.h used to leave HIP (draw cp_alpha, draw the OODS point and sample,
 * draw deep_alpha and prepare the DEEP quotients), as six entries that read what they depend on from device memory.
 * Included by ss_prover.h (tests/test_host.py pins the entry count of ss_prover.h itself).  Entries 1, 3, 4 and 5 live
 * in csrc/ss_prover_transcript.hip, entries 2 and 6 beside the kernels they share a body with in csrc/ss_prover.hip.
 *
 * Chained with ss_p_channel_fri_layer / ss_p_fri_fold_dev and ss_prover_record.h, a whole proof is enqueued without a
 * host read.  All entries are asynchronous on `stream`, validate their arguments on the host (SS_ERR_ARG) and take
 * `hash` 0 (SHA-256) or 1 (Blake2s) where they hash.  state_dev[9] is the channel as ss_p_channel_fri_layer defines
 * it: 8 stored digest words + the draw counter.  err_dev is the word of ss_prover_record.h: a draw that exhausts the
 * reference's 256 tries (channel.simf:115-140) or a non-invertible 1 + t^2 ORs SS_P_ERR_TRANSCRIPT into it; every
 * output is written with defined values all the same (a failed draw gives 0).
 */
#ifndef SS_PROVER_TRANSCRIPT_H
#define SS_PROVER_TRANSCRIPT_H

#include <stddef.h>
#include <stdint.h>

#include "ss_verify.h"

#ifdef __cplusplus
extern "C" {
#endif

/* log2 of the tile of ss_p_eval_at_point_dev: one workgroup folds 2^12 coefficients (16 KB) to one QM31. */
#define SS_P_EVAL_TILE_LOG 12u

/* 1. channel_init; mix const_root[8] (host, stored words); mix the trace root trace_root_dev[8] (the last row of the
 * trace tree's `levels`); cp_alpha_out_dev[4] <- draw_qm31; state_dev[9] <- the channel.  One lane.                  */
int ss_p_channel_begin_dev(ss_ctx *ctx, uint32_t hash, const uint32_t const_root[8], const uint32_t *trace_root_dev,
                           uint32_t *state_dev, uint32_t *cp_alpha_out_dev, uint32_t *err_dev, void *stream);

/* 2. ss_p_composition with alpha read from device memory (alpha_dev[4], written by entry 1). */
int ss_p_composition_dev(ss_ctx *ctx, uint32_t n_log, uint32_t n_cols, const uint32_t *ev, const uint32_t *hx_c,
                         const uint32_t *alpha_dev, uint32_t *out, void *stream);

/* 3. Mix the composition root cp_root_dev[8]; draw t; P = ((1 - t^2) / (1 + t^2), 2t / (1 + t^2)) and 2P
 * (channel.simf:143-151).  One lane.
 *   points_out_dev[16]                  px, py, p2x, p2y
 *   factors_p_out_dev[trace_log][4]     y, x, pi(x), pi^2(x), ... of P: the fold factors of a trace column
 *   factors_2p_out_dev[trace_log-1][4]  x, pi(x), ... of 2P: the composition columns have no y term and are held
 *                                       compact (may be NULL when trace_log = 1)                                    */
int ss_p_oods_point_dev(ss_ctx *ctx, uint32_t hash, uint32_t trace_log, uint32_t *state_dev, const uint32_t *cp_root_dev,
                        uint32_t *points_out_dev, uint32_t *factors_p_out_dev, uint32_t *factors_2p_out_dev,
                        uint32_t *err_dev, void *stream);

/* 4. out[ncols][4] <- `ncols` columns of 2^m M31 coefficients (stride col_stride words) evaluated at the point whose m
 * QM31 fold factors are factors_dev[m][4], bit 0 first: the words ss_p_eval_at_point_batch gives, in
 * ceil(m / SS_P_EVAL_TILE_LOG) launches instead of m (two up to m = 24).  A workgroup folds one tile of 2^12
 * coefficients of one column to one QM31: four levels in registers, six between the lanes of a wavefront, two through
 * LDS; the next launch folds the partials the same way.  scratch_dev: ss_p_eval_scratch_words(m, ncols) words (may be
 * NULL when that is 0, i.e. m <= 12).                                                                               */
size_t ss_p_eval_scratch_words(uint32_t m, uint32_t ncols);
int ss_p_eval_at_point_dev(ss_ctx *ctx, uint32_t m, uint32_t ncols, const uint32_t *coeffs, size_t col_stride,
                           const uint32_t *factors_dev, uint32_t *scratch_dev, uint32_t *out, void *stream);

/* 5. Mix the n_cols + 16 samples samples_dev[.][4] (trace columns first: channel_mix_oods_evals); draw deep_alpha; for
 * column k of each batch (trace columns at P, composition columns at 2P) the interpolant of deep/quotients.simf:25-36
 * times alpha^(k+1).  points_dev[16]: what entry 3 wrote.  One workgroup; the powers are a prefix product over lanes.
 *   bcoef_out_dev[n_cols + 16][4]   the b coefficients ss_p_quotients takes
 *   sums_alpha16_out_dev[20]        A1, C1, A2, C2, alpha^16                                                       */
int ss_p_deep_coeffs_dev(ss_ctx *ctx, uint32_t hash, uint32_t n_cols, uint32_t *state_dev, const uint32_t *samples_dev,
                         const uint32_t *points_dev, uint32_t *bcoef_out_dev, uint32_t *sums_alpha16_out_dev,
                         uint32_t *err_dev, void *stream);

/* 6. ss_p_quotients with p, p2 = points_dev[16] and sums_alpha16_dev[20] read from device memory. */
int ss_p_quotients_dev(ss_ctx *ctx, uint32_t lde_log, uint32_t n_cols, const uint32_t *trace_lde, const uint32_t *cp_lde,
                       uint32_t cp_log, const uint32_t *hx_hy, const uint32_t *bcoef, const uint32_t *points_dev,
                       const uint32_t *sums_alpha16_dev, uint32_t *out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SS_PROVER_TRANSCRIPT_H */
