/*
 * ss_prover_pow.h -- the end of the transcript with the proof of work ground by the WHOLE GPU, in one launch.
 *
 * ss_p_finish_dev (ss_prover_record.h) searches the nonce in one workgroup: one compute unit hashes and the others
 * idle, which is fine at the 5 bits of the fixtures and hopeless at the 20 to 30 bits a deployment grinds.
 * ss_p_finish_grid_dev does the same steps and writes the same words, with the search spread over a grid of
 * persistent workgroups that claim chunks of consecutive nonces from a counter in device memory and never wait for
 * one another (csrc/ss_prover_pow.hip).  The smallest nonce is unique, so nothing a verifier sees differs.
 * Included by ss_prover.h (tests/test_host.py pins the entry count of ss_prover.h itself).
 */
#ifndef SS_PROVER_POW_H
#define SS_PROVER_POW_H

#include <stddef.h>
#include <stdint.h>

#include "ss_prover_record.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ss_p_finish_dev with the nonce search on the whole device: the same arguments, the same words in state_dev,
 * queries_out_dev and nonce_out_dev, the same bits in *err_dev (SS_P_ERR_LAST_LAYER; SS_P_ERR_POW_SPAN: no nonce in
 * [0, span), state_dev left as it came, queries 0).  span is a full 64-bit count.
 *   work_dev[3]  three 64-bit words (chunk counter, smallest hit, workgroups gone) the launch needs ZERO when it
 *                starts and leaves zero when it ends: the caller zeroes them once, when it allocates them, and then
 *                passes them to any number of calls ONE AT A TIME (calls on one stream; proofs in flight on several
 *                streams need a triple each).
 * SS_ERR_ARG, with nothing launched: a null pointer, hash > 1, span == 0, n_last == 0, lde_log / n_queries outside the
 * layout's range, last_dev not 16-byte aligned, work_dev not 8-byte aligned.                                          */
int ss_p_finish_grid_dev(ss_ctx *ctx, uint32_t hash, uint32_t lde_log, uint32_t n_queries, uint64_t pow_target,
                         uint64_t span, uint32_t *state_dev, const uint32_t *last_dev, size_t n_last,
                         uint32_t *queries_out_dev, uint32_t *nonce_out_dev, uint32_t *err_dev, uint64_t *work_dev,
                         void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SS_PROVER_POW_H */
