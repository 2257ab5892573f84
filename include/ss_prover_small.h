/*
 * ss_prover_small.h -- a batch of SMALL proofs in one launch, one workgroup per proof.
 *
 * GpuProver.prove_record enqueues about fifty launches per proof, and at the reference's own shape (2^9 rows x 4
 * columns, LDE 2^13) what a proof costs is those launches and the host thread behind them, not the 40 k hash
 * compressions it is made of.  ss_p_prove_small_dev proves n such proofs in ONE launch: a workgroup owns a whole proof
 * from the trace to the last word of the verifier's per-query record and runs every phase of prover.py's _commit
 * (device transcript), ss_p_finish_dev and ss_p_decommit_record between workgroup barriers (csrc/ss_prover_small.hip,
 * DESIGN.md 7).  Workgroup g proves g, g + n_groups, g + 2 n_groups, ... in its own slot of an arena; workgroups never
 * read each other's memory and never wait for one another.  The words are those of prove_record(transcript="device").
 * Included by ss_prover.h (tests/test_host.py pins the entry count of ss_prover.h itself).
 */
#ifndef SS_PROVER_SMALL_H
#define SS_PROVER_SMALL_H

#include <stddef.h>
#include <stdint.h>

#include "ss_prover_record.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The tables of ss_p_twiddles the kernel reads (device memory, shared read-only by all workgroups), n = trace_log,
 * L = lde_log.  hxhy = hx_out with the table's layer 0 (the pairs' y) copied behind it, 2^m words.                   */
typedef struct ss_p_small_tables {
    const uint32_t *itw_n;                       /* inverse twiddles of the coset of log size n                     */
    const uint32_t *tw_c, *itw_c, *hxhy_c;       /* of log size n + 1 (the composition's coset)                     */
    const uint32_t *tw_l, *itw_l, *hxhy_l;       /* of log size L                                                   */
} ss_p_small_tables;

/* The largest lde_log, n_cols and n_queries the kernel serves (compile-time constants of the library: 13, 32, 64),
 * for either hash.  Any of the pointers may be NULL.                                                                 */
void ss_p_small_limits(uint32_t *lde_log_out, uint32_t *n_cols_out, uint32_t *n_queries_out);

/* Words of arena for n_groups resident workgroups (a slot each, reused from proof to proof); 0 for a cfg the kernel
 * refuses or n_groups == 0.                                                                                          */
size_t ss_p_small_arena_words(const ss_stwo_cfg *cfg, size_t n_groups);

/* For every i < n: row i of records_out_dev (rows row_stride_words apart) <- the ss_stwo_record_words(cfg) words of
 * the record of the proof of seed seeds_dev[i] (the trace's seed term is (seed * 0x9E3779B1) mod (2^31 - 1)), every word
 * written exactly once and none behind them; err_dev[i] <- the SS_P_ERR_* bits of that proof (stored, not ORed: the
 * array may be uninitialised).  With SS_P_ERR_POW_SPAN (no nonce in [0, pow_span)) the row's content is unspecified.
 *   cfg         n_cols <= 32, 2 <= lde_log <= 13, 1 <= trace_log < lde_log, n_layers == trace_log - 1, n_queries <= 64
 *   n_groups    workgroups launched (<= n); 0 = choose: two per compute unit, never more than n or than arena_words holds
 *   arena_dev   arena_words >= ss_p_small_arena_words(cfg, n_groups) words, 16-byte aligned, may be uninitialised
 *   const_root  (host) the stored words of the constant commitment's root, H("")
 * Asynchronous on `stream`.  SS_ERR_ARG, with nothing launched: a cfg outside those limits, n == 0, n_groups > n,
 * pow_span == 0, row_stride_words < the record's words, a null pointer, an arena that is not 16-byte aligned or too small
 * for n_groups slots (for one, when n_groups == 0).                                                                  */
int ss_p_prove_small_dev(ss_ctx *ctx, const ss_stwo_cfg *cfg, uint64_t pow_target, uint64_t pow_span,
                         const uint64_t *seeds_dev, size_t n, size_t n_groups, const ss_p_small_tables *tables,
                         const uint32_t const_root[8], uint32_t *arena_dev, size_t arena_words, uint32_t *records_out_dev,
                         size_t row_stride_words, uint32_t *err_dev, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SS_PROVER_SMALL_H */
