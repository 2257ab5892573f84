/*
 * ss_prover_minimal.h -- the decommitment of a proof written by the GPU as the MINIMAL record of
 * include/ss_verify_forms.h ("minimal records": one sorted, deduplicated decommitment per tree, what upstream stwo's
 * prover sends), and the packing of a batch of such variable-length records into the back-to-back form with an offset
 * table that ss_stwo_verify_minimal_dev reads.  Included by ss_prover.h (tests/test_host.py pins the entry count of
 * ss_prover.h itself); the entries live in csrc/ss_prover_minimal.hip.
 *
 * Where the per-query record of ss_prover_record.h is a gather of fixed shape, a minimal record's shape is data: which
 * siblings and fold partners are sent and where every list starts depends on the queries, which exist only at the very
 * end of the transcript, in device memory.  So the decommitment plans the layout on the device (sort, deduplicate,
 * Lone(a) per level, list offsets), gathers into it and reports the size it made.  Both entries are asynchronous on
 * `stream`, read nothing back, validate their arguments on the host and return SS_ERR_ARG otherwise.
 */
#ifndef SS_PROVER_MINIMAL_H
#define SS_PROVER_MINIMAL_H

#include <stddef.h>
#include <stdint.h>

#include "ss_prover_record.h"
#include "ss_verify.h"

#ifdef __cplusplus
extern "C" {
#endif

/* minimal_out_dev[.. *words_out_dev) <- the minimal record of the proof whose queries are queries_dev[Q] (positions of
 * lde_log bits; higher bits are ignored); *words_out_dev <- its size in words, at most ss_stwo_minimal_max_words(cfg).
 * Every other argument is that of ss_p_decommit_record: the same ss_p_tree table (3 + n_layers entries in DEVICE memory,
 * the composition tree over the storage pairs with `leaf` = the pair leaf hashes), samples_dev[(n_cols + 16)][4],
 * fri_roots_dev[1 + n_layers][8], last_dev[4], nonce_dev[2] = hi, lo, const_root[8] on the host.
 * One launch.  Every workgroup recomputes the plan from the queries in LDS (one wavefront, one lane per query), then
 * one wavefront per (tree, level), per FRI layer and per (distinct position, commitment) moves that list's entries,
 * lane = sorted query.  Every word below the size is written exactly once and no word at or above it is touched:
 * minimal_out_dev may be uninitialised and needs 4-byte alignment only (a row of an [n][max_words] array).          */
int ss_p_decommit_minimal(ss_ctx *ctx, const ss_stwo_cfg *cfg, const ss_p_tree *trees_dev,
                          const uint32_t *samples_dev, const uint32_t *fri_roots_dev, const uint32_t *last_dev,
                          const uint32_t *nonce_dev, const uint32_t const_root[8], const uint32_t *queries_dev,
                          uint32_t *minimal_out_dev, uint32_t *words_out_dev, void *stream);

/* n records, record p in the first words_dev[p] words of row p of rows_dev (rows row_stride_words apart; a size above
 * the stride counts as the stride) -> the records back to back in packed_out_dev (room for the sum of the sizes; n *
 * row_stride_words always suffices) and offs_out_dev[n + 1], record p at word offs_out_dev[p], offs_out_dev[n] = the
 * total: what ss_stwo_verify_minimal_dev takes.  Two launches: one workgroup scans the sizes (64-bit offsets, a carry
 * between rounds of 256 records), then a grid of (chunk, record) copies.                                           */
int ss_p_minimal_pack_dev(ss_ctx *ctx, size_t n, const uint32_t *rows_dev, size_t row_stride_words,
                          const uint32_t *words_dev, uint32_t *packed_out_dev, uint64_t *offs_out_dev, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SS_PROVER_MINIMAL_H */
