/*
 * ss_prover_record.h -- the end of a proof on the GPU: the tail of the Fiat-Shamir transcript and the
 * decommitment, written as the verifier's per-query record (include/ss_verify.h, "Record
 * (ss_stwo_record_words words)") straight into device memory.  Included by ss_prover.h; the entries live in
 * csrc/ss_prover.hip with the other ss_p_* kernels (tests/test_host.py pins the entry count of ss_prover.h itself).
 *
 * After the FRI commit (ss_p_channel_fri_layer / ss_p_fri_fold_dev) a caller holds, all in device memory, the
 * channel state, the FRI roots, the last layer and every tree.  The two entries below turn that into a record
 * that ss_stwo_pack_dev / ss_stwo_verify_batch_dev consume, and nothing but one error word has to be read back.
 * Both are asynchronous on `stream`, validate their arguments on the host and return SS_ERR_ARG otherwise.
 */
#ifndef SS_PROVER_RECORD_H
#define SS_PROVER_RECORD_H

#include <stddef.h>
#include <stdint.h>

#include "ss_verify.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bits ss_p_finish_dev ORs into *err_dev (the caller zeroes the word once and reads it when it synchronises). */
#define SS_P_ERR_LAST_LAYER 1u /* the last FRI layer is not constant: the quotient is not of low degree      */
#define SS_P_ERR_POW_SPAN 2u   /* no nonce in [0, span): state, nonce and queries are NOT those of the proof */
#define SS_P_ERR_TRANSCRIPT 4u /* ss_prover_transcript.h: a draw_qm31 ran out of tries, or 1 + t^2 has no inverse */

/* The transcript after the FRI commit, one workgroup: check that the n_last QM31 values of the last layer are
 * all equal (else SS_P_ERR_LAST_LAYER; the steps below run all the same), mix last[0] (channel.simf:31-172), find
 * the SMALLEST nonce in [0, span) with LE64(last 8 bytes of H(digest || be8(nonce))) < pow_target (pow.simf:22-36),
 * mix it, draw n_queries positions of lde_log bits (fri/queries.simf:29-43).
 *   state_dev[9]        in: the channel as ss_p_channel_fri_layer leaves it; out: the channel after the draws
 *   queries_out_dev[Q]  nonce_out_dev[2] = hi, lo
 * SS_P_ERR_POW_SPAN: state_dev is left as it came (the caller can redo the tail with ss_p_pow), queries are 0.   */
int ss_p_finish_dev(ss_ctx *ctx, uint32_t hash, uint32_t lde_log, uint32_t n_queries, uint64_t pow_target,
                    uint64_t span, uint32_t *state_dev, const uint32_t *last_dev, size_t n_last,
                    uint32_t *queries_out_dev, uint32_t *nonce_out_dev, uint32_t *err_dev, void *stream);

/* One committed tree of a proof, as the decommitment reads it.  Entry 0 = trace, 1 = composition, 2 + l = FRI layer l.
 *   levels  the tree's nodes as ss_p_merkle leaves them ([2n - 1][8], leaves first); n = 2^lde_log leaves for the
 *           trace, 2^(lde_log - l) for FRI layer l; for the composition the tree over the 2^(lde_log - 1) storage
 *           PAIRS that ss_p_merkle_dup starts (the two leaves of a pair are equal and exist nowhere)
 *   values  trace: the LDE columns (stride 2^lde_log words); composition: its 16 columns, one value per pair
 *           (stride 2^(lde_log - 1)); FRI layer l: the layer, [2^(lde_log - l)][4]
 *   leaf    composition only: the 2^(lde_log - 1) leaf hashes of the pairs ([.][8]); NULL otherwise            */
typedef struct ss_p_tree {
    const uint32_t *levels;
    const uint32_t *values;
    const uint32_t *leaf;
} ss_p_tree;

/* record_out_dev[ss_stwo_record_words(cfg)] <- the record of the proof whose queries are queries_dev[Q]
 * (positions of lde_log bits; higher bits are ignored).  trees_dev: 3 + n_layers ss_p_tree in DEVICE memory;
 * samples_dev[(n_cols + 16)][4]: the OODS samples, trace columns first; fri_roots_dev[1 + n_layers][8];
 * last_dev[4]; nonce_dev[2] = hi, lo; const_root[8] (host): the stored words of the constant commitment's root.
 * One wavefront per authentication chain (tree, query): lane 2 * level + half moves 16 bytes of that level's
 * sibling from `levels` into the chain's slot; the same wavefront moves the chain's queried values.  Every word of
 * the record is written exactly once, hashes in the word order the trees hold: record_out_dev may be uninitialised
 * and needs 4-byte alignment only (a row of an [n][record_words] array).                                     */
int ss_p_decommit_record(ss_ctx *ctx, const ss_stwo_cfg *cfg, const ss_p_tree *trees_dev,
                         const uint32_t *samples_dev, const uint32_t *fri_roots_dev, const uint32_t *last_dev,
                         const uint32_t *nonce_dev, const uint32_t const_root[8], const uint32_t *queries_dev,
                         uint32_t *record_out_dev, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SS_PROVER_RECORD_H */
