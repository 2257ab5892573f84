/*
 * ss_prover_fri.h -- the FRI commit of the layers that fit in ONE workgroup, in one launch.
 *
 * The commit loop of stark-symphony_amd/prover.py spends four to six dependent launches per layer (leaf hashes, one
 * launch per wide Merkle level, the tree's tail, the channel, the fold).  Once a layer is a few thousand QM31 values
 * each of them occupies a handful of CUs for a few microseconds and the loop is a chain of dispatch latencies.
 * ss_p_fri_tail_dev commits such a layer AND every layer after it in one launch of one workgroup: leaves, tree,
 * fri_layer_commit (channel mix + alpha draw) and fold, with the channel held in the registers of one wavefront from
 * the first layer to the last (csrc/ss_prover_fri.hip).  The bits are those of ss_p_hash_qm31,
 * ss_p_merkle, ss_p_channel_fri_layer and ss_p_fri_fold_dev run in turn.
 * Included by ss_prover.h (tests/test_host.py pins the entry count of ss_prover.h itself).
 */
#ifndef SS_PROVER_FRI_H
#define SS_PROVER_FRI_H

#include <stddef.h>
#include <stdint.h>

#include "ss_verify.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Largest log2 layer size the tail kernel takes (a compile-time constant of the library, >= 10). */
uint32_t ss_p_fri_tail_log(void);

/* Words of the arena below: 36 (2^log_n - n_last) + 18 n_last with n_last = 2^(log_n - n_layers + 1); 0 for arguments
 * ss_p_fri_tail_dev refuses.                                                                                        */
size_t ss_p_fri_tail_words(uint32_t log_n, uint32_t n_layers);

/* fri_layer_commit + fold (fri/commit.simf:34-46, 70-85; fri/folding.simf:15-41) for n_layers consecutive layers,
 * starting from a layer of 2^log_n QM31 values, in ONE launch of ONE workgroup.
 *
 * Arena: for layer j = 0 .. n_layers - 1 with n_j = 2^(log_n - j), block j starts at word 36 (2^log_n - n_j) and holds
 *   the tree   [2 n_j][8] words in ss_p_merkle's layout (leaves first, root in row 2 n_j - 2, row 2 n_j - 1 untouched),
 *   the fold   [n_j / 2][4] words: the next layer (the last block's fold is the proof's last layer).
 * Every word of the used rows is written exactly once: the arena may be uninitialised.  roots_out_dev[j] = the root of
 * tree j (stored words), alphas_out_dev[j] = the alpha drawn after it; state_dev is read once and written once.
 * SS_ERR_ARG, with nothing launched: log_n < 1, log_n > ss_p_fri_tail_log(), n_layers < 1, n_layers > log_n, hash > 1,
 * a null pointer.                                                                                                     */
int ss_p_fri_tail_dev(ss_ctx *ctx, uint32_t hash, uint32_t log_n, uint32_t n_layers,
                      uint32_t *state_dev,            /* [9] channel, in/out, as ss_p_channel_fri_layer */
                      const uint32_t *layer_dev,      /* [2^log_n][4] */
                      const uint32_t *coord_inv_dev,  /* inverse twiddles of the first layer; the next layers'
                                                         follow contiguously (ss_p_twiddles' layout) */
                      uint32_t *arena_dev, uint32_t *roots_out_dev /* [n_layers][8] */,
                      uint32_t *alphas_out_dev /* [n_layers][4] */, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SS_PROVER_FRI_H */
