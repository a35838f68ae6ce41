/*
 * phylo_hip_kseq_sum.h -- posterior summaries of the K-state sequence
 * likelihood (codon models): per draw the state posteriors of the internal
 * nodes and the expected number of labelled substitutions on each branch (for
 * codon models the synonymous and nonsynonymous counts).  Included by
 * phylo_hip_kseq.h.  The calls follow phylo_hip_seqsum.h.
 *
 * A summary context is a mixture context (phylo_hip_kseq_mix.h: S, P, K, M, C,
 * rooted, tipmasks, weights, peel, max_draws, device; M = 1 is the single model)
 * plus 1 <= n_labels <= 4 labellings of the unordered state pairs:
 *
 *   labels[n_labels][R]   finite, non-negative weights lab_l[x,y] = lab_l[y,x]
 *                    in the order of the rates (phylo_hip_kseq.h)
 *
 * blens[n][B] and params[n][M (R + K) + 2 M C] are phy_kseq_mix_eval's.
 *
 *   loglik[n]        log L
 *   bcounts[n][n_labels][B]   bcounts[l][b] = sum_i w_i E[ sum over the
 *                    substitutions x -> y on the edge above node b of
 *                    lab_l[x,y] | column i ], the expectation under the
 *                    mixture: per (component, category) the integral
 *                    int_0^t P(s) (Q o lab_l) P(t - s) ds, t = blens[b] rs, on
 *                    the normalised Q.  The merged root edge of an unrooted
 *                    tree follows blens' convention
 *   node_post[n][S-1][K][P]   node_post[v - S][j][i]: the posterior probability
 *                    that internal node v (S .. 2S-2) is in state j at pattern
 *                    i; or NULL
 *
 * Contracts:
 *   - phy_kseq_sum_create makes every refusal of phy_kseq_mix_create, and
 *     refuses n_labels outside 1..4, a NULL labels, a negative or non-finite
 *     label (PHY_EINVAL, the message names the argument) and a node_post row
 *     (S-1) K P longer than 2^31 - 1 doubles, all before the first device call;
 *   - loglik[d] carries the bits of phy_kseq_mix_eval's row[0] for the same
 *     draw: the eigen, way-up and site phases are the same kernels;
 *   - a draw without a likelihood (phy_kseq_mix_eval's conditions) gives -inf
 *     and zeros, with status 0; phy_kseq_sum_add leaves it out of the sum and
 *     out of n_finite; the other draws of the call are untouched;
 *   - every (v, i) of node_post sums to one over the K states wherever L_i is
 *     positive and finite, patterns of weight zero included; a pattern of
 *     weight zero contributes nothing to bcounts;
 *   - a branch of length zero, and a category with rs = 0, have counts
 *     exactly 0;
 *   - on an unrooted tree the root 2S-2 and the merged child 2S-3 describe the
 *     same point, and their posteriors are equal;
 *   - node_post sums over (component, category) in ascending order, bcounts
 *     over (component, category, pattern tile) in one fixed order; a draw's
 *     outputs are bitwise independent of n_draws, of its position in the
 *     call, of max_draws and of the draws in flight.  After phy_kseq_sum_reset,
 *     phy_kseq_sum_read returns bit for bit the left-to-right fp64 sum (from
 *     +0) of the finite draws' node_post as phy_kseq_sum_eval returns them,
 *     however the draws were split into phy_kseq_sum_add calls;
 *   - no atomics.
 *
 * All arithmetic is fp64.  Beside the mixture context's memory the device
 * holds n_labels 16 ceil(K/16) 16 ceil(K/16) doubles per (draw, component) of a
 * call and (S-1) K P doubles per draw in flight and for the running sum.
 */
#ifndef PHYLO_HIP_KSEQ_SUM_H
#define PHYLO_HIP_KSEQ_SUM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct phy_kseq_sum_ctx phy_kseq_sum_ctx;

/* max_draws: most draws one eval or add call may take. */
int phy_kseq_sum_create(int S, int P, int K, int M, int C, int rooted, const uint64_t* tipmasks,
                        const double* weights, const int32_t* peel, int n_labels, const double* labels,
                        int max_draws, int device, phy_kseq_sum_ctx** out);
int phy_kseq_sum_destroy(phy_kseq_sum_ctx* ctx);
int phy_kseq_sum_num_branches(const phy_kseq_sum_ctx* ctx); /* B; -1 for NULL */

/* Host buffers, synchronous.  PHY_EINVAL: a NULL ctx or buffer (node_post may
 * be NULL); PHY_ERANGE: n_draws outside 1..max_draws. */
int phy_kseq_sum_eval(phy_kseq_sum_ctx* ctx, int n_draws, const double* blens, const double* params, double* loglik,
                      double* bcounts, double* node_post);

/* The running sum of node_post on the device: reset zeroes it, add joins the
 * finite draws of a call to it (loglik and bcounts come back per draw), read
 * returns it [S-1][K][P] with the number of draws in it (n_finite may be
 * NULL). */
int phy_kseq_sum_reset(phy_kseq_sum_ctx* ctx);
int phy_kseq_sum_add(phy_kseq_sum_ctx* ctx, int n_draws, const double* blens, const double* params, double* loglik,
                     double* bcounts);
int phy_kseq_sum_read(phy_kseq_sum_ctx* ctx, double* node_post_sum, int* n_finite);

#ifdef __cplusplus
}
#endif
#endif /* PHYLO_HIP_KSEQ_SUM_H */
