/*
 * phylo_hip_part.h -- the partitioned boundary of the sequence likelihood: K
 * disjoint site sets (partitions) of one alignment on the same S taxa and ONE
 * tree.  Every partition has its own model vector theta_k and a relative
 * rate mu_k > 0; the branch lengths t are shared:
 *
 *   log L(t, mu, theta) = sum_k log L_k(mu_k t; theta_k)
 *   d/dt_b  = sum_k mu_k g_kb      g_k = dlog L_k / d(its scaled lengths)
 *   d/dmu_k = sum_b t_b g_kb
 *
 * The workload it serves is the codon-position or per-gene split of a
 * protein-coding alignment; with one phy_ctx per partition that is K contexts
 * and K latency-bound calls per gradient.
 *
 * Included by phylo_hip.h, whose conventions hold unchanged:
 *   - the partitions share the model family, C categories and rootedness;
 *   - tipcodes[S][sum P_k] and weights[sum P_k] hold the partitions' patterns
 *     side by side, partition 0 first;
 *   - a partition's compact row is phy_eval's: 1 + B + 2C + 14 doubles
 *     (log-likelihood, dlogL/d(scaled blens), drs, dps, dfreqs (root), the six
 *     exchangeabilities, dfreqs (total));
 *   - a draw's output row is [log L][d/dt B], then per partition
 *     [d/dmu_k][the 2C + 14 tail of that partition's row];
 *   - a draw with a partition whose log-likelihood is not finite (a negative
 *     frequency, a NaN branch length or rate) returns -inf with status 0 and
 *     zeros; the other draws are untouched.
 *
 * Contract: the scaled lengths are the rounded fp64 products mu_k * t_b, and
 * the fold of a draw's K rows is fixed: log L the left-to-right sum over k,
 * d/dt_b the left-to-right sum over k of the rounded products mu_k * g_kb,
 * d/dmu_k the left-to-right sum over b of the rounded products t_b * g_kb; no
 * fused multiply-add, no atomics.  A row is bitwise repeatable: its bits do
 * not depend on n_draws, on the draw's position or on the other draws, only
 * on what fixes the context's plan (the sizes, the data, max_draws, the PHY_*
 * preferences at create).
 *
 * Not in the partitioned form (use a phy_ctx per partition): the rescaled
 * sweep, the class sweep, clade compression, the quad sweeps, multi-device
 * handles, device-buffer and asynchronous evaluation.  The padded alignment
 * is swept one workgroup per (draw, partition): alignments of 10^5 and more
 * patterns are the class sweep's workload, not this form's.
 */
#ifndef PHYLO_HIP_PART_H
#define PHYLO_HIP_PART_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct phy_part_ctx phy_part_ctx;

/* P_k[K]: patterns per partition.  peel: phy_create's form.  max_draws: most
 * draws one phy_part_eval may take.  PHY_EINVAL: K < 1, a partition with
 * P_k < 1 (the message names it), max_draws * K past 65,535 rows, and
 * everything phy_create refuses. */
int phy_part_create(int S, int K, const int32_t* P_k, int C, int rooted, int model, const uint8_t* tipcodes,
                    const double* weights, const int32_t* peel, int max_draws, int device, phy_part_ctx** out);
int phy_part_destroy(phy_part_ctx* ctx);
int phy_part_num_partitions(const phy_part_ctx* ctx); /* K; -1 for NULL */
int phy_part_num_branches(const phy_part_ctx* ctx);   /* B */
int phy_part_row_len(const phy_part_ctx* ctx);        /* 1 + B + 2C + 14 */
int phy_part_output_len(const phy_part_ctx* ctx);     /* 1 + B + K (1 + 2C + 14) */

/* n_draws draws, host buffers, synchronous: blens[n][B] (shared), mu[n][K],
 * model[n][K][PHY_MODEL_LEN(C)], out[n][phy_part_output_len()];
 * part_rows[n][K][phy_part_row_len()] or NULL: the partitions' rows the fold
 * consumed (d/dblens with respect to the scaled lengths; a rejected
 * partition's row is -inf and zeros); site_ll[n][sum P_k] or NULL, in the
 * caller's pattern order.  PHY_ERANGE: n_draws outside 1..max_draws;
 * PHY_EINVAL: a NULL ctx, blens, mu, model or out. */
int phy_part_eval(phy_part_ctx* ctx, int n_draws, const double* blens, const double* mu, const double* model,
                  double* out, double* part_rows, double* site_ll);

#ifdef __cplusplus
}
#endif
#endif /* PHYLO_HIP_PART_H */
