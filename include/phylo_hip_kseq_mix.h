/*
 * phylo_hip_kseq_mix.h -- the K-state sequence likelihood under a mixture of
 * M reversible models over sites, each with C rate categories (codon site
 * models: one omega per component):
 *
 *   L_i = sum_m sum_c ps[m][c] L_i(Q_m, t rs[m][c], pi_m),  log L = sum_i w_i log L_i
 *
 * Each Q_m is normalised by its own s_m = 2 sum_{i<j} rates_m,ij pi_m,i pi_m,j;
 * a class proportion and any common rate scale go into ps and rs.  Included by
 * phylo_hip_kseq.h, whose conventions (tipmasks, peel, blens, the order of the
 * rates) hold unchanged: phy_kseq_* is the M = 1 case of the same kernels, and
 * phy_kseq_mix_eval at M = 1 returns phy_kseq_eval's rows bit for bit.
 *
 *   params[n][M (R + K) + 2 M C]   [rates_0 R][freqs_0 K] .. [rates_{M-1}]
 *                    [freqs_{M-1}][rs M C][ps M C], rs and ps component by
 *                    component
 *   rows[n][1 + B + 2 M C + M (R + K)]   [log L][d/dblens B][d/drs M C]
 *                    [d/dps M C][d/drates_0 R][d/dfreqs_0 K] .. ; d/dfreqs_m is
 *                    total: through Q_m, s_m, the D^{+-1/2} factors and the root
 *                    term of component m
 *   site_ll[n][P]    log L_i, or NULL
 *   class_post[n][M][P]   sum_c ps[m][c] L_imc / L_i, the posterior probability
 *                    of component m at pattern i, or NULL.  It is taken on the
 *                    pattern's shared power-of-two shift, so it is exact however
 *                    far the components' shifts differ; 0 for a component with
 *                    no live category
 *
 * Limits: 1 <= M <= 8 and M C <= 16.
 *
 * Contracts:
 *   - phy_kseq_mix_create makes every refusal (PHY_EINVAL, the message names
 *     the argument and, for the peel, the row) before the first device call: on
 *     a machine without a device a bad argument yields its own message;
 *   - a draw without a likelihood (in any component a frequency that is not
 *     positive, a negative or non-finite rate, or an eigensolve that does not
 *     converge; a negative or non-finite rs, ps or branch length; L_i that is
 *     not positive and finite at a pattern of positive weight; a log L that is
 *     not finite) gives -inf followed by zeros, site_ll = -inf and class_post
 *     = 0, with status 0; the other draws of the call are untouched.  A
 *     component whose weights are all 0 is no refusal: it is never alive;
 *   - partials are rescaled by powers of two per node, pattern and (component,
 *     category), and a pattern's smallest shift is taken over all its live
 *     (component, category) pairs;
 *   - a draw's row, site_ll and class_post are bitwise repeatable: they do not
 *     depend on n_draws, on the draw's position in the call, or on max_draws.
 *
 * All arithmetic is fp64.  The device holds 3 (2S-1) 16 ceil(K / 16) 16 doubles
 * per (component, category, 16-pattern tile) of a draw in flight; the draws in
 * flight follow from a fixed budget (1 GiB), and a shape whose single draw
 * passes it is refused.
 */
#ifndef PHYLO_HIP_KSEQ_MIX_H
#define PHYLO_HIP_KSEQ_MIX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The context type of phy_kseq_create under the mixture's name. */
typedef struct phy_kseq_ctx phy_kseq_mix_ctx;

/* max_draws: most draws one eval call may take. */
int phy_kseq_mix_create(int S, int P, int K, int M, int C, int rooted, const uint64_t* tipmasks,
                        const double* weights, const int32_t* peel, int max_draws, int device,
                        phy_kseq_mix_ctx** out);
int phy_kseq_mix_destroy(phy_kseq_mix_ctx* ctx);
int phy_kseq_mix_num_branches(const phy_kseq_mix_ctx* ctx); /* B; -1 for NULL */
int phy_kseq_mix_row_len(const phy_kseq_mix_ctx* ctx);      /* 1 + B + 2MC + M(R + K); -1 for NULL */

/* Host buffers, synchronous.  PHY_EINVAL: a NULL ctx or buffer; PHY_ERANGE:
 * n_draws outside 1..max_draws. */
int phy_kseq_mix_eval(phy_kseq_mix_ctx* ctx, int n_draws, const double* blens, const double* params, double* rows,
                      double* site_ll, double* class_post);

/* Diagnostics, as phylo_hip_diag.h's phy_kseq_plan and phy_kseq_info.  The plan
 * without a device or a context: facts[16] as phy_kseq_plan, items per draw
 * being M C tiles.  facts may be NULL. */
int phy_kseq_mix_plan(int S, int P, int K, int M, int C, int rooted, const uint64_t* tipmasks, const double* weights,
                      const int32_t* peel, int max_draws, int cu_count, long long* facts);
/* The live plan and the Jacobi sweeps of the last call's first n draws,
 * sweeps[n][M] (-1: refused before the eigensolve).  Either may be NULL. */
int phy_kseq_mix_info(const phy_kseq_mix_ctx* ctx, int n, int32_t* sweeps, long long* facts);

#ifdef __cplusplus
}
#endif
#endif /* PHYLO_HIP_KSEQ_MIX_H */
