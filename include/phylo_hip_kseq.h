/*
 * phylo_hip_kseq.h -- the K-state sequence likelihood: an alignment of P
 * patterns and C rate categories on one tree under a reversible model of
 * 2 <= K <= 64 states (codon models are K = 61).  One context holds one
 * alignment and one tree; a call takes n parameter points and returns, per
 * draw, the row
 *
 *   [log L][d/dblens B][d/drs C][d/dps C][d/drates R][d/dfreqs K]
 *
 * and, if asked, the site log-likelihoods [P].  R = K (K - 1) / 2, the strict
 * lower triangle of the exchangeabilities column by column (phylo_hip_geo.h's
 * order); the entries of freqs are independent variables.
 *
 * Included by phylo_hip.h, whose conventions hold unchanged: blens[b] is the
 * edge above node b, B = 2S-2 rooted (the last peel row's parent is 2S-2) and
 * 2S-3 unrooted (the (child1, 2S-3, 2S-2) last-row rule).
 *
 *   tipmasks[S][P]   uint64: bit j set when state j is compatible with the
 *                    tip's observation; all K bits for an unknown.  A mask with
 *                    no bit, or a bit >= K, is refused
 *   params[n][R + K + 2C]   rates, freqs, rs (category rates), ps (category
 *                    weights), per draw
 *
 * Contracts:
 *   - phy_kseq_create makes every refusal (PHY_EINVAL, the message names the
 *     argument and, for the peel, the row) before the first device call: on a
 *     machine without a device a bad argument yields its own message;
 *   - a draw without a likelihood (a frequency that is not positive, a negative
 *     or non-finite rate, rs, ps or branch length, an eigensolve that does not
 *     converge, L_i that is not positive and finite at a pattern of positive
 *     weight, a log L that is not finite) gives -inf followed by zeros and
 *     site_ll = -inf, with status 0; the other draws of the call are untouched;
 *   - partials are rescaled by powers of two per node, pattern and category:
 *     there is no taxon limit from the fp64 range;
 *   - a draw's row and site_ll are bitwise repeatable: they do not depend on
 *     n_draws, on the draw's position in the call, or on max_draws.
 *
 * All arithmetic is fp64.  The device holds 3 (2S-1) 16 ceil(K / 16) 16 doubles
 * per (category, 16-pattern tile) of a draw in flight; the draws in flight
 * follow from a fixed budget (1 GiB), and a shape whose single draw passes it is
 * refused.
 */
#ifndef PHYLO_HIP_KSEQ_H
#define PHYLO_HIP_KSEQ_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct phy_kseq_ctx phy_kseq_ctx;

/* max_draws: most draws one eval call may take. */
int phy_kseq_create(int S, int P, int K, int C, int rooted, const uint64_t* tipmasks, const double* weights,
                    const int32_t* peel, int max_draws, int device, phy_kseq_ctx** out);
int phy_kseq_destroy(phy_kseq_ctx* ctx);
int phy_kseq_num_branches(const phy_kseq_ctx* ctx); /* B; -1 for NULL */
int phy_kseq_row_len(const phy_kseq_ctx* ctx);      /* 1 + B + 2C + R + K; -1 for NULL */

/* Host buffers, synchronous: blens[n][B], params[n][R + K + 2C], rows[n][row_len],
 * site_ll[n][P] or NULL.  PHY_EINVAL: a NULL ctx or buffer; PHY_ERANGE: n_draws
 * outside 1..max_draws. */
int phy_kseq_eval(phy_kseq_ctx* ctx, int n_draws, const double* blens, const double* params, double* rows,
                  double* site_ll);

#ifdef __cplusplus
}
#endif

/* The same engine under a mixture of M models over sites (codon site models):
 * phy_kseq_mix_ctx and phy_kseq_mix_create / destroy / num_branches / row_len /
 * eval, with its plan and info calls. */
#include "phylo_hip_kseq_mix.h"

/* Its posterior summaries: the internal nodes' state posteriors and the
 * expected labelled substitution counts per branch, phy_kseq_sum_*. */
#include "phylo_hip_kseq_sum.h"

#endif /* PHYLO_HIP_KSEQ_H */
