/*
 * phylo_hip_seqsum.h -- posterior summaries of the sequence likelihood: what
 * the sequence at every internal node was, and how fast every site evolves.
 * One context holds one alignment and one tree; a call takes n parameter
 * points (posterior draws) and returns, per draw,
 *
 *   row[0]                 the log-likelihood
 *   anc[S-1][4][P]         the marginal state posterior of internal node
 *                          v = S .. 2S-2 (index v - S), states A, C, G, T, at
 *                          every pattern: sum_c ps_c part[v] q[v] / L_i with
 *                          part the forward and q the pre-order partials;
 *                          every (v, i) sums to one
 *   cat[C][P]              the rate-category posterior L_ci / L_i
 *   rate[P]                the posterior mean rate sum_c rs_c cat[c][i]
 *
 * or adds the draws' rows to a running sum kept on the device.
 *
 * Included by phylo_hip.h, whose conventions hold unchanged: blens[b] is the
 * edge above node b, B = 2S-2 rooted and 2S-3 unrooted (the (child1, 2S-3)
 * last-row rule), the model vector is PHY_MODEL_LEN(C) doubles.
 *
 * Contracts:
 *   - a draw whose log-likelihood is not finite (a NaN branch length, a
 *     negative frequency, L_i = 0 at a pattern) gives -inf followed by zeros
 *     from phy_seqsum_eval, with status 0; phy_seqsum_add reports -inf for it
 *     and leaves it out of the sum and of n_finite; the other draws of the
 *     call are untouched;
 *   - a draw's row is bitwise repeatable: its bits do not depend on n_draws,
 *     on its position in the call, or on the context's max_draws;
 *   - the sum is sequential in draw order: after phy_seqsum_reset, what
 *     phy_seqsum_read returns after any sequence of phy_seqsum_add calls is,
 *     bit for bit, the left-to-right fp64 sum (from +0) of the finite draws'
 *     phy_seqsum_eval rows, however the draws are split into calls or into
 *     launches inside a call;
 *   - the sums over categories (anc, L_i) run in category order.
 *
 * All arithmetic is fp64 without rescaling: the taxon limit is that of the
 * unrescaled engines (partials underflow past roughly 400 taxa; such draws
 * come back rejected).  The device holds 2 (S-1) C 4 Ppad doubles of partials
 * per draw in flight; the draws per launch follow from a fixed budget (1 GiB,
 * at least one draw), and PHY_ENOMEM is returned when the device cannot hold
 * one.
 */
#ifndef PHYLO_HIP_SEQSUM_H
#define PHYLO_HIP_SEQSUM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct phy_seqsum_ctx phy_seqsum_ctx;

/* phy_create's arguments and refusals (PHY_EINVAL), plus a row longer than
 * 2^31 - 1 doubles.  max_draws: most draws one eval / add call may take. */
int phy_seqsum_create(int S, int P, int C, int rooted, int model, const uint8_t* tipcodes, const double* weights,
                      const int32_t* peel, int max_draws, int device, phy_seqsum_ctx** out);
int phy_seqsum_destroy(phy_seqsum_ctx* ctx);
int phy_seqsum_num_branches(const phy_seqsum_ctx* ctx); /* B; -1 for NULL */
int phy_seqsum_row_len(const phy_seqsum_ctx* ctx);      /* 1 + (4(S-1) + C + 1) * P */

/* Host buffers, synchronous: blens[n][B], model[n][PHY_MODEL_LEN(C)],
 * rows[n][row_len].  PHY_ERANGE: n_draws outside 1..max_draws; PHY_EINVAL: a
 * NULL ctx or buffer. */
int phy_seqsum_eval(phy_seqsum_ctx* ctx, int n_draws, const double* blens, const double* model, double* rows);

/* The running sum over draws.  reset zeroes it and n_finite; add evaluates n
 * draws, adds the finite ones in draw order and returns their
 * log-likelihoods in loglik[n] (-inf for a rejected draw); read copies the
 * sums out (row[row_len]; n_finite may be NULL).  Codes as phy_seqsum_eval. */
int phy_seqsum_reset(phy_seqsum_ctx* ctx);
int phy_seqsum_add(phy_seqsum_ctx* ctx, int n_draws, const double* blens, const double* model, double* loglik);
int phy_seqsum_read(phy_seqsum_ctx* ctx, double* row, int* n_finite);

#ifdef __cplusplus
}
#endif
#endif /* PHYLO_HIP_SEQSUM_H */
