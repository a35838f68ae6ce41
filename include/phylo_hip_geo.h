/*
 * phylo_hip_geo.h -- C-ABI of the K-state discrete-trait ("phylogeography")
 * likelihood engine of libphylo_hip.so.  Part of the consumer boundary:
 * phylo_hip.h includes it, and its conventions (return codes,
 * phy_last_error, -inf with status 0, node ids, the unrooted peel) are the
 * ones stated there.
 */
#ifndef PHYLO_HIP_GEO_H
#define PHYLO_HIP_GEO_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------
 * Phylogeography: the K-state discrete-trait likelihood on a fixed tree
 * (the reference's --geo model, generate_script.py:1102-1165).
 *
 * One site of K = STATES locations, S tips, the unrooted convention above:
 * peel[(S-1)*3] with the last row (child1, 2S-3, 2S-2), B = 2S-3 branch
 * lengths, the merged root branch being the sum of the two root-child edges
 * (phylostan.py:245-247 means this; as shipped it adds to the wrong slot).
 *   Params per draw, length R + K, R = K(K-1)/2:
 *     [0 .. R)     rates_geo, the strict lower triangle of the symmetric R
 *                  column by column: for col in 1:(K-1), for row in
 *                  (col+1):K   (generate_script.py:913-920)
 *     [R .. R+K)   freqs_geo (pi)
 *   Row per draw, length phy_geo_output_len() = 1 + B + R + K:
 *     [0]              log L = log(sum(root partial))  (generate_script.py:1096,
 *                      unknown_root_frequencies=True, the only form emitted)
 *     [1 .. 1+B)       dlogL/dblens
 *     [1+B .. 1+B+R)   dlogL/drates_geo
 *     [1+B+R .. +K)    dlogL/dfreqs_geo, the K entries taken as independent
 *                      (through Q, its normalisation and the D^{+-1/2} factors
 *                      of P; the simplex transform is the caller's)
 * A draw whose likelihood is not finite (a non-positive frequency, an
 * eigensolve that does not converge, L = 0) gives -inf and a zero gradient
 * with status 0.  Partials are rescaled by exact powers of two after every
 * internal node, always: the reference's --rescaling_geo (:1065-1084) has
 * nothing left to switch.
 * ------------------------------------------------------------------------- */
typedef struct phy_geo_ctx phy_geo_ctx;

/* Copies the tip partials and the level schedule of the tree to the device
 * and allocates every work buffer.  tip_partials[S*K] in [0, 1]: one-hot for
 * a known location, all ones for a missing one (the data block's geodata,
 * generate_script.py:1112-1116; phylostan.py:233-237).  Replaces the Stan
 * data of phylostan.py:249-253.  PHY_EINVAL: K outside 2..64, S < 3, a
 * malformed peel, a partial outside [0, 1]. */
int phy_geo_create(int S, int K, const double* tip_partials, const int32_t* peel, int max_draws, int device,
                   phy_geo_ctx** out);
int phy_geo_destroy(phy_geo_ctx* ctx);
/* B = 2S-3 (transformed data bcount, generate_script.py:1121). */
int phy_geo_num_branches(const phy_geo_ctx* ctx);
/* 1 + B + R + K. */
int phy_geo_output_len(const phy_geo_ctx* ctx);
/* Log-likelihood and gradient of n_draws <= max_draws parameter points, host
 * buffers, synchronous: blens[n*B], params[n*(R+K)], out[n*(1+B+R+K)].
 * Replaces calculate_p_matrices (generate_script.py:895-950), the pruning loop
 * (:1085-1096) and Stan's reverse sweep through both.  PHY_ERANGE: n_draws
 * outside 1..max_draws. */
int phy_geo_eval(phy_geo_ctx* ctx, int n_draws, const double* blens, const double* params, double* out);

/* ---------------------------------------------------------------------------
 * Posterior summaries: where the ancestors were, how often lineages moved and
 * on which branches, per draw, from what the gradient pass leaves on the
 * device.  The reference has no counterpart (its --geo run stops at the
 * posterior of rates_geo and freqs_geo).
 *   Summary row per draw, length phy_geo_summary_len() = N K + K K + B,
 *   N = 2S-1 nodes, B = 2S-3 branches:
 *     [0 .. N K)            marg[n][i]: the posterior probability that node n
 *                           is in state i, (lower partial of n)_i *
 *                           dlogL/d(lower partial of n)_i.  Every row sums to
 *                           1.  Tips are included: a known tip is one-hot, a
 *                           missing one (all-ones partial) gets its imputed
 *                           distribution.  Node 2S-3, the merged root child,
 *                           has no branch of its own: it is the root of the
 *                           unrooted tree, and its row repeats row 2S-2.
 *     [N K .. N K + K K)    jumps[i][j], row-major.  i != j: the expected
 *                           number of i -> j transitions over the whole tree
 *                           given the tip data, A_ij G_ij with A = D^1/2 Q
 *                           D^-1/2 and G = dlogL/dA entry by entry (Minin &
 *                           Suchard 2008); not symmetric.  i == j: the
 *                           expected time spent in i, G_ii, in the units of
 *                           blens; the K of them sum to sum(blens).
 *     [N K + K K .. +B)     bjumps[b]: the expected number of transitions of
 *                           any kind on branch b (the edge above node b; the
 *                           merged root branch is child1's); their sum is the
 *                           sum of the off-diagonal jumps.
 * A draw whose likelihood is not finite (its out row is -inf and zeros) has
 * an all-zero summary row; the other draws of the call are not touched by it.
 * Rows are bitwise repeatable and do not depend on the batch a draw is in.
 * ------------------------------------------------------------------------- */
/* N K + K K + B; -1 for NULL. */
int phy_geo_summary_len(const phy_geo_ctx* ctx);
/* phy_geo_eval and the summaries of the same draws in one launch: out[n*(1+B+
 * R+K)] receives phy_geo_eval's rows bit for bit and may be NULL,
 * summaries[n*summary_len] the rows above.  The device buffer of the summaries
 * is allocated by the first call: a context that never asks holds no more
 * memory than before.  PHY_ERANGE: n_draws outside 1..max_draws; PHY_EINVAL: a
 * NULL ctx, blens, params or summaries. */
int phy_geo_eval_summaries(phy_geo_ctx* ctx, int n_draws, const double* blens, const double* params, double* out,
                           double* summaries);

/* ---------------------------------------------------------------------------
 * A sample of trees: the mixture likelihood over T trees on the same S tips
 * (an "empirical tree distribution": the posterior sample of a tree
 * inference, any mix of topologies).  The reference has no counterpart: its
 * --geo model conditions on one tree.
 *     L_mix(theta) = sum_t w_t L_t(theta),        w_t = exp(log_weights[t])
 *     grad log L_mix = sum_t p_t grad log L_t,    p_t = w_t L_t / L_mix
 * p_t is the posterior probability of tree t.  Each tree is a peel in the
 * unrooted convention above with its own B = 2S-3 branch lengths; these are
 * data of the context, so a row carries no d/dblens.  One eigensolve per draw
 * serves all T trees; the trees of a draw run on separate workgroups.
 *   Params per draw: as phy_geo_eval, length R + K.
 *   Row per draw, length phy_geo_trees_output_len() = 1 + R + K:
 *     [0]            log L_mix
 *     [1 .. 1+R)     dlogL_mix/drates_geo
 *     [1+R .. +K)    dlogL_mix/dfreqs_geo, the K entries taken as independent
 *   tree_ll[n][T]: log L_t of every tree and draw (without log w_t), so that
 *     p_t = exp(tree_ll[t] + log_weights[t] - row[0]).
 *   Summary row per draw, length phy_geo_trees_summary_len() = K K + K: the
 *   p_t-weighted means of what does not depend on a topology,
 *     [0 .. K K)     jumps[i][j] as in phy_geo_eval_summaries (i != j: expected
 *                    i -> j transitions; i == j: expected time in i)
 *     [K K .. +K)    root[i]: the posterior probability that the root (of the
 *                    unrooted tree: the merged root child) is in state i.
 * Partials are rescaled by powers of two after every internal node, always,
 * and the trees' terms are summed against a running maximum of log w_t + log
 * L_t, so L_mix itself may lie far outside the fp64 range.  A tree whose
 * likelihood is 0 or not finite has weight 0 and tree_ll = -inf for that entry
 * alone.  A draw with bad parameters, a non-converged eigensolve, or no tree
 * with a finite likelihood gives -inf, a zero gradient, tree_ll all -inf and a
 * zero summary row with status 0; the other draws are not touched by it.  Rows
 * are bitwise repeatable and do not depend on the batch a draw is in: how the
 * trees are grouped and summed is fixed by the context.
 * ------------------------------------------------------------------------- */
typedef struct phy_geo_trees_ctx phy_geo_trees_ctx;

/* tip_partials[S*K] as phy_geo_create; peels[T][(S-1)*3], blens[T][B];
 * log_weights[T], used as given (not renormalised), or NULL for -log T each.
 * PHY_EINVAL: what phy_geo_create refuses, for any tree (the message names the
 * tree's index); T < 1; a NULL peels or blens; a NaN or infinite log weight; a
 * branch length that is not finite; a sample whose schedules and branch
 * lengths pass 256 MiB on the device. */
int phy_geo_trees_create(int S, int K, const double* tip_partials, int T, const int32_t* peels, const double* blens,
                         const double* log_weights, int max_draws, int device, phy_geo_trees_ctx** out);
int phy_geo_trees_destroy(phy_geo_trees_ctx* ctx);
/* T; -1 for NULL. */
int phy_geo_trees_num_trees(const phy_geo_trees_ctx* ctx);
/* 1 + R + K; -1 for NULL. */
int phy_geo_trees_output_len(const phy_geo_trees_ctx* ctx);
/* K K + K; -1 for NULL. */
int phy_geo_trees_summary_len(const phy_geo_trees_ctx* ctx);
/* n_draws <= max_draws parameter points, host buffers, synchronous:
 * params[n*(R+K)], out[n*(1+R+K)], tree_ll[n*T] or NULL.  PHY_ERANGE: n_draws
 * outside 1..max_draws; PHY_EINVAL: a NULL ctx, params or out. */
int phy_geo_trees_eval(phy_geo_trees_ctx* ctx, int n_draws, const double* params, double* out, double* tree_ll);
/* The same rows, bit for bit (out and tree_ll may be NULL), and the summary
 * rows summaries[n*(K K + K)].  The device buffer of the summaries is
 * allocated by the first call. */
int phy_geo_trees_eval_summaries(phy_geo_trees_ctx* ctx, int n_draws, const double* params, double* out,
                                 double* tree_ll, double* summaries);

/* ---------------------------------------------------------------------------
 * A trait clock rate.  Q is normalised to one expected transition per unit of
 * branch length, so the calls above read a branch length as an expected number
 * of migrations.  On a time-scaled tree (years, days, substitutions per site)
 * the process needs a rate of its own: mu > 0, the expected number of
 * migrations per lineage per unit of the tree's time at stationarity,
 *     P_b = exp(Q mu t_b).
 * The tree sample's branch lengths live on the device, so mu enters there:
 * clock[n] holds one mu per draw, and every effective length mu * t_tb is one
 * fp64 product formed before anything else uses it (a context on blens at mu
 * gives the bits of a context on the products mu * blens).
 *   Row per draw, length phy_geo_trees_clock_output_len() = 2 + R + K:
 *     [0 .. 1+R+K)   as phy_geo_trees_eval's row, at the effective lengths
 *     [1+R+K]        dlogL_mix/dmu = sum_t p_t sum_b t_tb dlogL_t/dt_eff,b,
 *                    formed as (1/mu) sum_k lam_k Wbar_kk from the draw's
 *                    eigenvalues and the p_t-weighted W of the gradient pass
 *   tree_ll as above.  Summary row, length K K + K as above: jumps[i][j], i !=
 *   j, and root[i] keep their meaning; jumps[i][i] is the expected time in i in
 *   the tree's own unit, G_ii / mu, and the K of them sum to sum_t p_t
 *   length_t.
 * A draw whose mu is not finite or not > 0 behaves like a draw with a bad
 * frequency: -inf, a zero gradient, tree_ll all -inf, a zero summary row,
 * status 0, the other draws untouched.  Everything said above about fixed
 * summation order and bitwise independence of the batch holds, with a
 * different mu per draw.  The calls without a clock run the code they ran
 * before; the buffers of the clock calls are allocated by the first of them.
 *
 * A single tree needs no call of its own, because phy_geo_eval takes blens per
 * draw: pass mu * blens; multiply the returned dlogL/dblens by mu to have the
 * derivative with respect to the tree's lengths; dlogL/dmu = sum_b t_b *
 * (the returned dlogL/dblens_b before that multiplication).  The dwell times
 * jumps[i][i] of phy_geo_eval_summaries divided by mu are in the tree's unit.
 * ------------------------------------------------------------------------- */
/* 2 + R + K; -1 for NULL. */
int phy_geo_trees_clock_output_len(const phy_geo_trees_ctx* ctx);
/* params[n*(R+K)], clock[n], out[n*(2+R+K)], tree_ll[n*T] or NULL.
 * PHY_ERANGE: n_draws outside 1..max_draws; PHY_EINVAL: a NULL ctx, params,
 * clock or out. */
int phy_geo_trees_eval_clock(phy_geo_trees_ctx* ctx, int n_draws, const double* params, const double* clock,
                             double* out, double* tree_ll);
/* The same rows, bit for bit (out and tree_ll may be NULL), and the summary
 * rows summaries[n*(K K + K)], dwell times in the tree's unit.  PHY_EINVAL: a
 * NULL ctx, params, clock or summaries. */
int phy_geo_trees_eval_clock_summaries(phy_geo_trees_ctx* ctx, int n_draws, const double* params,
                                       const double* clock, double* out, double* tree_ll, double* summaries);

#ifdef __cplusplus
}
#endif
#endif /* PHYLO_HIP_GEO_H */
