/*
 * phylo_hip_forest.h -- the forest boundary of the sequence likelihood: one
 * context holds the alignment once and T binary trees on its S tips, and one
 * call evaluates n rows, each naming its tree.  The workload it serves runs
 * the same model on every topology of a tree file (one ELBO per topology
 * approximates the topology posterior); with one phy_ctx per tree that is T
 * contexts and T latency-bound calls per iteration.
 *
 * Included by phylo_hip.h, whose conventions hold unchanged:
 *   - the tip ids of every peel refer to the one tipcodes row order;
 *   - blens[b] of a row is the edge above node b in THAT ROW'S tree;
 *   - unrooted trees follow the (child1, 2S-3) last-row rule, tree by tree;
 *   - the output row is phy_eval's compact row: 1 + B + 2C + 14 doubles
 *     (log-likelihood, dlogL/dblens, drs, dps, dfreqs (root), the six
 *     exchangeabilities, dfreqs (total)), without the dL/dP block;
 *   - a row whose log-likelihood is not finite (a negative frequency, a NaN
 *     branch length) returns -inf with status 0 and a zero gradient (its
 *     site_ll row is left as computed); the other rows are untouched.
 *
 * Contract: a row is bitwise repeatable.  Its bits do not depend on n_rows,
 * on the row's position in the call, or on which other rows or trees the call
 * or the context holds beyond what fixes the context's plan (the sizes, the
 * data, max_rows, the deepest tree's stack, the PHY_* preferences at create):
 * the kernel form is the context's, never a call's.
 *
 * Not in the forest form (use a phy_ctx per tree): the rescaled sweep, the
 * class sweep, clade compression, the quad sweeps, multi-device handles,
 * device-buffer and asynchronous evaluation.
 */
#ifndef PHYLO_HIP_FOREST_H
#define PHYLO_HIP_FOREST_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct phy_forest_ctx phy_forest_ctx;

/* peels[T][(S-1)*3]: one peel per tree, phy_create's form.  max_rows: most
 * rows one phy_forest_eval may take.  PHY_EINVAL: T < 1, trees whose device
 * tables pass 256 MiB, a malformed tree (the message names its index) and
 * everything phy_create refuses. */
int phy_forest_create(int S, int P, int C, int rooted, int model, const uint8_t* tipcodes, const double* weights,
                      int T, const int32_t* peels, int max_rows, int device, phy_forest_ctx** out);
int phy_forest_destroy(phy_forest_ctx* ctx);
int phy_forest_num_trees(const phy_forest_ctx* ctx);    /* T; -1 for NULL */
int phy_forest_num_branches(const phy_forest_ctx* ctx); /* B */
int phy_forest_output_len(const phy_forest_ctx* ctx);   /* 1 + B + 2C + 14 */

/* n_rows rows, host buffers, synchronous: tree_of_row[n], blens[n][B],
 * model[n][PHY_MODEL_LEN(C)], out[n][phy_forest_output_len()], site_ll[n][P]
 * or NULL.  PHY_ERANGE: n_rows outside 1..max_rows, a tree_of_row entry
 * outside 0..T-1 (the message names the row); PHY_EINVAL: a NULL ctx,
 * tree_of_row, blens, model or out. */
int phy_forest_eval(phy_forest_ctx* ctx, int n_rows, const int32_t* tree_of_row, const double* blens,
                    const double* model, double* out, double* site_ll);

#ifdef __cplusplus
}
#endif
#endif /* PHYLO_HIP_FOREST_H */
