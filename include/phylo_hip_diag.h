/*
 * phylo_hip_diag.h -- planning, tuning and introspection calls of the
 * MI355X pruning engine (libphylo_hip.so), beside the consumer boundary in
 * phylo_hip.h.  None of these has a reference counterpart: they expose the
 * launch plans (LDS chunks, column plans, class-sweep fusions, the sampler's
 * quad schedule), switch between engines and between bitwise-equal fused and
 * unfused forms (the tests' reference paths), and time the dominant kernel
 * (bench.py).  A Stan external function needs none of them.
 */
#ifndef PHYLO_HIP_DIAG_H
#define PHYLO_HIP_DIAG_H

#include "phylo_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Traversal-program facts: steps (= S-1), partial slots, deep-stack entries
 * (operands that wait while a sibling subtree runs), pattern blocks of the
 * current column plan. */
int phy_program_info(const phy_ctx* ctx, int* nsteps, int* nslots, int* depth, int* nblocks);

/* The traversal program of a tree and the batched (two-columns-per-lane)
 * sweep's step records for one plan, without a device: `program` receives
 * steps (= S-1) x 16 ints of raw indices after the chunk plan for LDS
 * chunks of at most `cap` matrices (x, y, mx, my, mv, vslot, flags, xslot,
 * yslot, xdpos, vdpos, chunk, m0, mn, node, rebuild depth; flags: 1 own
 * matrix, 2 x deep, 4 v deep, 8 not stored, 16 previous-step child rebuilt),
 * `records` the steps x 16 ints the kernel loads, every index already the
 * byte offset the kernel adds (x row, y row, LDS offsets of mx / my / mv in
 * the chunk, a_v's scratch offset, flags | depth << 8, the reverse's a_x and
 * a_y scratch offsets or 0x40000000 where it loads none, xdpos, vdpos, slot
 * offset of mx, m0, mn, slot offsets of my and mv).  `cols` columns per
 * lane and C categories give the scratch entry stride (cols * 2 * C * 1024
 * bytes), R the vectors per matrix record (R * 32 bytes).  Either output
 * may be NULL. */
int phy_plan_records(int S, const int32_t* peel, int rooted, int C, int R, int cols, int cap, int recompute,
                     int32_t* program, int32_t* records, int* nmat, int* n_chunks);

/* Clade compression of the batched sweep (default automatic).  A clade whose
 * tips take at most 128 distinct state tuples (classes) over the context's
 * patterns is run once per draw on one column per class instead of once per
 * pattern block: its steps (program L) run on a class block of tip states,
 * the rest of the tree (program U) on the pattern blocks with the clade root
 * a gathered leaf, and the root's upper partial is summed per class, in
 * ascending pattern order, before L's reverse.  Only maximal clades of at
 * least three internal nodes are taken, at most 8 sharing one class block.
 * mode: 0 off, 1 every qualifying clade, -1 automatic (a clade is kept when
 * the steps it saves outweigh its boundary: the cost model of DESIGN.md 5);
 * PHY_CLADE_COMPRESSION sets the default at phy_create.  A launch takes the
 * compressed plan only when it is one workgroup per draw of the two-column
 * sweep without rescaling; every other launch (the one-column and quad
 * sweeps, draws over several workgroups, the rescaled sweep, the class
 * sweep) runs what it ran without it.  With mode 0 every row is bit for bit
 * what it was; compressed rows agree with them to the rounding of the
 * reordered sums and are bitwise reproducible.  Same preconditions as
 * phy_set_engine; applies to every shard of a multi-device context.
 *
 * phy_clade_compression: the mode and the plan a compressed launch would
 * use (zeros when there is none).  facts[12]: clades, L steps, U steps, L
 * matrices, U matrices, aggregation rounds (the largest class size, rounded
 * up to 8), live columns of the class block, pattern blocks, scratch entries
 * per workgroup (one per step, then one r plane entry per clade and block),
 * deep-stack entries, LDS chunks, rebuilt partials.  clades[8][6]: root
 * node, internal nodes, classes, largest class, first and last L step.  Any
 * output may be NULL. */
int phy_set_clade_compression(phy_ctx* ctx, int mode);
int phy_clade_compression(const phy_ctx* ctx, int* mode, int* facts, int* clades);

/* The compressed plan of a tree and its tip data, without a device: facts
 * and clades as above (facts[0] = 0: nothing taken, the other outputs are
 * untouched); `program` the raw steps [L | U] after the chunk plan (as
 * phy_plan_records; a gathered child is x or y = -2 - clade, chunks never
 * straddle the L / U boundary) and `records` what the kernel loads (a
 * gathered child keeps that code, carries its root's scratch offset where an
 * internal child does and its r plane's scratch offset in the place
 * of a tip child's dL/dP slot offset); mat_branch[B] the branch of each
 * matrix, numbered in order of use over [L | U]; cls_of[clades][blocks * 128]
 * the class of every pattern column (-1 on padding); members[clades][rounds]
 * [128] the t-th pattern of class j in ascending order (-1 past its size);
 * rep[clades][128] the first pattern of class j, whose tip states the class
 * block holds.  tipcodes is [S][P] as phy_create takes it. */
int phy_clade_plan(int S, int P, int C, int rooted, const uint8_t* tipcodes, const int32_t* peel, int R, int cap,
                   int recompute, int mode, int* facts, int* clades, int32_t* program, int32_t* records,
                   int32_t* mat_branch, int32_t* cls_of, int32_t* members, int32_t* rep);

/* Everything the host plans for a context and one call of n_draws draws,
 * without a device: what phy_create on a device of `cu_count` compute units
 * followed by phy_set_tuning(wg_budget, cols, lds_budget),
 * phy_set_deep_stack(deep), phy_set_recompute(recompute),
 * phy_set_clade_compression(clade_mode) and phy_set_rescaling(rescaling)
 * would plan (the PHY_* environment preferences apply as at phy_create), and
 * what a phy_eval of n_draws draws would then launch on the pattern engine
 * (the class engine's choice needs its class plan and is not made here).
 * facts[PHY_PLAN_FACTS]:
 *    0 ..12  steps, partial slots, deep-stack entries, vectors per matrix
 *            record R; columns per lane, 1 for the one-column latency plan,
 *            pattern blocks, matrices per chunk, chunks, deep entries in LDS,
 *            rebuilt partials, resident workgroups, LDS bytes per workgroup
 *            (phy_program_info, phy_lds_plan and the getters beside them);
 *   13 ..16  PHY_PLAN_QUAD: 1 when the quad sweep's LDS plan fits, then
 *            phy_quad_plan's waves, span and slots;
 *   17 ..28  PHY_PLAN_CLADE: phy_clade_compression's facts[12];
 *   29 ..35  PHY_PLAN_LAUNCH: path (0 class, 1 one-wave quad, 2 multi-wave
 *            quad, 3 compressed pattern, 4 pattern sweep), sweep workgroups
 *            per draw, 1 when one workgroup runs a draw, 1 when the sweep
 *            finalizes the row itself, 1 when it also runs the Q-parameter
 *            chain rule, 1 when the finalize sums the per-workgroup dL/dP
 *            slots itself, 1 when the quad sweep builds its matrix records
 *            (eigensystems host-formed: calls of <= 32 draws). */
#define PHY_PLAN_QUAD 13
#define PHY_PLAN_CLADE 17
#define PHY_PLAN_LAUNCH 29
#define PHY_PLAN_FACTS 36
int phy_plan_sweep(int S, int P, int C, int rooted, const uint8_t* tipcodes, const int32_t* peel, int max_draws,
                   int cu_count, int wg_budget, int cols, int lds_budget, int deep, int recompute, int clade_mode,
                   int rescaling, int n_draws, int* facts);

/* The class plan (csrc/class_plan.h) phy_set_engine(ctx, 2) would build for
 * these inputs, without a device (the PHY_CLADE, PHY_CHAIN, PHY_ROOT_WGS,
 * PHY_STAGE_ORDER, PHY_PAIR, PHY_PAIR_MAX, PHY_REVFIX and PHY_ROOT_CHAIN
 * preferences of the environment apply as they do there; weights NULL: 1).
 * facts[PHY_CLASS_FACTS]:
 *    0 .. 6  phy_class_info: classes, levels, root classes, contributions,
 *            staged contributions, tiles, tile-crossing segments;
 *    7 .. 9  phy_class_clades: fused levels, clades, the largest's classes;
 *   10 ..12  phy_class_chain: chain levels, lowest chained level, top classes;
 *   13 ..15  phy_class_fused: level pairs, chunk spans, parent-order levels;
 *   16 ..24  dL/dP partial rows per category, staging positions, tiles, root
 *            workgroups per draw, rounds per root workgroup, pre-summed
 *            sub-ranges of long branches, chunk spans, the clade roots' RED
 *            tiles and long segments;
 *   25       1: the root recomputes the chain's top (0: PHY_ROOT_CHAIN=0).
 * digests[PHY_CLASS_TABLES]: the 64-bit FNV-1a hash of the bytes of every
 * table the engine uploads, in upload order: chain links, chain table, chain
 * representatives (the offset basis when there is no chain: not uploaded),
 * nodes, chunks, cls, secpos, stperm, tiles, spans, wroot, pat_root, gbase,
 * gcount, gsub, pbase, clade table, rtile, rspan, lfix, sspan, pair, clf,
 * clong, gc.  Either output may be NULL. */
#define PHY_CLASS_FACTS 26
#define PHY_CLASS_TABLES 25
int phy_plan_class(int S, int P, int C, int rooted, const uint8_t* tipcodes, const double* weights,
                   const int32_t* peel, long long* facts, unsigned long long* digests);

/* Measurement hooks (bench.py): while enabled, every phy_eval* records HIP
 * events around the sweep kernel on the stream it runs on;
 * phy_timing_read synchronises and returns the summed sweep-kernel time in
 * ms and the number of launches since phy_timing_start. */
int phy_timing_start(phy_ctx* ctx);
int phy_timing_read(phy_ctx* ctx, double* total_ms, int* launches);

/* Tuning: persistent workgroup budget per launch (0 = keep), columns per
 * lane `cols` (0 = automatic: 2 for C <= 8, else 1) and the LDS bytes one
 * workgroup may use (0 = keep; smaller budgets stage the P-matrix records
 * in more chunks).  The automatic LDS plan (no PHY_LDS_BUDGET, nothing set
 * here) takes the most workgroups per CU the kernel's register budget
 * allows whose LDS share still holds chunks of >= 24 matrices (or the whole
 * program).  The environment variables PHY_WG_BUDGET, PHY_COLS and
 * PHY_LDS_BUDGET set the defaults at phy_create. */
int phy_set_tuning(phy_ctx* ctx, int wg_budget, int cols, int lds_budget);

/* The LDS plan the next launch will use: chunks per pass, matrices per
 * chunk, LDS bytes per workgroup. */
int phy_lds_plan(const phy_ctx* ctx, int* n_chunks, int* matrices_per_chunk, int* lds_bytes);

/* Pattern columns each lane carries in the current plan (1 or 2). */
int phy_columns_per_lane(const phy_ctx* ctx);

/* Where the sweep keeps its deep stack (operands that wait while a sibling
 * subtree runs; phy_program_info's `depth` entries): 0 = automatic (all of
 * it in LDS when that leaves matrix chunks of >= 24 at the plan's
 * occupancy, else its outermost entries in LDS and the rest in the global
 * per-workgroup region), 1 = LDS, 2 = global.  Replans; PHY_DEEP sets the
 * default at phy_create.  phy_deep_stack_in_lds returns how many entries
 * the current plan holds in LDS. */
int phy_set_deep_stack(phy_ctx* ctx, int mode);
int phy_deep_stack_in_lds(const phy_ctx* ctx);

/* Recomputed cherries (default on; PHY_RECOMPUTE=0 at phy_create turns it
 * off): a node whose two children are tips, computed by the step just before
 * its parent's and in the same LDS chunk, is not written to scratch in the
 * forward half; the parent's reverse step rebuilds it from LDS.  Results are
 * identical either way (same operations in the same order).
 * phy_recomputed_partials: moved partials per column the current plan does
 * not store. */
int phy_set_recompute(phy_ctx* ctx, int on);
int phy_recomputed_partials(const phy_ctx* ctx);

/* Engine: 1 = pattern sweep (one lane per pattern column; a call of at most
 * 32 draws takes its quad form -- a quad of lanes per column, matrix records
 * built in the sweep when the eigensystems are host-formed, an epilogue split
 * over workgroups; PHY_QUAD=0 at phy_create keeps the column sweep), 2 = class sweep
 * (site repeats: the forward pass once per distinct tip-state tuple of each
 * subtree, the reverse on upper partials aggregated per tuple -- the exact,
 * total form of the reference's column-reuse cache, pruner/tree.cpp:140-174),
 * 0 = automatic (class sweep for alignments of >= 16384 patterns whose
 * subtree classes are at most a quarter of the pattern sweep's node-pattern
 * work).  Results agree to rounding either way.  PHY_ENGINE sets the default
 * at phy_create.  Mode 3 (round 3's resident class sweep) is retired and
 * refused with PHY_EINVAL: the quad sweep is faster for a sampler's calls on
 * every workload.  phy_engine returns the engine the next launch uses (0
 * pattern, 1 class). */
int phy_set_engine(phy_ctx* ctx, int mode);
int phy_engine(const phy_ctx* ctx);

/* Partial-likelihood rescaling (default off; with it off every row is bit for
 * bit what it was).  Without it the per-site likelihood of a tree of more
 * than roughly 400 taxa leaves the fp64 range: between about 400 and 500 taxa
 * sites turn subnormal and lose digits, past that every draw is -inf.  With
 * it on the pattern sweep renormalises every stored moved partial by the
 * power of two that brings its largest entry into [1, 2) (exact), keeps the
 * removed exponents in an int plane beside the moved-partial scratch
 * (allocated by the first phy_set_rescaling(ctx, 1); a context that never
 * switches it on pays nothing), adds them back at the root and folds them
 * into the upper partials of the reverse half, so the output rows and the
 * site log-likelihoods are the true values for any tree the context holds.
 * Only the pattern sweep has a rescaled form: while it is on the engine is
 * the pattern sweep (phy_engine reports 0), calls of <= 32 draws take the
 * column sweep instead of its quad form, and phy_set_engine(ctx, 2) is
 * refused with PHY_EINVAL; switching it off restores the engine preference's
 * choice.  phy_set_tuning, phy_set_deep_stack and phy_set_recompute work as
 * before.  Same preconditions as phy_set_engine (no submission in flight);
 * applies to every shard of a multi-device context.  phy_rescaling returns
 * 1 when it is on. */
int phy_set_rescaling(phy_ctx* ctx, int on);
int phy_rescaling(const phy_ctx* ctx);

/* Class-plan facts (zeros when no plan is built): non-root subtree classes
 * (the class sweep's forward work per category), levels (the root's level),
 * root classes (distinct site patterns by tip state), contributions (sum over
 * internal nodes of classes x internal children: the reverse's aggregation
 * inputs), the part of them staged through HBM (secondary children; a
 * primary child's are reduced in registers), reduction tiles and
 * tile-crossing segments. */
int phy_class_info(const phy_ctx* ctx, long long* classes, int* levels, int* root_classes, long long* stage,
                   long long* staged, int* tiles, int* spans);

/* Bottom clades of the class plan: the levels 1..fused_levels run as one
 * workgroup per clade (a maximal subtree of nodes at those levels) instead
 * of one launch per level and phase; clades, and the classes of the largest.
 * Chosen automatically (the deepest level whose largest clade has at most
 * 1024 classes); PHY_CLADE=k at phy_create fixes k levels (0: off).
 * Results are bitwise the same either way. */
int phy_class_clades(const phy_ctx* ctx, int* fused_levels, int* clades, long long* largest);

/* Top chain of the class plan: the run of single-node levels below the root
 * (caterpillar-like trees), fused into one forward and one reverse launch
 * (one lane per class of the top node, the classes below it from host
 * tables); chain levels (0: none), the lowest chained level and the top
 * node's classes.  Chosen when at least two such levels lie above the clade
 * levels (at most 8); PHY_CHAIN=0 at phy_create turns it off.  The forward
 * values are bitwise the level launches'; the dL/dP sums of the chained
 * branches run over the top classes, so they agree to rounding, not bits.
 */
int phy_class_chain(const phy_ctx* ctx, int* levels, int* lowest, int* top_classes);

/* Launch fusions and layouts of the class sweep's level launches, all
 * bitwise the unfused / default values (read at phy_create):
 *   level_pairs   forward level pairs -- adjacent levels (above the fused
 *                 clade levels, below the top chain) in one launch, the upper
 *                 level recomputing its children of the level below from
 *                 theirs.  PHY_PAIR=0: none; PHY_PAIR_MAX=n: only upper
 *                 levels of at most n classes (default: no cap).
 *   chunk_spans   long tile-crossing segments summed by the reverse chunk
 *                 of their class (the whole wave), so those levels have no
 *                 FIX launch.  PHY_REVFIX=0: none.
 *   parent_order_levels  levels whose secondary children's staging is
 *                 written in the parent's class order and gathered by the
 *                 RED tiles through a permutation (levels staging at least
 *                 100,000 classes; PHY_STAGE_ORDER=n sets that threshold,
 *                 0: every level above the clades). */
int phy_class_fused(const phy_ctx* ctx, int* level_pairs, int* chunk_spans, int* parent_order_levels);

/* The sampler's small-call sweep (calls of <= 32 draws, the quad sweep):
 * waves per category (0: the quad sweep does not apply to this context, 1:
 * the one-wave quad sweep, 2 up to 16 / C: the multi-wave form, whose host
 * list-schedule splits the post-order program over that many waves with LDS
 * hand-offs -- the most waves whose hand-off slots still fit LDS),
 * the schedule's length in program steps (the one-wave sweep: every step),
 * and its LDS hand-off slots.  PHY_QMW=0 at phy_create keeps the one-wave
 * form; the rows are bitwise the same either way. */
int phy_quad_plan(const phy_ctx* ctx, int* waves, int* span, int* slots);

/* The discrete-trait engine's plan (csrc/geo_plan.h): levels of internal
 * nodes, rows of the widest level, dynamic LDS bytes, workgroup size and the
 * grid cap (draws beyond it are looped over).  Any output may be NULL. */
int phy_geo_info(const phy_geo_ctx* ctx, int* levels, int* widest_level, int* lds_bytes, int* threads,
                 int* workgroups);
/* Jacobi sweeps each draw of the last phy_geo_eval took (the first n_draws of
 * them; -1: the draw was refused before the eigensolve). */
int phy_geo_sweeps(phy_geo_ctx* ctx, int n_draws, int* sweeps);
/* The tree-sample plan (csrc/geo_plan.h, geo_trees_plan): rows of the widest
 * level and the largest level count over the trees, the accumulation groups G
 * a draw's trees are split into (group g walks trees floor(g T / G) ..
 * floor((g + 1) T / G) - 1 in ascending order), workgroup size, dynamic LDS
 * bytes and the grid cap of the tree phase ((draw, group) items beyond it are
 * looped over).  Any output may be NULL. */
int phy_geo_trees_info(const phy_geo_trees_ctx* ctx, int* widest_level, int* max_levels, int* groups, int* threads,
                       int* lds_bytes, int* workgroups);
/* The forest's plan (csrc/forest_plan.h): columns per lane, matrices per LDS
 * chunk (common to all trees), the largest and smallest chunk count and deep
 * stack over the trees, the deep-stack entries kept in LDS, and the LDS
 * bytes per workgroup.  Any output may be NULL. */
int phy_forest_info(const phy_forest_ctx* ctx, int* cols, int* cap_m, int* max_chunks, int* min_chunks,
                    int* max_depth, int* min_depth, int* deep_in_lds, int* lds_bytes);
/* The same plan without a device or a context (phy_forest_create's arguments
 * and refusals, the PHY_* preferences of the environment, cu_count compute
 * units; 0: 256).  facts[12]: phy_forest_info's eight numbers, then whether
 * the one-column plan is the latency form, and whether the finalize / the
 * chain rule run inside the sweep / the chain rule inside the finalize kernel.
 * chunks[T], depths[T]: every tree's chunk count and deep stack.  Any output
 * may be NULL. */
int phy_forest_plan(int S, int P, int C, int rooted, int model, const uint8_t* tipcodes, const double* weights, int T,
                    const int32_t* peels, int max_rows, int cu_count, int* facts, int* chunks, int* depths);
/* The sequence-summary engine's plan (csrc/seqsum_plan.h) without a device or
 * a context: phy_seqsum_create's arguments and refusals.  facts[8]: the row
 * length, the padded pattern count, the workgroups per draw, the bytes of a
 * draw's partials workspace, the device bytes a draw in flight holds, the
 * draws per launch, the summary kernel's LDS bytes and the 4-vectors per
 * matrix record.  order[S-1]: the internal nodes in the forward pass's order
 * (the reverse pass walks it backwards).  Either output may be NULL. */
int phy_seqsum_plan(int S, int P, int C, int rooted, int model, const uint8_t* tipcodes, const double* weights,
                    const int32_t* peel, int max_draws, long long* facts, int32_t* order);
/* The partitioned engine's plan (csrc/part_plan.h) without a device or a
 * context: phy_part_create's arguments and refusals, the PHY_* preferences of
 * the environment, cu_count compute units (0: 256).  facts[PHY_PART_FACTS]:
 * columns per lane, whether the one-column plan is the latency form, the
 * blocks and the columns P of the padded alignment, its Ppad, the 4-vectors
 * per matrix record R, the low and high 32 bits of the extra tip masks (both
 * of the union of the partitions' tip masks), matrices per LDS chunk, chunks
 * per pass, deep-stack entries in LDS, whether that is the whole deep stack,
 * LDS bytes per workgroup, and whether the finalize / the chain rule run
 * inside the sweep / the chain rule inside the finalize kernel.
 * blocks[K][2]: every partition's block range [lo, hi).  col_part[P],
 * col_pat[P]: the partition and the pattern in it of every padded column
 * (-1, -1 between partitions); P = (the sum over k < K-1 of P_k rounded up
 * to 128) + P_{K-1}.  Any output may be NULL. */
#define PHY_PART_FACTS 16
int phy_part_plan(int S, int K, const int32_t* P_k, int C, int rooted, int model, const uint8_t* tipcodes,
                  const double* weights, const int32_t* peel, int max_draws, int cu_count, int* facts, int* blocks,
                  int* col_part, int* col_pat);
/* The plan a live context took (its device's compute units): phy_part_plan's
 * facts[PHY_PART_FACTS] and blocks[K][2].  Either output may be NULL. */
int phy_part_info(const phy_part_ctx* ctx, int* facts, int* blocks);

/* The K-state sequence engine's plan (csrc/kseq_plan.h) without a device or a
 * context: phy_kseq_create's arguments and refusals, for a device of cu_count
 * compute units.  facts[16]: padded states KT, pattern tiles, items per draw
 * (C * tiles), draws per chunk, item workgroup size, the item kernels' grid
 * cap, the per-draw kernels' grid cap, dynamic LDS bytes of the way up, of the
 * way down and of the per-draw kernels, doubles of an item's workspace, of a
 * slot and of a draw's record, the row length, B, bytes of workspace
 * allocated.  facts may be NULL. */
int phy_kseq_plan(int S, int P, int K, int C, int rooted, const uint64_t* tipmasks, const double* weights,
                  const int32_t* peel, int max_draws, int cu_count, long long* facts);
/* The live plan of a context (facts[16] as phy_kseq_plan) and the Jacobi sweeps
 * each of the first n draws of the last phy_kseq_eval took (-1: refused before
 * the eigensolve).  sweeps and facts may be NULL. */
int phy_kseq_info(const phy_kseq_ctx* ctx, int n, int32_t* sweeps, long long* facts);

#ifdef __cplusplus
}
#endif
#endif /* PHYLO_HIP_DIAG_H */
