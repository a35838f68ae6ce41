"""The output-file contract of ``phylostan run`` / ``phylostan parse``.

* Sample CSV (what pystan writes to ``sample_file``): ``#`` comment lines, a
  header ``lp__,<sampler columns>,<params>,<transformed params>`` with Stan's
  ``name.k`` flattening, one row per draw.  NUTS adds the sampler columns
  ``accept_stat__,stepsize__,treedepth__,n_leapfrog__,divergent__,energy__``
  and the adaptation comment block; ADVI writes ``lp__ = 0`` rows, the first
  one being the mean of the approximation (Stan ``advi::run``).
* ``.diag`` (ADVI ``diagnostic_file``): ``iter,time_in_seconds,ELBO`` rows.
* ``.trees``: NEXUS written by ``convert_samples_to_nexus``
  (``phylostan/utils.py:193-287``), restated here on our tree objects;
  ``run --geo --ancestral`` writes its one annotated tree with
  ``write_geo_nexus`` and ``OUT.jumps.tsv`` with ``write_jumps_tsv``.
* ``parse_log`` (``utils.py:290-409``): mean / median / CI summaries printed
  after a run and by ``phylostan parse``.
"""
import re
import sys

import numpy as np

NUTS_COLUMNS = ["accept_stat__", "stepsize__", "treedepth__", "n_leapfrog__", "divergent__", "energy__"]
HMC_COLUMNS = ["accept_stat__", "stepsize__", "int_time__", "energy__"]  # diag_e_static_hmc


def _fmt(v):
    return "%.6g" % v


def write_nuts_csv(path, colnames, chain, rows, config, elapsed=None, save_warmup=False, algorithm="nuts"):
    """``rows``: [n_draws, len(colnames)] constrained values of the recorded
    draws of ``chain`` (a ``nuts.Chain`` or ``nuts.StaticHMCChain``), in the
    same order.  Static HMC writes Stan's HMC sampler columns."""
    hmc = algorithm == "hmc"
    with open(path, "w") as fp:
        for k, v in config:
            fp.write("# %s = %s\n" % (k, v))
        fp.write(",".join(["lp__"] + (HMC_COLUMNS if hmc else NUTS_COLUMNS) + colnames) + "\n")
        adapt_written = False
        for d, vals in zip(chain.draws, rows):
            q, lp, acc, eps, depth, nlf, div, energy, warm = d
            if warm and not save_warmup:
                continue
            if not warm and not adapt_written:
                fp.write("# Adaptation terminated\n# Step size = %g\n# Diagonal elements of inverse mass matrix:\n# %s\n"
                         % (chain.eps, ", ".join("%g" % x for x in chain.inv_metric)))
                adapt_written = True
            if hmc:  # the depth slot holds int_time
                sampler = [_fmt(lp), _fmt(acc), _fmt(eps), _fmt(depth), _fmt(energy)]
            else:
                sampler = [_fmt(lp), _fmt(acc), _fmt(eps), "%d" % depth, "%d" % nlf, "%d" % div, _fmt(energy)]
            fp.write(",".join(sampler + [_fmt(x) for x in vals]) + "\n")
        if elapsed is not None:
            w, s = elapsed
            fp.write("# \n#  Elapsed Time: %g seconds (Warm-up)\n#                %g seconds (Sampling)\n"
                     "#                %g seconds (Total)\n# \n" % (w, s, w + s))


def write_vb_csv(path, colnames, mean_row, draw_rows, config, eta):
    with open(path, "w") as fp:
        for k, v in config:
            fp.write("# %s = %s\n" % (k, v))
        fp.write(",".join(["lp__"] + colnames) + "\n")
        fp.write("# Stepsize adaptation complete.\n# eta = %g\n" % eta)
        fp.write(",".join(["0"] + [_fmt(x) for x in mean_row]) + "\n")
        for r in draw_rows:
            fp.write(",".join(["0"] + [_fmt(x) for x in r]) + "\n")


class DiagWriter:
    """ADVI diagnostic file: ``iter,time_in_seconds,ELBO``."""

    def __init__(self, path, config=()):
        self.fp = open(path, "w")
        for k, v in config:
            self.fp.write("# %s = %s\n" % (k, v))
        self.fp.write("iter,time_in_seconds,ELBO\n")

    def __call__(self, it, seconds, elbo):
        self.fp.write("%d,%.3f,%.6f\n" % (it, seconds, elbo))
        self.fp.flush()

    def close(self):
        self.fp.close()


# --------------------------------------------------------------------------
# utils.py:193-287
# --------------------------------------------------------------------------
def to_nexus(node, fp):
    if not node.is_leaf():
        fp.write("(")
        for i, n in enumerate(node.child_node_iter()):
            to_nexus(n, fp)
            if i == 0:
                fp.write(",")
        fp.write(")")
    else:
        fp.write(str(node.index))
    if hasattr(node, "date"):  # setup_dates gives every node a date (0.0 when isochronous)
        fp.write("[&height={}".format(node.date))
        if getattr(node, "rate", None) is not None:
            fp.write(",rate={}".format(node.rate))
        fp.write("]")
    if node.parent_node is not None:
        fp.write(":{}".format(node.edge_length))
    else:
        fp.write(";")


def convert_samples_to_nexus(tree, input, output, rate=None):
    S = len(tree.taxon_namespace)
    with open(output, "w") as outp:
        outp.write("#NEXUS\nBegin trees;\nTranslate\n")
        outp.write(",\n".join([str(i + 1) + " " + x.label.replace("'", "") for i, x in enumerate(tree.taxon_namespace)]))
        outp.write("\n;\n")
        header = None
        rows = []
        with open(input) as fp:
            for line in fp:
                if line.startswith("lp"):
                    header = line.strip().split(",")
                elif not line.startswith("#") and line.strip() and header is not None:
                    rows.append(line.strip().split(","))
        if header is None:
            raise ValueError("%s has no header line" % input)
        time_tree = "blens.1" not in header
        count = 1
        nodes = list(tree.postorder_node_iter())
        if time_tree:
            hindex = header.index("heights.1")
            strict = True
            rindex = None
            if rate is None:
                if "substrates.1" in header:
                    rindex = header.index("substrates.1")
                    strict = False
                else:
                    rindex = header.index("rate") if "rate" in header else None
            for l in rows:
                for n in nodes:
                    if not n.is_leaf():
                        n.date = float(l[hindex + n.index - S - 1])
                for n in nodes:
                    if n.parent_node is not None:
                        if strict:
                            n.rate = float(l[rindex]) if rate is None and rindex is not None else rate
                        else:
                            n.rate = float(l[rindex + n.index - 1])
                for n in nodes:
                    if n.parent_node is not None:
                        n.edge_length = n.parent_node.date - n.date
                outp.write("tree {} = ".format(count))
                count += 1
                to_nexus(tree.seed_node, outp)
                outp.write("\n")
        else:
            bindex = header.index("blens.1")
            for l in rows:
                for n in nodes:
                    if n.parent_node is not None:
                        k = bindex + n.index - 1
                        n.edge_length = float(l[k]) if k < len(l) else 0.0
                outp.write("tree {} = ".format(count))
                count += 1
                to_nexus(tree.seed_node, outp)
                outp.write("\n")
        outp.write("END;")


# --------------------------------------------------------------------------
# run --geo --ancestral (no counterpart in the reference: its geo run writes no tree)
# --------------------------------------------------------------------------
GEO_SET_MASS = 0.95  # location.set: the fewest states, most probable first, holding this much probability


def _geo_name(state):
    return '"' + re.sub(r'[\[\]";]', "_", str(state)) + '"'


def _geo_annotation(states, prob, jumps):
    order = np.argsort(-prob, kind="stable")
    k = int(np.searchsorted(np.cumsum(prob[order]), GEO_SET_MASS)) + 1
    keep = order[:min(k, len(order))]
    text = "[&location={},location.prob={!r},location.set={{{}}},location.set.prob={{{}}}".format(
        _geo_name(states[order[0]]), float(prob[order[0]]), ",".join(_geo_name(states[i]) for i in keep),
        ",".join(repr(float(prob[i])) for i in keep))
    if jumps is not None:
        text += ",jumps={!r}".format(float(jumps))
    return text + "]"


def write_geo_nexus(tree, output, states, marg, bjumps):
    """One NEXUS tree in the format of ``convert_samples_to_nexus``: the input
    topology and edge lengths, every node annotated with its modal location
    (``location``, ``location.prob``) and the smallest set of locations holding
    95% of its posterior probability (``location.set``, ``location.set.prob``),
    every edge with the expected number of transitions on it (``jumps``).
    ``marg [2S-1, K]`` and ``bjumps [2S-3]`` are indexed by node id (``index -
    1``): branch b is the edge above node b; the two root edges are one branch
    of the unrooted model, counted on the first root child's edge (where
    ``geo.tree_branch_lengths`` puts its length), so the second root child's
    edge carries ``jumps=0.0`` and that child the root's distribution."""
    marg = np.asarray(marg, float)
    nb = len(bjumps)

    def emit(node, fp):
        if not node.is_leaf():
            fp.write("(")
            for i, n in enumerate(node.child_node_iter()):
                emit(n, fp)
                if i == 0:
                    fp.write(",")
            fp.write(")")
        else:
            fp.write(str(node.index))
        b = node.index - 1
        top = node.parent_node is None
        fp.write(_geo_annotation(states, marg[b], None if top else (float(bjumps[b]) if b < nb else 0.0)))
        fp.write(";" if top else ":{}".format(node.edge_length))

    with open(output, "w") as outp:
        outp.write("#NEXUS\nBegin trees;\nTranslate\n")
        outp.write(",\n".join([str(i + 1) + " " + x.label.replace("'", "") for i, x in enumerate(tree.taxon_namespace)]))
        outp.write("\n;\ntree 1 = ")
        emit(tree.seed_node, outp)
        outp.write("\nEND;")


def write_subs_nexus(tree, output, blens, subs):
    """One NEXUS tree in ``write_geo_nexus``'s format (``run
    --ancestral_seq``): the input topology with the edge lengths ``blens [B]``
    (posterior means; branch b is the edge above node b = ``index - 1``), every
    internal node labelled with its id and every edge annotated with the
    expected number of substitutions on it, ``[&subs=...]``.  The second root
    child of an unrooted model has no branch of its own (B = 2S-3): its edge
    is written with length 0 and ``subs=0.0``."""
    nb = len(blens)

    def emit(node, fp):
        if not node.is_leaf():
            fp.write("(")
            for i, n in enumerate(node.child_node_iter()):
                emit(n, fp)
                if i == 0:
                    fp.write(",")
            fp.write(")")
        fp.write(str(node.index))
        if node.parent_node is None:
            fp.write(";")
            return
        b = node.index - 1
        fp.write("[&subs={!r}]:{!r}".format(float(subs[b]) if b < nb else 0.0, float(blens[b]) if b < nb else 0.0))

    with open(output, "w") as outp:
        outp.write("#NEXUS\nBegin trees;\nTranslate\n")
        outp.write(",\n".join([str(i + 1) + " " + x.label.replace("'", "") for i, x in enumerate(tree.taxon_namespace)]))
        outp.write("\n;\ntree 1 = ")
        emit(tree.seed_node, outp)
        outp.write("\nEND;")


def write_ancestral_fasta(output, S, anc, site_pattern):
    """One record per internal node, ``>node<id>`` with the 1-based node id
    (S+1 .. 2S-1): the modal state of ``anc [S-1, 4, P]`` at every alignment
    site (``site_pattern [sites]``: the pattern of every site)."""
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    with open(output, "w") as fp:
        for k in range(S - 1):
            seq = letters[np.argmax(anc[k], axis=0)][np.asarray(site_pattern)]
            fp.write(">node%d\n%s\n" % (S + k + 1, seq.tobytes().decode("ascii")))


def write_ancestral_tsv(output, S, anc):
    """``node, pattern, A, C, G, T``: every internal node's state
    probabilities at every pattern (node ids and patterns 1-based)."""
    P = anc.shape[2]
    with open(output, "w") as fp:
        fp.write("node\tpattern\tA\tC\tG\tT\n")
        for k in range(S - 1):
            for i in range(P):
                fp.write("%d\t%d\t%s\n" % (S + k + 1, i + 1, "\t".join(repr(float(v)) for v in anc[k, :, i])))


def write_codon_ancestral_fasta(output, S, anc, codon_pattern, codons):
    """``run --codon_ancestral``: one record per internal node, ``>node<id>`` (1-based, S+1 .. 2S-1): the three
    nucleotides of the modal codon of ``anc [S-1, 61, P]`` at every codon of the alignment (``codon_pattern
    [codons]``: the pattern of every codon; ``codons``: the 61 triplets)."""
    at = np.asarray(codon_pattern, np.int64)
    with open(output, "w") as fp:
        for k in range(S - 1):
            best = np.argmax(anc[k], axis=0)[at]
            fp.write(">node%d\n%s\n" % (S + k + 1, "".join(codons[j] for j in best)))


def write_codon_ancestral_tsv(output, S, anc, codon_pattern, codons, amino):
    """``node, codon_site, codon, amino_acid, probability``: every internal node's modal codon at every codon of
    the alignment, its amino acid and its posterior probability (node ids and codon sites 1-based)."""
    at = np.asarray(codon_pattern, np.int64)
    with open(output, "w") as fp:
        fp.write("node\tcodon_site\tcodon\tamino_acid\tprobability\n")
        for k in range(S - 1):
            best = np.argmax(anc[k], axis=0)
            for s, i in enumerate(at):
                j = int(best[i])
                fp.write("%d\t%d\t%s\t%s\t%.6g\n" % (S + k + 1, s + 1, codons[j], amino[j], float(anc[k, j, i])))


def write_codon_branches_tsv(output, syn, nonsyn, neutral_ratio):
    """``branch, S_mean, S_2.5%, S_97.5%, N_mean, N_2.5%, N_97.5%, dNdS``: the posterior mean and 95 % interval
    over the draws of the expected synonymous and nonsynonymous substitutions on every branch (``syn``,
    ``nonsyn`` ``[draws, B]``; branch b, 1-based, is the edge above node b), and dN/dS = (mean N / mean S) /
    ``neutral_ratio`` (the posterior mean of rho_N / rho_S), ``nan`` where mean S is 0."""
    syn, nonsyn = np.atleast_2d(syn), np.atleast_2d(nonsyn)
    with open(output, "w") as fp:
        fp.write("branch\tS_mean\tS_2.5%\tS_97.5%\tN_mean\tN_2.5%\tN_97.5%\tdNdS\n")
        for b in range(syn.shape[1]):
            ms, mn = float(syn[:, b].mean()), float(nonsyn[:, b].mean())
            ls, hs = np.percentile(syn[:, b], [2.5, 97.5])
            ln, hn = np.percentile(nonsyn[:, b], [2.5, 97.5])
            dnds = (mn / ms) / neutral_ratio if ms > 0 else float("nan")
            fp.write("%d\t%.6g\t%.6g\t%.6g\t%.6g\t%.6g\t%.6g\t%.6g\n" % (b + 1, ms, ls, hs, mn, ln, hn, dnds))


def write_codon_subs_nexus(tree, output, blens, syn, nonsyn):
    """``write_subs_nexus`` with every edge annotated ``[&S=...,N=...]``: the posterior mean expected synonymous
    and nonsynonymous substitutions on it (``syn``, ``nonsyn`` ``[B]``); an edge without a branch of its own has
    length 0 and both counts 0.0."""
    nb = len(blens)

    def emit(node, fp):
        if not node.is_leaf():
            fp.write("(")
            for i, n in enumerate(node.child_node_iter()):
                emit(n, fp)
                if i == 0:
                    fp.write(",")
            fp.write(")")
        fp.write(str(node.index))
        if node.parent_node is None:
            fp.write(";")
            return
        b = node.index - 1
        have = b < nb
        fp.write("[&S={!r},N={!r}]:{!r}".format(float(syn[b]) if have else 0.0, float(nonsyn[b]) if have else 0.0,
                                               float(blens[b]) if have else 0.0))

    with open(output, "w") as outp:
        outp.write("#NEXUS\nBegin trees;\nTranslate\n")
        outp.write(",\n".join([str(i + 1) + " " + x.label.replace("'", "") for i, x in enumerate(tree.taxon_namespace)]))
        outp.write("\n;\ntree 1 = ")
        emit(tree.seed_node, outp)
        outp.write("\nEND;")


def write_siterates_tsv(output, rate, cat, site_pattern):
    """``site, pattern, rate, p_cat1..p_catC``: every alignment site's
    posterior mean rate and rate-category probabilities (1-based)."""
    C = cat.shape[0]
    with open(output, "w") as fp:
        fp.write("\t".join(["site", "pattern", "rate"] + ["p_cat%d" % (c + 1) for c in range(C)]) + "\n")
        for s, i in enumerate(np.asarray(site_pattern)):
            fp.write("%d\t%d\t%s\n" % (s + 1, i + 1, "\t".join(repr(float(v)) for v in [rate[i]] + list(cat[:, i]))))


def write_jumps_tsv(output, states, migrations, times):
    """The K x K expected i -> j transitions (row i, column j; the diagonal
    blank) with a final ``time`` column, the expected time spent in i."""
    K = len(states)
    with open(output, "w") as fp:
        fp.write("\t".join(["from\\to"] + [str(x) for x in states] + ["time"]) + "\n")
        for i in range(K):
            cells = ["" if i == j else repr(float(migrations[i, j])) for j in range(K)]
            fp.write("\t".join([str(states[i])] + cells + [repr(float(times[i]))]) + "\n")


# --------------------------------------------------------------------------
# utils.py:290-409
# --------------------------------------------------------------------------
def descriptive_stats(d, alpha):
    median, low, high = np.quantile(d, (0.5, alpha / 2.0, 1.0 - alpha / 2.0))
    return np.mean(d), median, low, high


VARIABLES = {
    "wshape": "Weibull (shape)",
    "pinv": "Proportion invariant",
    "kappa": "HKY (kappa)",
    "rate": "Strict clock (rate)",
    "theta": "Constant population size (theta)",
    "tau": "GMRF precision (tau)",
    "netDiversificationRate": "net diversification rate",
    "relativeExtinctionRate": "relative extinction rate",
    "ucln_mean": "UCLN mean",
    "ucln_stdev": "UCLN stdev",
    "R": "effective reproductive number",
    "delta": "rate of becoming uninfectious",
    "s": "probability of an individual being sampled",
    "thetas": "effective population size",
    "heights": "coalescence times of nodes",
}


def read_samples(inputfile):
    header, rows = None, []
    with open(inputfile) as fp:
        for line in fp:
            line = line.strip()
            if line.startswith("lp"):
                header = line.split(",")
            elif not line.startswith("#") and len(line) != 0:
                rows.append([float(h) for h in line.split(",")])
    return header, np.array(rows).reshape(len(rows), len(header) if header else 0)


def parse_log(inputfile, alpha=0.05, tree=None, out=None):
    """Print the summaries of ``utils.parse_log``; returns them as a dict
    ``label -> (mean, median, low, high)``."""
    out = out or sys.stdout
    header, data = read_samples(inputfile)
    res = {}
    GTR = ("AC", "AG", "AT", "CG", "CT", "GC")
    freqs = ("A", "C", "G", "T")
    pct = (1 - alpha) * 100
    for var in header:
        if var == "rates.1":
            print("GTR", file=out)
            for i in range(6):
                m, md, lo, hi = descriptive_stats(data[:, header.index("rates." + str(i + 1))], alpha)
                res["rates.%d" % (i + 1)] = (m, md, lo, hi)
                print("  {} mean: {:.3E} {}% CI: ({:.3E},{:.3E})".format(GTR[i], m, pct, lo, hi), file=out)
            for i in range(4 if "freqs.1" in header else 0):  # a codon model's GTR rates come without freqs
                m, md, lo, hi = descriptive_stats(data[:, header.index("freqs." + str(i + 1))], alpha)
                res["freqs.%d" % (i + 1)] = (m, md, lo, hi)
                print("  {} mean: {:.4f} {}% CI: ({:.4f},{:.4f})".format(freqs[i], m, pct, lo, hi), file=out)
        elif var in VARIABLES:
            if "substrates.1" not in header or var != "rate":
                m, md, lo, hi = descriptive_stats(data[:, header.index(var)], alpha)
                res[var] = (m, md, lo, hi)
                print("{} mean: {} {}% CI: ({},{})".format(VARIABLES[var], m, pct, lo, hi), file=out)
    if "heights.1" in header:
        idx_root, max_h = 0, 0
        for idx, h in enumerate(header):
            if h.startswith("heights.") and data[0, idx] > max_h:
                idx_root, max_h = idx, data[0, idx]
        m, md, lo, hi = descriptive_stats(data[:, idx_root], alpha)
        res["root_height"] = (m, md, lo, hi)
        print("Root height mean: {} {}% CI: ({},{})".format(m, pct, lo, hi), file=out)
        if tree is not None and "substrates.1" in header:
            # relaxed clock (utils.py:354-380): per draw the mean rate
            # sum(rate * time) / sum(time) over the branches; the "variance"
            # is numpy.var of every branch rate seen in this and all earlier
            # draws (the reference's list is never reset between draws)
            rindex = header.index("substrates.1")
            hindex = header.index("heights.1")
            S = len(tree.taxon_namespace)
            nodes = list(tree.postorder_node_iter())
            mean_rates, variances, rates = [], [], []
            for i in range(data.shape[0]):
                for n in nodes:
                    if not n.is_leaf():
                        n.date = data[i, hindex + n.index - S - 1]
                    if n.parent_node is not None:
                        n.rate = data[i, rindex + n.index - 1]
                        rates.append(n.rate)
                dist = tm = 0.0
                for n in nodes:
                    if n.parent_node is not None:
                        el = n.parent_node.date - n.date
                        dist += n.rate * el
                        tm += el
                mean_rates.append(dist / tm)
                variances.append(np.var(rates))
            m, md, lo, hi = descriptive_stats(mean_rates, alpha)
            res["mean_rate"] = (m, md, lo, hi)
            print("Mean rate mean: {} {}% CI: ({},{})".format(m, pct, lo, hi), file=out)
            m, md, lo, hi = descriptive_stats(variances, alpha)
            res["variance_rate"] = (m, md, lo, hi)
            print("Variance rate mean: {} {}% CI: ({},{})".format(m, pct, lo, hi), file=out)
    else:
        idx = [k for k, h in enumerate(header) if h.startswith("blens")]
        sums = data[:, idx].sum(axis=1)
        m, md, lo, hi = descriptive_stats(sums, alpha)
        res["tree_length"] = (m, md, lo, hi)
        print("Tree length mean: {} {}% CI: ({},{})".format(m, pct, lo, hi), file=out)
    for var in ("R", "delta", "s", "thetas", "heights"):
        if "%s.1" % var in header:
            print(var, file=out)
            for k, h in enumerate(header):
                if h.startswith("%s." % var):
                    m, md, lo, hi = descriptive_stats(data[:, k], alpha)
                    print("  {} mean: {:.3E} {}% CI: ({:.3E},{:.3E})".format(h, m, pct, lo, hi), file=out)
    return res
