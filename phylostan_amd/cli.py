"""``phylostan`` command line with the Stan runtime removed.

Same sub-commands, flags and output files as ``phylostan/phylostan.py``
(``build`` ``:149-161``, ``run`` ``:164-335``, ``parse`` ``:130-146``), driven
by the GPU likelihood engine instead of pystan:

* ``build -s SCRIPT ...`` writes SCRIPT as a JSON model description (the
  options that shape the model and the Stan parameter names it implies) in
  place of the emitted Stan program.  ``--compile`` "compiles" it: the HIP
  engine is loaded and the compiled-model artifact is written under the
  reference's name, SCRIPT with ``.stan`` replaced by ``.pkl`` (or SCRIPT +
  ``.pkl``; phylostan.py:154-161).  The artifact is JSON, never a pickle:
  the model options, the engine library and its kernel-source hash.
* ``run`` follows phylostan.py:292-300: if the artifact is missing or
  ``--compile`` is given it is (re)built, otherwise the existing one is
  loaded and its model is used -- a run whose flags describe a different
  model than the artifact is refused (the reference would hand Stan a data
  dict that does not fit the compiled model).
* ``run -s SCRIPT -t TREE -i ALN -o OUT ...`` reads and indexes the data
  exactly as the reference (``phylostan_amd.data.load``), builds the host
  posterior around ``TreeLikelihood`` and runs ``-a vb`` (ADVI,
  (``-q meanfield``, the default, or ``-q fullrank``), ``-a nuts`` or
  ``-a hmc`` (static HMC); it writes OUT (Stan-format sample CSV; ``OUT_{chain}.csv``
  for several chains, as pystan), ``OUT.diag`` (vb), ``OUT.trees`` and prints
  the ``parse_log`` summary.
* ``run ... --ancestral_seq`` evaluates the recorded posterior draws once more
  (``sequence_summaries``) and writes ``OUT.ancestral.fasta``,
  ``OUT.ancestral.tsv``, ``OUT.siterates.tsv`` and ``OUT.ancestral.trees``:
  the internal nodes' sequences, the sites' rates and the expected
  substitutions per branch.
* ``run --codon --codon_sites M1a|M2a|M3:k`` lets omega vary over sites
  (``codon.CodonSitesPosterior`` on the K-state mixture likelihood); after
  sampling it evaluates the recorded draws once more with the class
  posteriors and writes ``OUT.codon_sites.tsv``, one line per codon.
* ``run --codon --codon_ancestral`` evaluates the recorded draws once more on
  the K-state summaries (``codon_summaries``) and writes
  ``OUT.ancestral.fasta``, ``OUT.ancestral.tsv``, ``OUT.codon_branches.tsv``
  and ``OUT.ancestral.trees``: the internal nodes' codons and the expected
  synonymous and nonsynonymous substitutions (dN / dS) per branch.
* ``run --geo -M META -t TREE -s SCRIPT -o OUT`` is phylogeography
  (``run_geo``): the K-state discrete-trait model of the locations in META on
  TREE's own branch lengths, no alignment; it writes OUT (``lp__, rates_geo.*,
  freqs_geo.*``), ``OUT.diag`` (vb) and the summary, and no ``.trees`` file;
  with ``--ancestral`` it evaluates the posterior draws once more and writes
  ``OUT.trees`` (one tree, every node's location and every branch's expected
  migrations) and ``OUT.jumps.tsv``.
* ``parse --samples CSV -t TREE -o OUT.trees`` post-processes a sample file.

Run as ``python -m phylostan_amd <command> ...``.
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

from . import data as dataio
from . import stan_io
from .posterior import ModelSpec, Posterior, TreeData


def create_parse_parser(sub):
    p = sub.add_parser("parse", help="parse Stan log files")
    p.add_argument("--samples", required=True, help="Path to sample file from Stan")
    p.add_argument("-t", "--tree", required=True, help="Tree file")
    p.add_argument("-o", "--output", required=True, help="Nexus output file")
    p.add_argument("--alpha", type=float, default=0.05,
                   help="Controls level for 100*(1-alpha)%% Bayesian credible intervals")
    p.add_argument("--rate", type=float, help="Value of fixed rate")
    p.add_argument("--dates", help="Comma-separated (csv) file containing sequence dates with header 'name,date'")
    p.add_argument("--heterochronous", action="store_true",
                   help="Heterochronous data. Expect a date in the leaf names or a csv file containing dates")
    return p


def create_build_parser(sub, prog, help):
    p = sub.add_parser(prog, help=help)
    p.add_argument("-s", "--script", required=True, help="Model script file")
    p.add_argument("-m", "--model", choices=["JC69", "HKY", "GTR"], default="GTR",
                   help="Substitution model [default: %(default)s]")
    p.add_argument("-I", "--invariant", action="store_true", help="Include a proportion of invariant sites")
    p.add_argument("-C", "--categories", metavar="C", type=int, default=1, help="Number of categories")
    p.add_argument("--heterogeneity", choices=["weibull", "discrete"], default="weibull",
                   help="Weibull or discrete distribution to model rate heterogeneity across sites")
    p.add_argument("--heterochronous", action="store_true", help="Heterochronous data. Expect a date in the leaf names")
    p.add_argument("--clock", choices=["strict", "ace", "acln", "acg", "aoup", "ucln", "uced", "gmrf", "hsmrf"],
                   default=None, help="Type of clock")
    p.add_argument("--estimate_rate", action="store_true", help="Estimate substitution rate")
    p.add_argument("-c", "--coalescent", choices=["constant", "skyride", "skygrid"], default=None,
                   help="Type of coalescent (constant or skyride)")
    p.add_argument("--speciation", choices=["bd", "yule"], default=None, help="Speciation model")
    p.add_argument("--grid", metavar="I", type=int, help="Number of grid points in skygrid")
    p.add_argument("--cutoff", metavar="G", type=float, help="a cutoff for skygrid")
    p.add_argument("--compile", action="store_true", help="Check that the GPU engine loads")
    p.add_argument("--geo", action="store_true",
                   help="Phylogeography: discrete-trait model of the sampling locations on the fixed tree (run: with -M)")
    p.add_argument("--rescaling_geo", action="store_true",
                   help="Phylogeography: accepted and changes nothing -- the engine always rescales its partials")
    p.add_argument("--geo_clock", action="store_true",
                   help="Phylogeography (--geo): estimate the trait clock rate (migrations per lineage per unit of the "
                        "tree's time), for trees whose branch lengths are times; sample column rate_geo")
    p.add_argument("--geo_rate", type=float, metavar="X", help="Phylogeography (--geo): fix the trait clock rate at X")
    p.add_argument("--geo_clock_prior", metavar="SHAPE,RATE",
                   help="--geo_clock: the Gamma prior of the rate [default: 0.5 and the (mean) tree length]")
    p.add_argument("--codon", action="store_true",
                   help="Codon model (GY94 / MG94 style): the alignment is read as triplets of the universal genetic "
                        "code (61 sense codons) with one dN/dS ratio omega ~ lognormal(-1, 1.25); -m gives the "
                        "nucleotide exchangeabilities (HKY: kappa, GTR: rates, JC69: all 1). Q is normalised to one "
                        "expected substitution per codon per unit of branch length. Sample column omega; run writes "
                        "OUT.codon.tsv (omega, kappa or rates, the 61 codon frequencies). Runs on the device's K-state "
                        "sequence engine (kseq.DeviceKStateLikelihood, DESIGN.md 5j)")
    p.add_argument("--codon_freqs", choices=["F3x4", "F1x4", "F61"], default="F3x4",
                   help="--codon: codon frequencies from three position-specific nucleotide simplexes freqs_pos1..3 "
                        "(F3x4), one simplex freqs (F1x4), or fixed at the observed codon counts plus one each (F61) "
                        "[default: %(default)s]")
    p.add_argument("--codon_sites", metavar="M1a|M2a|M3:k",
                   help="--codon: omega varies over sites as a mixture of classes with proportions pclass ~ "
                        "dirichlet(1). M1a: omega0 in (0, 1) and omega1 = 1; M2a: M1a and omega2 > 1 (omega2 - 1 ~ "
                        "exponential(1)); M3:k, k in 2..4: k free ordered omegas. Q is normalised so that the mean "
                        "rate over the classes is one substitution per codon. Sample columns omega.m (free omegas) "
                        "and pclass.m; run writes OUT.codon_sites.tsv: per codon of the alignment the posterior "
                        "class probabilities, the posterior mean omega and P(omega > 1). Runs on the K-state mixture "
                        "engine (kseq.DeviceKStateMixLikelihood, DESIGN.md 5j)")
    return p


def create_run_parser(sub):
    p = create_build_parser(sub, "run", help="run an analysis")
    p.add_argument("-t", "--tree", required=True, help="Tree file")
    p.add_argument("-i", "--input", required=False, help="Sequence file")
    p.add_argument("-o", "--output", required=True, help="Stem for output files")
    p.add_argument("--lower_root", type=float, default=0.0, help="Lower bound of the root")
    p.add_argument("--rate", type=float, help="Substitution rate")
    p.add_argument("--dates", help="Comma-separated (csv) file containing sequence dates with header 'name,date'")
    p.add_argument("-a", "--algorithm", choices=["vb", "nuts", "hmc"], default="vb", type=str.lower,
                   help="Algorithm [default: %(default)s]")
    p.add_argument("-S", "--seed", type=int, help="Seed")
    p.add_argument("-q", "--variational", choices=["meanfield", "fullrank"], default="meanfield",
                   help="Variational distribution family")
    p.add_argument("-e", "--eta", type=float, help="eta (variational only)")
    p.add_argument("--elbo_samples", type=int, default=100, help="Monte Carlo draws per ELBO estimate")
    p.add_argument("--grad_samples", type=int, default=1, help="Monte Carlo draws per ELBO gradient")
    p.add_argument("--samples", type=int, default=1000, help="Draws from the variational distribution")
    p.add_argument("--tol_rel_obj", type=float, default=0.001, help="Relative ELBO convergence tolerance")
    p.add_argument("--chains", type=int, default=1, help="Number of chains (NUTS)")
    p.add_argument("--thin", type=int, default=1, help="Period for saving samples (NUTS)")
    p.add_argument("--iter", type=int, default=100000,
                   help="Maximum iterations (vb) or iterations including warmup (nuts)")
    p.add_argument("-M", "--metadata",
                   help="Phylogeography (--geo): tab-separated metadata file, first column the taxon")
    p.add_argument("--metadata_key", help="Phylogeography: metadata column holding the location [default: Country]")
    p.add_argument("--ancestral", action="store_true",
                   help="Phylogeography (--geo): after sampling, write OUT.trees (the tree annotated with every node's "
                        "posterior location and every branch's expected migrations) and OUT.jumps.tsv (expected "
                        "migrations between locations and time spent in each)")
    p.add_argument("--ancestral_seq", action="store_true",
                   help="After sampling, evaluate the posterior draws once more and write OUT.ancestral.fasta (the modal "
                        "state of every internal node at every site), OUT.ancestral.tsv (its state probabilities per "
                        "pattern), OUT.siterates.tsv (every site's posterior mean rate and rate-category probabilities; "
                        "with -C > 1) and OUT.ancestral.trees (the tree with posterior mean branch lengths, every edge "
                        "annotated with its expected number of substitutions)")
    p.add_argument("--codon_ancestral", action="store_true",
                   help="--codon: after sampling, evaluate the posterior draws once more on the K-state summaries "
                        "(kseq.DeviceKStateSummaries, DESIGN.md 5j) and write OUT.ancestral.fasta (the modal codon of "
                        "every internal node at every codon site), OUT.ancestral.tsv (that codon, its amino acid and "
                        "its posterior probability), OUT.codon_branches.tsv (per branch the expected synonymous and "
                        "nonsynonymous substitutions S and N, mean and 95 %% interval, and dN/dS) and "
                        "OUT.ancestral.trees (posterior mean branch lengths, every edge annotated [&S=...,N=...])")
    p.add_argument("--trees",
                   help="Phylogeography (--geo): a NEXUS or Newick file holding a sample of trees on the taxa of -t; "
                        "the likelihood is the equal-weight mixture over them (-t then only fixes the taxon order). "
                        "With --ancestral: OUT.jumps.tsv, OUT.root.tsv and OUT.treeprob.tsv")
    p.add_argument("--trees_burnin", type=float, default=0.0,
                   help="--trees: leading fraction of the file's trees to drop [default: %(default)s]")
    p.add_argument("--trees_max", type=int, default=0,
                   help="--trees: keep at most this many evenly spaced trees after the burn-in (0: all)")
    p.add_argument("--topologies",
                   help="A NEXUS or Newick file of tree topologies on the taxa of -t: the model (-a vb -q meanfield, no "
                        "--clock) is fitted to every one of them in lockstep on one forest likelihood. Writes "
                        "OUT_tree{k}, OUT_tree{k}.diag and OUT_tree{k}.trees per topology k and OUT.topologies.tsv "
                        "(ELBO, importance-sampling marginal likelihood and posterior per topology)")
    p.add_argument("--topologies_burnin", type=float, default=0.0,
                   help="--topologies: leading fraction of the file's trees to drop [default: %(default)s]")
    p.add_argument("--topologies_max", type=int, default=0,
                   help="--topologies: keep at most this many evenly spaced trees after the burn-in (0: all)")
    p.add_argument("--partitions", metavar="FILE",
                   help="A RAxML / IQ-TREE style partition file ('DNA, name = 1-658\\3, 2-658\\3' per line; 1-based "
                        "inclusive ranges, optional \\stride). Every partition gets its own substitution and site-rate "
                        "parameters (columns suffixed _p1, _p2, ...) and a relative rate mu.k on the shared tree; "
                        "writes OUT.partitions.tsv (name, sites, patterns, posterior mean and 95%% interval of mu.k)")
    p.add_argument("--device", type=int, default=None, help="HIP device (default LOCAL_RANK or 0)")
    p.add_argument("--rescaling", action="store_true",
                   help="Rescale the tree likelihood's partials (needed past roughly 400 taxa, where the per-site "
                        "likelihood leaves the fp64 range). The reference has no such option for the tree "
                        "likelihood: its --rescaling_geo belongs to phylogeography only")
    return p


class GeoSpec:
    """The options of a ``--geo`` model description (generate_script.py:1168-1170:
    ``get_model`` returns the geo model alone, whatever else is set)."""

    def __init__(self, rescaling_geo=False, geo_clock=None, geo_clock_prior=None):
        self.geo = True
        self.rescaling_geo = bool(rescaling_geo)
        if geo_clock is not None:  # a description without a clock is the one it always was
            self.geo_clock = geo_clock  # "estimate" or the fixed rate
        if geo_clock_prior is not None:
            self.geo_clock_prior = [float(v) for v in geo_clock_prior]


def _geo_clock_options(arg):
    """(clock, prior) of --geo_clock / --geo_rate / --geo_clock_prior: (None |
    "estimate" | float, None | (shape, rate)); refuses what does not fit."""
    estimate = bool(getattr(arg, "geo_clock", False))
    rate = getattr(arg, "geo_rate", None)
    prior = getattr(arg, "geo_clock_prior", None)
    if not arg.geo:
        for flag, given in (("--geo_clock", estimate), ("--geo_rate", rate is not None),
                            ("--geo_clock_prior", prior is not None)):
            if given:
                raise SystemExit("the trait clock rate (%s) needs --geo" % flag)
        return None, None
    if estimate and rate is not None:
        raise SystemExit("--geo_clock estimates the trait clock rate and --geo_rate fixes it: give one of them")
    if prior is not None and not estimate:
        raise SystemExit("--geo_clock_prior is the prior of an estimated rate: it needs --geo_clock")
    if rate is not None and not (rate > 0.0 and np.isfinite(rate)):
        raise SystemExit("--geo_rate must be a positive number")
    if prior is not None:
        try:
            prior = tuple(float(v) for v in prior.split(","))
            if len(prior) != 2 or not all(v > 0.0 and np.isfinite(v) for v in prior):
                raise ValueError
        except ValueError:
            raise SystemExit("--geo_clock_prior takes SHAPE,RATE, two positive numbers")
    return ("estimate" if estimate else rate), prior


def _codon_refusals(arg):
    """--codon with what it does not cover: refused before anything is sampled or written."""
    sites = getattr(arg, "codon_sites", None)
    anc = bool(getattr(arg, "codon_ancestral", False))
    if not getattr(arg, "codon", False):
        if sites:
            raise SystemExit("--codon_sites needs --codon")
        if anc:
            raise SystemExit("--codon_ancestral needs --codon")
        return
    if anc and getattr(arg, "ancestral_seq", False):
        raise SystemExit("--codon_ancestral is not supported with --ancestral_seq")
    if anc and getattr(arg, "algorithm", None) == "vb" and getattr(arg, "samples", 1) <= 0:
        raise SystemExit("--codon_ancestral needs at least one posterior draw (--samples)")
    if sites:
        from .codon import parse_site_model
        try:
            parse_site_model(sites)
        except ValueError as e:
            raise SystemExit("--codon_sites: %s" % e)
    for what, bad in (("--geo", arg.geo), ("--topologies", bool(getattr(arg, "topologies", None))),
                      ("--partitions", bool(getattr(arg, "partitions", None))),
                      ("--ancestral_seq", bool(getattr(arg, "ancestral_seq", False))),
                      ("--rescaling", bool(getattr(arg, "rescaling", False)))):
        if bad:
            raise SystemExit("--codon is not supported with %s" % what)


def _spec(arg):
    clock, prior = _geo_clock_options(arg)
    _codon_refusals(arg)
    if arg.geo:
        return GeoSpec(arg.rescaling_geo, clock, prior)
    if getattr(arg, "metadata", None):
        raise SystemExit("a metadata file (-M) needs --geo")
    if getattr(arg, "trees", None):
        raise SystemExit("a tree sample (--trees) needs --geo")
    spec = ModelSpec.from_args(arg)
    if getattr(arg, "codon", False):  # a description without --codon is the one it always was
        spec.codon = True
        spec.codon_freqs = arg.codon_freqs
        if getattr(arg, "codon_sites", None):  # a description without --codon_sites is the one it always was
            spec.codon_sites = arg.codon_sites
    return spec


def artifact_path(script):
    """phylostan.py:155-158 / :292-294: the compiled model's file name."""
    binary = script.replace(".stan", ".pkl")
    return script + ".pkl" if binary == script else binary


def compile_artifact(spec, script):
    """Load the HIP engine and write the compiled-model artifact (JSON)."""
    import hashlib
    from . import _lib
    _lib.load()
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "phylo_hip.hip")
    h = hashlib.sha1()
    if os.path.exists(src):
        with open(src, "rb") as fp:
            h.update(fp.read())
    doc = {"phylostan_amd_compiled": 1, "script": script, "options": dict(vars(spec)),
           "engine": _lib.LIB_PATH, "kernel_source_sha1": h.hexdigest()[:12],
           "note": "compiled-model artifact of the GPU engine (JSON; replaces the pickled pystan StanModel)"}
    path = artifact_path(script)
    with open(path, "w") as fp:
        json.dump(doc, fp, indent=1)
    return path


def load_artifact(script):
    path = artifact_path(script)
    try:
        with open(path) as fp:
            doc = json.load(fp)
    except (ValueError, UnicodeDecodeError):  # e.g. a real pystan pickle left at that path
        raise SystemExit("%s is not a compiled-model artifact of this engine" % path)
    if not isinstance(doc, dict) or doc.get("phylostan_amd_compiled") != 1:
        raise SystemExit("%s is not a compiled-model artifact of this engine" % path)
    from . import _lib
    _lib.load()
    return doc


def build(arg):
    spec = _spec(arg)
    doc = {"phylostan_amd_model": 1, "options": dict(vars(spec)),
           "note": "model description for the GPU engine (replaces the emitted Stan program)"}
    with open(arg.script, "w") as fp:
        json.dump(doc, fp, indent=1)
    if arg.compile:
        path = compile_artifact(spec, arg.script)
        print("GPU engine: %s (compiled model %s)" % (os.environ.get("PHYLO_HIP_LIB", "libphylo_hip.so"), path))


def _read_script(path):
    try:
        with open(path) as fp:
            doc = json.load(fp)
        return doc.get("options") if isinstance(doc, dict) and "phylostan_amd_model" in doc else None
    except (OSError, ValueError):
        return None


def load_run_data(arg):
    rooted = arg.clock is not None
    d = dataio.load(arg.tree, arg.input, rooted=rooted, heterochronous=arg.heterochronous or bool(arg.dates),
                    dates=arg.dates)
    return d


def run_geo(arg, likelihood_factory=None, log=print):
    """``run --geo -M FILE``: the discrete-trait model of the locations in FILE
    on the tree's own branch lengths (phylostan.py:206-253, generate_script.py:
    1102-1165).  No alignment is read.  ``likelihood_factory(tips, peel0,
    max_draws=, device=)`` replaces the device engine (the CPU suite's).

    With ``--trees FILE`` the likelihood is the equal-weight mixture over the
    trees of FILE that ``geo.select_trees`` keeps (``--trees_burnin``,
    ``--trees_max``); ``-t`` fixes the taxon order alone, and the factory is
    called as ``likelihood_factory(tips, peels, blens, max_draws=, device=)``."""
    from . import geo
    if not arg.metadata:
        raise SystemExit("phylogeography (--geo) needs a metadata file (-M)")
    spec = _spec(arg)
    opts = _read_script(arg.script)
    if likelihood_factory is None:
        if arg.compile or not os.path.lexists(artifact_path(arg.script)):
            compile_artifact(spec, arg.script)
        else:
            opts = load_artifact(arg.script)["options"]
    if opts is not None and not opts.get("geo"):
        raise SystemExit("run option geo=True differs from the built model")
    clock, clock_prior = getattr(spec, "geo_clock", None), getattr(spec, "geo_clock_prior", None)
    if opts is not None and opts.get("geo_clock") != clock:
        raise SystemExit("run option geo_clock=%r differs from the built model" % (clock,))
    if opts is not None and opts.get("geo_clock_prior") != clock_prior:
        raise SystemExit("run option geo_clock_prior=%r differs from the built model" % (clock_prior,))
    tree = dataio.read_tree(arg.tree)
    tree.resolve_polytomies(update_bipartitions=True)
    dataio.setup_indexes(tree)
    taxa = [t.label for t in tree.taxon_namespace]
    S = len(taxa)
    peel0 = np.asarray(dataio.unrooted_peel(dataio.get_peeling_order(tree)), dtype=np.int32) - 1
    try:
        blens = geo.tree_branch_lengths(tree, peel0)
    except ValueError as e:  # phylostan.py:242-243
        print(str(e), file=sys.stderr)
        raise SystemExit(3)
    try:
        tips, states = geo.read_metadata(arg.metadata, key=arg.metadata_key or "Country", taxa=taxa)
    except ValueError as e:
        raise SystemExit(str(e))
    K = len(states)
    log('"' + '","'.join(states) + '"')  # phylostan.py:229
    log("Number of sequences: {} states {} ".format(S, K))
    if K < 2 or K > geo.K_MAX:
        raise SystemExit("phylogeography needs 2 to %d distinct locations, found %d" % (geo.K_MAX, K))
    chains = max(1, arg.chains) if arg.algorithm in ("nuts", "hmc") else 1
    max_draws = chains if arg.algorithm in ("nuts", "hmc") else max(arg.elbo_samples, arg.grad_samples, 1)
    sample = getattr(arg, "trees", None)
    kept_trees = None
    if sample:
        from . import treeio
        trees = treeio.read_trees(sample)
        try:
            kept_trees = geo.select_trees(len(trees), arg.trees_burnin, arg.trees_max)
            if kept_trees.size == 0:
                raise ValueError("no tree of %s is left after the burn-in" % sample)
            peels, tblens = geo.tree_sample([trees[i] for i in kept_trees], taxa)
        except ValueError as e:
            raise SystemExit("--trees: %s" % e)
        log("Tree sample: %d of the %d trees of %s" % (kept_trees.size, len(trees), sample))
    if likelihood_factory is None:
        dev = arg.device if arg.device is not None else int(os.environ.get("LOCAL_RANK", "0"))
        if sample:
            lik = geo.GeoTreesLikelihood(tips, peels, tblens, max_draws=max_draws, device=dev)
        else:
            lik = geo.GeoLikelihood(tips, peel0, max_draws=max_draws, device=dev)
    elif sample:
        lik = likelihood_factory(tips, peels, tblens, max_draws=max_draws, device=0)
    else:
        lik = likelihood_factory(tips, peel0, max_draws=max_draws, device=0)
    if clock is not None and not hasattr(lik, "evaluate_rows_clock"):
        raise SystemExit("a trait clock rate needs a likelihood with evaluate_rows_clock")
    if clock is None:
        post = geo.GeoTreesPosterior(K, lik) if sample else geo.GeoPosterior(K, blens, lik)
    elif sample:
        post = geo.GeoTreesPosterior(K, lik, clock=clock, clock_prior=clock_prior)
    else:
        post = geo.GeoPosterior(K, blens, lik, clock=clock, clock_prior=clock_prior)
    if post.clock_estimated:
        log("Trait clock rate: estimated, Gamma(%g, %g) prior (%s length %g)"
            % (post.clock_prior + ("mean tree" if sample else "tree",
                                   lik.mean_length if sample else geo.mean_tree_length(blens))))
    elif clock is not None:
        log("Trait clock rate: fixed at %g" % clock)
    seed = arg.seed if arg.seed is not None else int(time.time()) % 100000
    rng = np.random.default_rng(seed)
    names = post.column_names()
    config = [("model", "phylostan_amd phylogeography (GPU likelihood; Stan runtime removed)"),
              ("method", arg.algorithm), ("seed", seed), ("dimension", post.dim)]
    sample_path = arg.output
    # no .trees file unless --ancestral asks for the annotated one: a geo sample file has no heights / blens
    # columns to annotate a tree with
    ancestral = bool(getattr(arg, "ancestral", False))
    if ancestral and not hasattr(lik, "evaluate_summaries"):
        raise SystemExit("--ancestral needs a likelihood with evaluate_summaries")
    if arg.algorithm == "vb":
        from .advi import ADVI
        diag = stan_io.DiagWriter(sample_path + ".diag", config)
        adv = ADVI(post, rng, grad_samples=arg.grad_samples, elbo_samples=arg.elbo_samples, log=log)
        q0 = post.initialize(rng)
        t0 = time.time()
        q, eta, iters = adv.run(q0, eta=arg.eta, adapt_engaged=arg.eta is None, tol_rel_obj=arg.tol_rel_obj,
                                max_iterations=arg.iter, diag=diag, family=arg.variational)
        diag.close()
        log("TIME: %.3f" % (time.time() - t0))
        mean_row = post.flat_rows(q.mu[None])[0]
        draws = post.flat_rows(q.sample(rng, arg.samples)) if arg.samples > 0 else np.zeros((0, len(names)))
        stan_io.write_vb_csv(sample_path, names, mean_row, draws,
                             config + [("algorithm", arg.variational), ("iter", iters), ("eta", eta),
                                       ("elbo_samples", arg.elbo_samples),
                                       ("grad_samples", arg.grad_samples), ("tol_rel_obj", arg.tol_rel_obj),
                                       ("output_samples", arg.samples)], eta)
        stan_io.parse_log(sample_path, 0.05)
        if ancestral and sample:
            geo_trees_ancestral(states, kept_trees, lik, max_draws, draws, sample_path, log, post=post)
        elif ancestral:
            geo_ancestral(tree, peel0, states, blens, lik, max_draws, draws, sample_path, log, post=post)
        return post
    from .nuts import run_chains
    num_warmup = arg.iter // 2
    num_samples = arg.iter - num_warmup
    q0s = [post.initialize(np.random.default_rng((seed, c, 0))) for c in range(chains)]
    t0 = time.time()
    res = run_chains(post, q0s, [(seed, c) for c in range(chains)], num_warmup=num_warmup,
                     num_samples=num_samples, thin=arg.thin, progress=log, algorithm=arg.algorithm)
    el = time.time() - t0
    kept = []
    for c, ch in enumerate(res):
        rows = post.flat_rows(np.stack([dr[0] for dr in ch.draws]))
        kept.append(rows[[not dr[8] for dr in ch.draws]])  # the sample file's rows: warmup draws are not written
        path = sample_path if chains == 1 else sample_path + "_{}.csv".format(c)
        stan_io.write_nuts_csv(path, names, ch, rows,
                               config + [("chain", c), ("num_warmup", num_warmup), ("num_samples", num_samples),
                                         ("thin", arg.thin), ("gradient_evaluations", ch.n_grad)],
                               elapsed=(el / 2, el / 2), algorithm=arg.algorithm)
        stan_io.parse_log(path, 0.05)
    if ancestral and sample:
        geo_trees_ancestral(states, kept_trees, lik, max_draws, np.concatenate(kept), sample_path, log, post=post)
    elif ancestral:  # one summary over every kept draw of every chain
        geo_ancestral(tree, peel0, states, blens, lik, max_draws, np.concatenate(kept), sample_path, log, post=post)
    return post


def _draw_clock(post, params, K):
    """(params [n, R + K], mu [n] or None) of the sample file's rows: an
    estimated clock's ``rate_geo`` is their last column."""
    width = K * (K - 1) // 2 + K
    if post is None or not post.has_clock:
        return params, None
    if post.clock_estimated:
        return params[:, :width], params[:, width].copy()
    return params, np.full(params.shape[0], post.clock_fixed)


def geo_clock_rates(states, params, mu, ok, stem, post, log=print):
    """With a trait clock: ``stem.rates.tsv``, the posterior mean of mu Q_ij
    (migrations i -> j per lineage per unit of the tree's time; the diagonal
    blank), and the log line of ``rate_geo``."""
    from . import geo
    K = len(states)
    R = K * (K - 1) // 2
    mean = np.zeros((K, K))
    for n in np.flatnonzero(ok):
        mean += mu[n] * geo.rate_matrix(params[n, R:], params[n, :R])[0]
    mean /= max(int(ok.sum()), 1)
    with open(stem + ".rates.tsv", "w") as fp:
        fp.write("\t".join(["from\\to"] + [str(x) for x in states]) + "\n")
        for i in range(K):
            fp.write("\t".join([str(states[i])] + ["" if i == j else repr(float(mean[i, j])) for j in range(K)]) + "\n")
    if post.clock_estimated:
        lo, hi = np.quantile(mu[ok], (0.025, 0.975))
        log("rate_geo: posterior mean %.6g, 95%% interval %.6g .. %.6g (migrations per lineage per unit of tree time)"
            % (mu[ok].mean(), lo, hi))
    return mean


def geo_ancestral(tree, peel0, states, blens, lik, max_draws, params, stem, log=print, post=None):
    """``run --geo --ancestral``: the posterior summaries of the constrained
    draws ``params [n, R + K]`` (``evaluate_summaries`` in chunks of
    ``max_draws``), averaged; writes ``stem.trees`` and ``stem.jumps.tsv`` and
    logs one line.  Returns the ``geo.GeoSummary``.  With a trait clock
    (``post``) the times of ``stem.jumps.tsv`` are in the tree's unit and
    ``stem.rates.tsv`` is written (``geo_clock_rates``)."""
    from . import geo
    params = np.atleast_2d(np.asarray(params, np.float64))
    if params.shape[0] == 0:
        raise SystemExit("--ancestral needs at least one posterior draw (--samples)")
    params, mu = _draw_clock(post, params, len(states))
    acc = geo.GeoSummary(len(tree.taxon_namespace), len(states))
    finite = np.zeros(params.shape[0], bool)
    for at in range(0, params.shape[0], max_draws):
        chunk = params[at:at + max_draws]
        tb = np.broadcast_to(blens, (chunk.shape[0], blens.size))
        res = lik.evaluate_summaries(tb, chunk) if mu is None else \
            lik.evaluate_summaries_clock(tb, chunk, mu[at:at + max_draws])
        finite[at:at + max_draws] = np.isfinite(res[0][:, 0])
        acc.add(*res)
    if acc.count == 0:
        raise SystemExit("--ancestral: no posterior draw has a finite likelihood")
    marg, bjumps = acc.marg, acc.bjumps
    stan_io.write_geo_nexus(tree, stem + ".trees", states, marg, bjumps)
    stan_io.write_jumps_tsv(stem + ".jumps.tsv", states, acc.migrations, acc.times)
    root = marg[-1]
    log("Expected migrations: %.3f over %d draws; root location: %s (probability %.3f)"
        % (acc.migrations.sum(), acc.count, states[int(np.argmax(root))], root.max()))
    if mu is not None:
        geo_clock_rates(states, params, mu, finite, stem, post, log)
    return acc


def geo_trees_ancestral(states, tree_ids, lik, max_draws, params, stem, log=print, post=None):
    """``run --geo --trees --ancestral``: the summaries of the constrained
    draws ``params [n, R + K]`` that do not depend on a topology, averaged over
    the draws with a finite likelihood.  Writes ``stem.jumps.tsv`` (as the
    single-tree run), ``stem.root.tsv`` (location, probability) and
    ``stem.treeprob.tsv`` (tree -- its index in the --trees file -- and its
    posterior probability averaged over the draws); no annotated ``.trees``
    file, since nodes do not correspond across topologies.  Logs one line and
    returns ``(jumps [K, K], root [K], tree_prob [T])``.  With a trait clock
    (``post``) the times are in the trees' unit and ``stem.rates.tsv`` is
    written (``geo_clock_rates``)."""
    params = np.atleast_2d(np.asarray(params, np.float64))
    if params.shape[0] == 0:
        raise SystemExit("--ancestral needs at least one posterior draw (--samples)")
    K = len(states)
    params, mu = _draw_clock(post, params, K)
    jumps, root, prob, count = np.zeros((K, K)), np.zeros(K), np.zeros(len(tree_ids)), 0
    finite = np.zeros(params.shape[0], bool)
    for at in range(0, params.shape[0], max_draws):
        if mu is None:
            rows, j, r = lik.evaluate_summaries(params[at:at + max_draws])
        else:
            rows, j, r = lik.evaluate_summaries_clock(params[at:at + max_draws], mu[at:at + max_draws])
        ok = np.isfinite(rows[:, 0])
        finite[at:at + max_draws] = ok
        count += int(ok.sum())
        jumps += j[ok].sum(0)
        root += r[ok].sum(0)
        prob += lik.tree_posterior(rows)[ok].sum(0)
    if count == 0:
        raise SystemExit("--ancestral: no posterior draw has a finite likelihood")
    jumps, root, prob = jumps / count, root / count, prob / count
    root, prob = root / root.sum(), prob / prob.sum()
    migrations = jumps.copy()
    np.fill_diagonal(migrations, 0.0)
    stan_io.write_jumps_tsv(stem + ".jumps.tsv", states, migrations, np.diag(jumps).copy())
    with open(stem + ".root.tsv", "w") as fp:
        fp.write("location\tprobability\n")
        for k in range(K):
            fp.write("%s\t%r\n" % (states[k], float(root[k])))
    with open(stem + ".treeprob.tsv", "w") as fp:
        fp.write("tree\tprobability\n")
        for t, i in enumerate(tree_ids):
            fp.write("%d\t%r\n" % (int(i), float(prob[t])))
    log("Expected migrations: %.3f over %d draws and %d trees; root location: %s (probability %.3f)"
        % (migrations.sum(), count, len(tree_ids), states[int(np.argmax(root))], root.max()))
    if mu is not None:
        geo_clock_rates(states, params, mu, finite, stem, post, log)
    return jumps, root, prob


def meanfield_log_q(q, U):
    """log N(u; mu, diag(exp(omega)^2)) of draws U [n, dim]."""
    eta = (U - q.mu) * np.exp(-q.omega)
    return -0.5 * (eta * eta).sum(axis=1) - float(q.omega.sum()) - 0.5 * len(q.mu) * math.log(2.0 * math.pi)


def topology_estimates(post, results, samples):
    """{t: (elbo, log_ml_is)} from every topology's output draws, all in one
    batched pass: elbo = sum of the finite log p / samples + entropy
    (``ADVI.calc_elbo``'s rule), log_ml_is = log(sum exp(log p - log q) /
    samples) over the same rows.  Without output draws: the last ELBO of the
    run (nan when none was taken) and nan."""
    est = {}
    live = [t for t, r in results.items() if r.q is not None]
    for t, r in results.items():
        last = r.trace[-1][2] if r.trace else float("nan")
        est[t] = (last if r.q is not None else -math.inf, float("nan"))
    if samples <= 0 or not live:
        return est
    U = np.concatenate([results[t].draws for t in live])
    tags = np.concatenate([np.full(results[t].draws.shape[0], t, np.int32) for t in live])
    lp = post.log_prob_grad(U, propto=False, need_grad=False, tags=tags)[0]
    lo = 0
    for t in live:
        q, n = results[t].q, results[t].draws.shape[0]
        l = lp[lo:lo + n]
        ok = np.isfinite(l)
        elbo = float(l[ok].sum()) / n + q.entropy()
        lw = l[ok] - meanfield_log_q(q, results[t].draws[ok])
        lml = float(lw.max() + math.log(np.exp(lw - lw.max()).sum() / n)) if ok.any() else -math.inf
        est[t] = (elbo, lml)
        lo += n
    return est


def run_topologies(arg, likelihood_factory=None, log=print):
    """``run --topologies FILE``: mean-field ADVI of a model without a clock
    on every topology of FILE (those ``--topologies_burnin`` / ``_max`` keep),
    in lockstep on one forest likelihood (forest.py).  ``-t`` supplies the
    taxon order.  ``likelihood_factory(tipcodes, weights, peels, rooted, model,
    C)`` replaces the device forest (the CPU suite's stand-in).  Returns
    ``(posterior, {k: LockstepResult})``, k the topology's index in FILE."""
    from . import forest as fr
    for what, bad in (("--geo", arg.geo), ("--clock", arg.clock is not None),
                      ("-a %s" % arg.algorithm, arg.algorithm != "vb"),
                      ("-q %s" % arg.variational, arg.variational != "meanfield"),
                      ("--rescaling", getattr(arg, "rescaling", False))):
        if bad:
            raise SystemExit("%s is not supported with --topologies (a model without a clock, -a vb -q meanfield)" % what)
    spec = _spec(arg)
    opts = _read_script(arg.script)
    if likelihood_factory is None:
        if arg.compile or not os.path.lexists(artifact_path(arg.script)):
            compile_artifact(spec, arg.script)
        else:
            opts = load_artifact(arg.script)["options"]
    if opts is not None:
        for k in ("model", "categories", "invariant", "clock", "estimate_rate", "coalescent", "heterochronous"):
            if opts.get(k) != getattr(spec, k):
                raise SystemExit("run option %s=%r differs from the built model (%r)" % (k, getattr(spec, k),
                                                                                        opts.get(k)))
    if not arg.input:
        raise SystemExit("an alignment (-i) is required")
    try:
        fd = dataio.load_forest(arg.tree, arg.topologies, arg.input, arg.topologies_burnin, arg.topologies_max)
    except ValueError as e:
        raise SystemExit("--topologies: %s" % e)
    d, T, C = fd.data, fd.T, spec.C
    log("Number of sequences: {} length {} ".format(d.S, int(np.sum(d.weights))))
    log("Model: " + arg.model)
    log("Topologies: %d of %s" % (T, arg.topologies))
    if likelihood_factory is None:
        dev = arg.device if arg.device is not None else int(os.environ.get("LOCAL_RANK", "0"))
        max_rows = min(T * max(arg.elbo_samples, arg.grad_samples, 1), 4096)  # larger calls are chunked
        forest = fr.ForestLikelihood(fd.tipcodes, fd.weights, fd.peels, False, arg.model, C, max_rows=max_rows,
                                     device=dev)
    else:
        forest = likelihood_factory(fd.tipcodes, fd.weights, fd.peels, False, arg.model, C)
    # without a clock the branch lengths are the parameters: one posterior serves every topology
    post = Posterior(spec, TreeData(d.S, d.peel0, d.map, None, None), fr.TaggedLikelihood(forest))
    seed = arg.seed if arg.seed is not None else int(time.time()) % 100000
    names = post.column_names()
    config = [("model", "phylostan_amd (GPU likelihood; Stan runtime removed)"), ("method", arg.algorithm),
              ("seed", seed), ("dimension", post.dim)]
    paths = {j: "%s_tree%d" % (arg.output, int(fd.index[j])) for j in range(T)}
    diags = {}

    def diag_of(j):
        diags[j] = stan_io.DiagWriter(paths[j] + ".diag", config + [("topology", int(fd.index[j]))])
        return diags[j]
    t0 = time.time()
    results = fr.lockstep_advi(post, range(T), seed, grad_samples=arg.grad_samples, elbo_samples=arg.elbo_samples,
                               eta=arg.eta, tol_rel_obj=arg.tol_rel_obj, max_iterations=arg.iter, samples=arg.samples,
                               diag=diag_of, ids=fd.index, eval_elbo=getattr(arg, "eval_elbo", 100))
    for w in diags.values():
        w.close()
    log("TIME: %.3f" % (time.time() - t0))
    est = topology_estimates(post, results, arg.samples)
    elbos = np.array([est[j][0] for j in range(T)], np.float64)
    fin = np.isfinite(elbos)
    prob = np.zeros(T)
    if fin.any():
        w = np.exp(elbos[fin] - elbos[fin].max())
        prob[fin] = w / w.sum()
    for j in range(T):
        r = results[j]
        if r.q is None:
            log("topology %d failed: %s" % (int(fd.index[j]), r.error))
            continue
        draws = post.flat_rows(r.draws) if arg.samples > 0 else np.zeros((0, len(names)))
        stan_io.write_vb_csv(paths[j], names, post.flat_rows(r.q.mu[None])[0], draws,
                             config + [("topology", int(fd.index[j])), ("algorithm", arg.variational),
                                       ("iter", r.iterations), ("eta", r.eta), ("elbo_samples", arg.elbo_samples),
                                       ("grad_samples", arg.grad_samples), ("tol_rel_obj", arg.tol_rel_obj),
                                       ("output_samples", arg.samples)], r.eta)
        stan_io.convert_samples_to_nexus(fd.trees[j], paths[j], paths[j] + ".trees", arg.rate)
    with open(arg.output + ".topologies.tsv", "w") as fp:
        fp.write("tree\titerations\tconverged\teta\telbo\tlog_ml_is\tposterior\n")
        for j in range(T):
            r = results[j]
            fp.write("%d\t%d\t%d\t%r\t%r\t%r\t%r\n" % (int(fd.index[j]), r.iterations, int(r.converged),
                                                       float(r.eta) if r.eta is not None else float("nan"),
                                                       float(est[j][0]), float(est[j][1]), float(prob[j])))
    if hasattr(forest, "close"):
        forest.close()
    return post, {int(fd.index[j]): results[j] for j in range(T)}


SEQ_SUMMARY_CHUNK = 64  # draws per call of the summary pass


def sequence_summaries(d, post, U, C, stem, summaries, full_lik, log=print):
    """``run --ancestral_seq``: the summary pass over the unconstrained
    posterior draws ``U [n, dim]``.  Every chunk goes through ``summaries.add``
    (seqsum.py: node posteriors, category posteriors and site rates, summed
    over the draws where they are formed) and through ``full_lik``'s full rows,
    whose dlogL/dP gives the expected substitutions per branch
    (``models.expected_substitutions``).  Writes ``stem.ancestral.fasta``,
    ``stem.ancestral.tsv``, ``stem.siterates.tsv`` (C > 1) and
    ``stem.ancestral.trees``, logs one line and returns the
    ``seqsum.SeqSummary``."""
    from . import models, seqsum
    U = np.atleast_2d(np.asarray(U, np.float64))
    blens, mv = post.blens(U), post.model_vectors(U)
    acc = seqsum.SeqSummary(d.S, d.P, C, blens.shape[1])
    summaries.reset()
    for at in range(0, U.shape[0], SEQ_SUMMARY_CHUNK):
        bl, m = blens[at:at + SEQ_SUMMARY_CHUNK], mv[at:at + SEQ_SUMMARY_CHUNK]
        ll = summaries.add(bl, m)
        ok = np.isfinite(ll)
        subs = np.zeros(bl.shape)
        if ok.any():
            G = np.stack([r.dLdP for r in full_lik.evaluate_batch(bl[ok], m[ok])])
            subs[ok] = models.expected_substitutions(G, bl[ok], m[ok, 10:10 + C], m[ok, :4], m[ok, 4:10])
        acc.add_branches(ll, subs, bl)
    acc.finish(*summaries.read())
    if acc.count == 0:
        raise SystemExit("--ancestral_seq: no posterior draw has a finite likelihood")
    site_pattern = d.site_pattern if getattr(d, "site_pattern", None) is not None else \
        np.repeat(np.arange(d.P), np.asarray(d.weights).astype(np.int64))
    stan_io.write_ancestral_fasta(stem + ".ancestral.fasta", d.S, acc.anc, site_pattern)
    stan_io.write_ancestral_tsv(stem + ".ancestral.tsv", d.S, acc.anc)
    if C > 1:
        stan_io.write_siterates_tsv(stem + ".siterates.tsv", acc.rate, acc.cat, site_pattern)
    stan_io.write_subs_nexus(d.tree, stem + ".ancestral.trees", acc.blens, acc.subs)
    log("Expected substitutions: %.3f over %d draws; mean site rate %.4f"
        % (acc.subs.sum(), acc.count, float(np.mean(acc.rate[site_pattern]))))
    return acc


def codon_summaries(d, post, U, codons, stem, summaries, log=print):
    """``run --codon_ancestral``: the summary pass over the unconstrained posterior draws ``U [n, dim]`` of a
    codon posterior.  Every chunk goes through ``summaries.add`` (kseq.py: the internal nodes' codon posteriors
    summed over the draws where they are formed, the expected synonymous and nonsynonymous substitutions per
    branch per draw).  Writes ``stem.ancestral.fasta``, ``stem.ancestral.tsv``, ``stem.codon_branches.tsv`` and
    ``stem.ancestral.trees``, logs the tree totals and returns (node posteriors ``[S-1, 61, P]``, S ``[n, B]``,
    N ``[n, B]`` of the draws with a likelihood)."""
    from . import codon as cdn
    U = np.atleast_2d(np.asarray(U, np.float64))
    blens, mv = post.blens(U), post.model_vectors(U)
    rho_s, rho_n = cdn.neutral_rates(post.nucleotide_rates(U), post.codon_summary(U)["pi"])
    summaries.reset()
    lls, counts = [], []
    for at in range(0, U.shape[0], SEQ_SUMMARY_CHUNK):
        ll, bc = summaries.add(blens[at:at + SEQ_SUMMARY_CHUNK], mv[at:at + SEQ_SUMMARY_CHUNK])
        lls.append(ll)
        counts.append(bc)
    total, n_finite = summaries.read()
    ok = np.isfinite(np.concatenate(lls))
    if n_finite == 0 or not ok.any():
        raise SystemExit("--codon_ancestral: no posterior draw has a finite likelihood")
    anc = total / n_finite
    bc = np.concatenate(counts)[ok]
    syn, nonsyn = bc[:, 0], bc[:, 1]
    with np.errstate(divide="ignore", invalid="ignore"):
        neutral = float(np.mean(rho_n[ok] / rho_s[ok]))
    stan_io.write_codon_ancestral_fasta(stem + ".ancestral.fasta", d.S, anc, codons[2], cdn.CODONS)
    stan_io.write_codon_ancestral_tsv(stem + ".ancestral.tsv", d.S, anc, codons[2], cdn.CODONS, cdn.AMINO)
    stan_io.write_codon_branches_tsv(stem + ".codon_branches.tsv", syn, nonsyn, neutral)
    stan_io.write_codon_subs_nexus(d.tree, stem + ".ancestral.trees", blens[ok].mean(axis=0), syn.mean(axis=0),
                                   nonsyn.mean(axis=0))
    ts, tn = float(syn.mean(axis=0).sum()), float(nonsyn.mean(axis=0).sum())
    log("Codon substitutions: S %.3f, N %.3f over %d draws; tree dN/dS %.4f"
        % (ts, tn, int(n_finite), (tn / ts) / neutral if ts > 0 else float("nan")))
    return anc, syn, nonsyn


def load_partitions(arg, d, log=print):
    """(partitions, their (tipcodes, weights, site_pattern)) of --partitions FILE on the run's alignment, in the
    taxon order of ``d``; one log line per partition."""
    from . import partition as pt
    chars = dataio.alignment_matrix(dataio.read_alignment(arg.input), d.tree.taxon_namespace)
    try:
        parts = pt.read_partitions(arg.partitions, chars.shape[1])
    except (OSError, ValueError) as e:
        raise SystemExit("--partitions: %s" % e)
    split = pt.split_alignment(chars, parts)
    for p, (tip, _, _) in zip(parts, split):
        log("Partition {}: {} sites, {} patterns".format(p.name, p.sites.size, tip.shape[1]))
    return parts, split


def partitioned_likelihood(arg, d, scheme, C, max_draws, likelihood_factory=None):
    """The device's ``PartitionedLikelihood``; with ``likelihood_factory`` (the run's single-alignment hook, called
    once per partition) ``partition_host`` over its likelihoods."""
    from . import partition as pt
    split = scheme[1]
    if likelihood_factory is None:
        dev = arg.device if arg.device is not None else int(os.environ.get("LOCAL_RANK", "0"))
        return pt.PartitionedLikelihood([(tip, w) for tip, w, _ in split], d.peel0, d.rooted, arg.model, C,
                                        max_draws=max_draws, device=dev)

    def evaluator(lik):
        def ev(bl, mv, site_ll):
            if hasattr(lik, "evaluate_rows"):
                return lik.evaluate_rows(bl[None], mv[None])[0], None
            r = lik.evaluate_batch(bl[None], mv[None])[0]
            return np.concatenate([[r.loglik], r.grad_blens, r.grad_rs, r.grad_ps, r.grad_freq_root, r.grad_rates,
                                   r.grad_freqs]), None
        return ev
    evs = [evaluator(likelihood_factory(tip, w, d.peel0, d.rooted, arg.model, C)) for tip, w, _ in split]
    return pt.partition_host(evs, d.B, C, [tip.shape[1] for tip, _, _ in split])


def write_partitions_tsv(path, scheme, names, draws, mean_row, log=print):
    """OUT.partitions.tsv: name, sites, patterns, the posterior mean of mu_k and its 95 % interval over the draws
    (one partition: mu = 1)."""
    parts, split = scheme
    K = len(parts)
    with open(path, "w") as fp:
        fp.write("partition\tsites\tpatterns\tmu_mean\tmu_2.5%\tmu_97.5%\n")
        for k, (p, (tip, _, _)) in enumerate(zip(parts, split)):
            if K > 1:
                j = names.index("mu.%d" % (k + 1))
                col = np.asarray(draws)[:, j] if len(draws) else np.array([mean_row[j]])
                mean = float(np.mean(col)) if len(draws) else float(mean_row[j])
                lo, hi = np.percentile(col, [2.5, 97.5])
            else:
                mean = lo = hi = 1.0
            fp.write("%s\t%d\t%d\t%.6g\t%.6g\t%.6g\n" % (p.name, p.sites.size, tip.shape[1], mean, lo, hi))
    log("Partitions: %s" % path)


def run(arg, likelihood_factory=None, log=print, summary_factory=None, codon_summary_factory=None):
    """``summary_factory(tipcodes, weights, peel0, rooted, model, C,
    max_draws=)`` replaces the device's ``seqsum.SequenceSummaries`` for
    ``--ancestral_seq`` (the CPU suite passes ``seqsum.seqsum_host``).
    ``codon_summary_factory(masks, weights, peel0, rooted, K, M, C, labels,
    max_draws=)`` is the summaries class of ``--codon_ancestral``
    (``kseq.DeviceKStateSummaries`` from ``cli.main``)."""
    ancestral_seq = bool(getattr(arg, "ancestral_seq", False))
    if ancestral_seq:  # refused before anything is sampled or written
        for what, bad in (("--geo", arg.geo), ("--topologies", bool(getattr(arg, "topologies", None))),
                          ("--rescaling", bool(getattr(arg, "rescaling", False)))):
            if bad:
                raise SystemExit("--ancestral_seq is not supported with %s" % what)
        if arg.algorithm == "vb" and arg.samples <= 0:
            raise SystemExit("--ancestral_seq needs at least one posterior draw (--samples)")
    _codon_refusals(arg)
    codon = bool(getattr(arg, "codon", False))
    sites = getattr(arg, "codon_sites", None) if codon else None
    if codon and likelihood_factory is None:
        # no fall-back to the host restatement on the product path: a missing kernel is an error
        raise SystemExit("--codon: this build has no device engine bound to cli.run itself: pass the likelihood, "
                         "cli.run(arg, likelihood_factory=kseq.DeviceKStateLikelihood), as cli.main does (DESIGN.md 5j)")
    codon_anc = codon and bool(getattr(arg, "codon_ancestral", False))
    if codon_anc and codon_summary_factory is None:  # as --codon: no fall-back to the host restatement
        raise SystemExit("--codon_ancestral: this build has no device summaries bound to cli.run itself: pass the "
                         "class, cli.run(arg, codon_summary_factory=kseq.DeviceKStateSummaries), as cli.main does "
                         "(DESIGN.md 5j)")
    partitions = getattr(arg, "partitions", None)
    if partitions:  # refused before anything is sampled or written
        for what, bad in (("--geo", arg.geo), ("--topologies", bool(getattr(arg, "topologies", None))),
                          ("--ancestral_seq", ancestral_seq), ("--rescaling", bool(getattr(arg, "rescaling", False)))):
            if bad:
                raise SystemExit("--partitions is not supported with %s" % what)
    if getattr(arg, "topologies", None):
        return run_topologies(arg, likelihood_factory, log)
    if arg.geo:
        return run_geo(arg, likelihood_factory, log)
    if getattr(arg, "ancestral", False):
        raise SystemExit("--ancestral (ancestral locations and migration counts) needs --geo")
    spec = _spec(arg)
    opts = _read_script(arg.script)
    if likelihood_factory is None:  # the GPU engine: compiled-model artifact (phylostan.py:292-300)
        if arg.compile or not os.path.lexists(artifact_path(arg.script)):
            compile_artifact(spec, arg.script)
        else:
            opts = load_artifact(arg.script)["options"]
    if opts is not None:
        for k in ("model", "categories", "invariant", "clock", "estimate_rate", "coalescent", "heterochronous"):
            if opts.get(k) != getattr(spec, k):
                raise SystemExit("run option %s=%r differs from the built model (%r)" % (k, getattr(spec, k),
                                                                                        opts.get(k)))
        if codon or opts.get("codon"):
            for k in ("codon", "codon_freqs") + (("codon_sites",) if getattr(spec, "codon_sites", None)
                                                 or opts.get("codon_sites") else ()):
                if opts.get(k) != getattr(spec, k, None):
                    raise SystemExit("run option %s=%r differs from the built model (%r)" % (k, getattr(spec, k, None),
                                                                                            opts.get(k)))
    if not arg.input:
        raise SystemExit("an alignment (-i) is required")
    d = load_run_data(arg)
    log("Number of sequences: {} length {} ".format(d.S, int(np.sum(d.weights))))
    log("Model: " + arg.model)
    C = spec.C
    chains = max(1, arg.chains) if arg.algorithm in ("nuts", "hmc") else 1
    # draws per likelihood call: one per chain (NUTS / HMC), else the ELBO / gradient samples
    max_draws = chains if arg.algorithm in ("nuts", "hmc") else max(arg.elbo_samples, arg.grad_samples, 1)
    scheme = None
    codons = None
    if codon:
        from . import codon as cdn
        chars = dataio.alignment_matrix(dataio.read_alignment(arg.input), d.tree.taxon_namespace)
        try:
            codons = cdn.codon_alignment(chars, d.taxa)
        except ValueError as e:
            raise SystemExit("--codon: %s" % e)
        log("Codons: {} in {} patterns; frequencies {}".format(int(codons[1].sum()), codons[0].shape[1],
                                                               arg.codon_freqs))
        if sites:
            if cdn.parse_site_model(sites)[1] * spec.C > 16:
                raise SystemExit("--codon_sites %s with %d rate categories: classes times categories must be <= 16"
                                 % (sites, spec.C))
            log("Codon site model: {} ({} classes)".format(sites, cdn.parse_site_model(sites)[1]))
    if partitions:
        scheme = load_partitions(arg, d, log)
    if codons is not None:
        make_lik = None
        if sites:  # the mixture likelihood: one component per omega class
            lik = likelihood_factory(codons[0], codons[1], d.peel0, d.rooted, cdn.K, cdn.parse_site_model(sites)[1], C)
        else:
            lik = likelihood_factory(codons[0], codons[1], d.peel0, d.rooted, cdn.K, C)
    elif scheme is not None:
        make_lik = None
        lik = partitioned_likelihood(arg, d, scheme, C, max_draws, likelihood_factory)
    elif likelihood_factory is None:
        from .engine import TreeLikelihood
        dev = arg.device if arg.device is not None else int(os.environ.get("LOCAL_RANK", "0"))

        def make_lik():
            lk = TreeLikelihood(d.tipcodes, d.weights, d.peel0, d.rooted, arg.model, C, max_draws=max_draws,
                                device=dev, rescaling=getattr(arg, "rescaling", False))
            if max_draws * C <= 256:  # batches within one workgroup per CU: the lowest-latency engine
                lk.prefer_latency_engine()
            return lk
        lik = make_lik()
    else:
        make_lik = None
        lik = likelihood_factory(d.tipcodes, d.weights, d.peel0, d.rooted, arg.model, C)
    tree = TreeData.from_phylodata(d)
    if not spec.heterochronous:
        # --dates alone dates the tips (setup_dates) but, as in the reference,
        # only --heterochronous puts lowers / lower_root into the model's data
        # (phylostan.py:259-263): the model stays homochronous
        tree = TreeData(d.S, d.peel0, d.map, None, None)
    if codons is not None and sites:
        post = cdn.CodonSitesPosterior(spec, tree, lik, arg.codon_freqs, sites,
                                       counts=cdn.codon_counts(codons[0], codons[1]))
    elif codons is not None:
        post = cdn.CodonPosterior(spec, tree, lik, arg.codon_freqs, counts=cdn.codon_counts(codons[0], codons[1]))
    elif scheme is not None:
        from .partition import PartitionedPosterior
        post = PartitionedPosterior(spec, tree, lik, [p.sites.size for p in scheme[0]])
    else:
        post = Posterior(spec, tree, lik, compact_rows=True)
    seed = arg.seed if arg.seed is not None else int(time.time()) % 100000
    rng = np.random.default_rng(seed)
    names = post.column_names()
    config = [("model", "phylostan_amd (GPU likelihood; Stan runtime removed)"), ("method", arg.algorithm),
              ("seed", seed), ("dimension", post.dim)]
    sample_path = arg.output
    tree_path = sample_path + ".trees"

    def codon_sites_pass(U):
        # the recorded draws once more, with the class posteriors: the sampling likelihood serves, its rows unread
        try:
            cls, mean_om, p_pos = cdn.site_summary(post.codon_summary(U)["omegas"], post.class_posteriors(U), codons[2])
        except ValueError as e:
            raise SystemExit("--codon_sites: %s" % e)
        cdn.write_codon_sites_tsv(sample_path + ".codon_sites.tsv", cls, mean_om, p_pos)
        log("Codon sites: %s (%d codons, %d with P(omega > 1) > 0.95)" % (sample_path + ".codon_sites.tsv", len(mean_om),
                                                                        int(np.sum(p_pos > 0.95))))

    def codon_ancestral_pass(U):
        # a context of its own, made after inference is over: the sampling likelihood is left as it was
        summ = codon_summary_factory(codons[0], codons[1], d.peel0, d.rooted, cdn.K,
                                     cdn.parse_site_model(sites)[1] if sites else 1, C, cdn.codon_labels(),
                                     max_draws=SEQ_SUMMARY_CHUNK)
        try:
            return codon_summaries(d, post, U, codons, sample_path, summ, log)
        finally:
            if hasattr(summ, "close"):
                summ.close()

    def summary_pass(U):
        # contexts of its own, made after inference is over: the sampling likelihood is left as it was
        dev = arg.device if arg.device is not None else int(os.environ.get("LOCAL_RANK", "0"))
        if summary_factory is None:
            from .seqsum import SequenceSummaries
            summ = SequenceSummaries(d.tipcodes, d.weights, d.peel0, d.rooted, arg.model, C,
                                     max_draws=SEQ_SUMMARY_CHUNK, device=dev)
        else:
            summ = summary_factory(d.tipcodes, d.weights, d.peel0, d.rooted, arg.model, C, max_draws=SEQ_SUMMARY_CHUNK)
        if likelihood_factory is None:  # full rows (the default of a new context): they carry dlogL/dP
            from .engine import TreeLikelihood
            full = TreeLikelihood(d.tipcodes, d.weights, d.peel0, d.rooted, arg.model, C, max_draws=SEQ_SUMMARY_CHUNK,
                                  device=dev)
        else:
            full = likelihood_factory(d.tipcodes, d.weights, d.peel0, d.rooted, arg.model, C)
        try:
            return sequence_summaries(d, post, U, C, sample_path, summ, full, log)
        finally:
            for ctx in (summ, full):
                if hasattr(ctx, "close"):
                    ctx.close()

    if arg.algorithm == "vb":
        from .advi import ADVI
        diag = stan_io.DiagWriter(sample_path + ".diag", config)
        adv = ADVI(post, rng, grad_samples=arg.grad_samples, elbo_samples=arg.elbo_samples, log=log)
        q0 = post.initialize(rng)
        t0 = time.time()
        q, eta, iters = adv.run(q0, eta=arg.eta, adapt_engaged=arg.eta is None, tol_rel_obj=arg.tol_rel_obj,
                                max_iterations=arg.iter, diag=diag, family=arg.variational)
        diag.close()
        log("TIME: %.3f" % (time.time() - t0))
        mean_row = post.flat_rows(q.mu[None])[0]
        U = q.sample(rng, arg.samples) if arg.samples > 0 else None
        draws = post.flat_rows(U) if arg.samples > 0 else np.zeros((0, len(names)))
        stan_io.write_vb_csv(sample_path, names, mean_row, draws,
                             config + [("algorithm", arg.variational), ("iter", iters), ("eta", eta),
                                       ("elbo_samples", arg.elbo_samples),
                                       ("grad_samples", arg.grad_samples), ("tol_rel_obj", arg.tol_rel_obj),
                                       ("output_samples", arg.samples)], eta)
        stan_io.convert_samples_to_nexus(d.tree, sample_path, tree_path, arg.rate)
        stan_io.parse_log(sample_path, 0.05)
        if ancestral_seq:
            summary_pass(U)
        if scheme is not None:
            post.output_draws = U  # the unconstrained output draws, at full precision (the CSV holds six digits)
            write_partitions_tsv(sample_path + ".partitions.tsv", scheme, names, draws, mean_row, log)
        if codons is not None:
            post.output_draws = U
            cdn.write_codon_tsv(sample_path + ".codon.tsv", post.codon_summary(U if arg.samples > 0 else q.mu[None]))
            log("Codon model: %s" % (sample_path + ".codon.tsv"))
            if sites:
                codon_sites_pass(U if arg.samples > 0 else q.mu[None])
            if codon_anc:
                codon_ancestral_pass(U)
        return post
    from .nuts import run_chains
    num_warmup = arg.iter // 2
    num_samples = arg.iter - num_warmup
    q0s = [post.initialize(np.random.default_rng((seed, c, 0))) for c in range(chains)]
    t0 = time.time()
    # one batched context for all chains: every leapfrog round of all chains
    # is one small-batch likelihood call
    res = run_chains(post, q0s, [(seed, c) for c in range(chains)], num_warmup=num_warmup,
                     num_samples=num_samples, thin=arg.thin, progress=log, algorithm=arg.algorithm)
    el = time.time() - t0
    kept_rows = []
    for c, ch in enumerate(res):
        rows = post.flat_rows(np.stack([dr[0] for dr in ch.draws]))
        kept_rows.append(rows)
        path = sample_path if chains == 1 else sample_path + "_{}.csv".format(c)
        tpath = tree_path if chains == 1 else sample_path + "_{}.trees".format(c)
        if chains == 1 and sample_path.endswith(".csv"):
            tpath = sample_path.replace(".csv", ".trees")
        stan_io.write_nuts_csv(path, names, ch, rows,
                               config + [("chain", c), ("num_warmup", num_warmup), ("num_samples", num_samples),
                                         ("thin", arg.thin), ("gradient_evaluations", ch.n_grad)],
                               elapsed=(el / 2, el / 2), algorithm=arg.algorithm)
        stan_io.convert_samples_to_nexus(d.tree, path, tpath, arg.rate)
        stan_io.parse_log(path, 0.05)
    if ancestral_seq:  # one summary over every kept draw of every chain
        kept = [dr[0] for ch in res for dr in ch.draws if not dr[8]]
        if not kept:
            raise SystemExit("--ancestral_seq: the chains kept no draw")
        summary_pass(np.stack(kept))
    if scheme is not None:
        allrows = np.concatenate(kept_rows)
        write_partitions_tsv(sample_path + ".partitions.tsv", scheme, names, allrows, allrows.mean(axis=0), log)
    if codons is not None:
        cdn.write_codon_tsv(sample_path + ".codon.tsv",
                            post.codon_summary(np.stack([dr[0] for ch in res for dr in ch.draws])))
        log("Codon model: %s" % (sample_path + ".codon.tsv"))
        if sites:
            codon_sites_pass(np.stack([dr[0] for ch in res for dr in ch.draws]))
        if codon_anc:  # one summary over every kept draw of every chain
            kept = [dr[0] for ch in res for dr in ch.draws if not dr[8]]
            if not kept:
                raise SystemExit("--codon_ancestral: the chains kept no draw")
            codon_ancestral_pass(np.stack(kept))
    return post


def parse(arg):
    tree = dataio.read_tree(arg.tree)
    # phylostan.py:140-141: a root with more than two children is rerooted at
    # its first child's edge (run resolves polytomies instead, :175; for a
    # trifurcating root, e.g. DS1's, both give the same shape and numbering)
    if len(tree.seed_node.child_nodes()) > 2:
        tree.reroot_at_edge(tree.seed_node.child_nodes()[0].edge)
    dataio.setup_indexes(tree)
    dataio.setup_dates(tree, arg.dates, arg.heterochronous)
    stan_io.convert_samples_to_nexus(tree, arg.samples, arg.output, arg.rate)
    stan_io.parse_log(arg.samples, arg.alpha, tree)


def run_command(arg):
    """``run`` from the command line: ``--codon`` on the device's K-state sequence engine."""
    if getattr(arg, "codon", False):
        from .kseq import DeviceKStateLikelihood, DeviceKStateMixLikelihood, DeviceKStateSummaries
        mix = bool(getattr(arg, "codon_sites", None))
        lik = DeviceKStateMixLikelihood if mix else DeviceKStateLikelihood
        if getattr(arg, "codon_ancestral", False):
            return run(arg, likelihood_factory=lik, codon_summary_factory=DeviceKStateSummaries)
        return run(arg, likelihood_factory=lik)  # without the flag the call is what it was
    return run(arg)


def main(argv=None):
    parser = argparse.ArgumentParser(prog="phylostan", description="Phylogenetic inference on MI355X "
                                     "(GPU pruning likelihood, Stan runtime removed)")
    sub = parser.add_subparsers()
    create_build_parser(sub, "build", "build a model script").set_defaults(func=build)
    create_run_parser(sub).set_defaults(func=run_command)
    create_parse_parser(sub).set_defaults(func=parse)
    arg = parser.parse_args(argv)
    if not hasattr(arg, "func"):
        parser.print_help()
        return 1
    arg.func(arg)
    return 0


if __name__ == "__main__":
    sys.exit(main())
