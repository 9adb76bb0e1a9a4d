"""What the command-line tools (tools/*.py behind bin/) share, in the order a tool uses it: the entry wrapper, option
parsing, the rank of a multi-rank job, the device and the model on it, batching, the score-point sweeps, the likelihood
report.  Small functions, no framework: a tool's run() still reads top to bottom like the reference binary's main().
Writing an object file is kaldi_cli.write_kaldi_object.  INTEGRATION.md "Writing a command-line tool" walks through them."""
import importlib
import os
import sys

import numpy as np

from . import capi
from . import kaldi_cli as cli

# What a tool's main() turns into "ERROR (prog) message", status 255 - the binaries' "catch(const std::exception &e) {
# std::cerr << e.what(); return -1; }".  The tools differ in it (DESIGN.md "Command line": a known divergence).
KALDI = (cli.KaldiError, ValueError)
KALDI_KH = KALDI + (capi.KhError,)


# ---------------------------------------------------------------- entry
def run_tool(prog, run, argv, catch, assert_status=None, on_error=None):
    """main() of a tool: run(cli, [prog] + arguments) -> exit status.  An exception of `catch` becomes the ERROR line and
    255 (on_error() after the line); with assert_status an AssertionError becomes its bare message and that status
    (KALDI_ASSERT aborts: 134); the pipe helper is stopped however run() ends."""
    argv = [prog] + list(sys.argv[1:] if argv is None else argv)
    try:
        return run(cli, argv)
    except catch as e:
        sys.stderr.write("ERROR (%s) %s\n" % (prog, e))
        if on_error is not None:
            on_error()
        return 255
    except AssertionError as e:
        if assert_status is None:
            raise
        sys.stderr.write("%s\n" % e)
        return assert_status
    finally:
        cli.stop_pipe_helper()


# ---------------------------------------------------------------- options
GPU_DOC = "[MI355X] device ordinal; -1: LOCAL_RANK, else 0"
WORLD_DOC = ("[MI355X] number of ranks sharing the job (default: WORLD_SIZE, else 1).  Rank r is the recipe's JOB r + 1: "
             "every JOB in the arguments becomes r + 1 (run.pl JOB=1:$nj)")
RANK_DOC = "[MI355X] this process's rank (default: RANK, else 0)"


def register_gpu(po, doc=GPU_DOC):
    """--gpu with the -1 = LOCAL_RANK default (select_gpu below).  print_usage prints the text: a tool with another
    wording passes its own."""
    po.register("gpu", -1, doc, int)


def register_ranks(po, world_doc=WORLD_DOC):
    po.register("world", 0, world_doc, int)
    po.register("rank", -1, RANK_DOC, int)


def parse(cli, prog, usage, argv, register, n_args):
    """The head of every run(): the pipe helper BEFORE anything can initialise the GPU, register(po), the command line, the
    number of arguments (an int, a range or a predicate).  None: the usage was printed, return 1."""
    cli.start_pipe_helper()
    po = cli.ParseOptions(usage)
    if register is not None:
        register(po)
    po.read(argv)
    cli.set_program_name(prog)
    n = po.num_args()
    if not (n == n_args if isinstance(n_args, int) else n in n_args if isinstance(n_args, range) else n_args(n)):
        po.print_usage()
        return None
    return po


# ---------------------------------------------------------------- ranks
def rank_substitute(argv):
    """--world / --rank looked at before the options are parsed, because run.pl replaces JOB in the WHOLE command line
    (options too): -> (argv with every JOB replaced by rank + 1 when world > 1, rank, world, the positional arguments as
    typed - the tool checks that its outputs carried JOB).  Called in front of parse()."""
    cli.start_pipe_helper()               # the helper is forked before sharding brings torch in
    sharding = importlib.import_module(__package__ + ".sharding")
    w_opt = r_opt = None
    for a in argv[1:]:
        if a.startswith("--world="):
            w_opt = int(a.split("=", 1)[1])
        elif a.startswith("--rank="):
            r_opt = int(a.split("=", 1)[1])
    rank, world = sharding.tool_ranks(w_opt or 0, -1 if r_opt is None else r_opt)
    raw_positional = [a for a in argv[1:] if not a.startswith("--")]
    if world > 1:
        argv = [argv[0]] + sharding.job_substitute(argv[1:], rank)
    return argv, rank, world, raw_positional


# ---------------------------------------------------------------- device and model
def select_gpu(api, po):
    """--gpu, -1: the launcher's LOCAL_RANK, else 0."""
    api.select_gpu(po["gpu"] if po["gpu"] >= 0 else int(os.environ.get("LOCAL_RANK", "0")))


def read_gmm_model(cli, kio, rx):
    """`trans_model.Read; am_gmm.Read` of a .mdl -> (transition model, AmDiagGmm on the host)."""
    return cli.read_kaldi_object(rx, lambda s, b: (kio.read_transition_model(s, b), kio.read_am_diag_gmm(s, b)))


def device_gmm(api, am):
    """The host AmDiagGmm on the device, with the gconsts DiagGmm::Read computes."""
    gconsts, _ = api.gmm_compute_gconsts(am["weights"], am["means_invvars"], am["inv_vars"])
    return api.AmDiagGmm(gconsts, am["means_invvars"], am["inv_vars"], am["pdf_offsets"])


def stack_rows(mats, dim=None):
    """The matrices stacked into one float32 device tensor; with dim, no matrix at all is [0, dim]."""
    import torch
    if not mats and dim is not None:
        return torch.from_numpy(np.zeros((0, dim), np.float32)).cuda()
    return torch.from_numpy(np.ascontiguousarray(np.concatenate(mats, 0), dtype=np.float32)).cuda()


def check_transition_ids(cli, key, tids, n_tids):
    if len(tids) and (tids.min() < 1 or tids.max() > n_tids):
        raise cli.KaldiError("utterance %s: transition-id %d, the model has 1 .. %d" % (
            key, int(tids.max() if tids.min() >= 1 else tids.min()), n_tids))


# ---------------------------------------------------------------- batching
def batches(items, size, limit, rule):
    """The items of a tool's own generator (it tests has_key, warns and skips) in batches of about `limit`, measured by
    size(item); the last, partial batch comes at the end.  rule "after": a batch closes once it has reached the limit
    (the lattice tools' --batch-arcs, --batch-frames of the decoders); rule "before": it closes before the item that would
    take it over (the accumulators' --batch-frames; a longer item is a batch alone).  An item is pulled, with its
    warnings, before the batch in front of it is closed by "before" and after it is closed by "after"."""
    assert rule in ("after", "before")
    batch, total = [], 0
    for item in items:
        n = size(item)
        if rule == "before" and batch and total + n > limit:
            yield batch
            batch, total = [], 0
        batch.append(item)
        total += n
        if rule == "after" and total >= limit:
            yield batch
            batch, total = [], 0
    if batch:
        yield batch


# ---------------------------------------------------------------- sweeps
def parse_sweep_list(text, what):
    """"9:20" (integers, both ends included) or "9,10.5,12" -> the tokens as typed."""
    text = text.strip()
    if ":" in text:
        lo, _, hi = text.partition(":")
        try:
            lo, hi = int(lo), int(hi)
        except ValueError:
            raise ValueError("Invalid %s range %r (expected first:last, integers)" % (what, text))
        if hi < lo:
            raise ValueError("Invalid %s range %r (empty)" % (what, text))
        return [str(v) for v in range(lo, hi + 1)]
    toks = [t.strip() for t in text.split(",")]
    for t in toks:
        try:
            float(t)
        except ValueError:
            raise ValueError("Invalid %s list %r" % (what, text))
    return toks


def substitute(wspecifier, lmwt, wip):
    return wspecifier.replace("LMWT", lmwt).replace("WIP", wip)


def score_sweep(cli, api, po, args, what="wspecifiers"):
    """--inv-acoustic-scales x --word-ins-penalties of the scoring tools: None without either, else (points [one
    api.score_point per (LMWT, WIP)], specs [per point the positional arguments `args` with LMWT / WIP replaced by the
    values as typed], tag [point -> the prefix of its log lines]).  An output named alike for two points is an error."""
    if po["inv-acoustic-scales"] == "" and po["word-ins-penalties"] == "":
        return None
    lmwts = parse_sweep_list(po["inv-acoustic-scales"], "--inv-acoustic-scales") if po["inv-acoustic-scales"] else ["1"]
    wips = parse_sweep_list(po["word-ins-penalties"], "--word-ins-penalties") if po["word-ins-penalties"] else ["0.0"]
    names = [(l, w) for w in wips for l in lmwts]
    points = [api.score_point(inv_acoustic_scale=float(l), word_ins_penalty=float(w)) for l, w in names]
    specs = [tuple(substitute(po.get_opt_arg(k), l, w) for k in args) for l, w in names]
    for k in range(len(args)):
        used = [s[k] for s in specs if s[k] != ""]
        if len(set(used)) != len(used):
            raise cli.KaldiError("the sweep's %s must differ per point (use LMWT and WIP in them): %s" % (what, used[0]))
    return points, specs, lambda p: "[LMWT=%s WIP=%s] " % names[p]


def beam_specs(spec, beams):
    return [spec.replace("BEAM", b) for b in beams]


def beam_sweep(cli, po, specs):
    """--beams with --acoustic-scale of lattice-oracle / lattice-depth (lattice-prune in front of them): -> (beams as
    typed, or [None] without the option; per spec its names per beam; tag)."""
    if po["beams"] == "":
        if np.float32(po["acoustic-scale"]) != 1.0:
            raise cli.KaldiError("--acoustic-scale belongs to the sweep: give --beams with it")
        return [None], [[s] for s in specs], lambda p: ""
    beams = parse_sweep_list(po["beams"], "--beams")
    for b in beams:
        if not np.float32(float(b)) > 0.0:                                     # KALDI_ASSERT(beam > 0.0), PruneLattice :192
            raise AssertionError("KALDI_ASSERT: at PruneLattice:lattice-functions.cc:192, failed: beam > 0.0")
    if np.float32(po["acoustic-scale"]) == 0.0:
        raise cli.KaldiError("Do not use a zero acoustic scale (cannot be inverted)")
    for spec in specs:
        if spec != "" and len(set(beam_specs(spec, beams))) != len(beams):
            raise cli.KaldiError("the sweep's wspecifiers must differ per point (use BEAM in them): %s" % spec)
    return beams, [beam_specs(s, beams) for s in specs], lambda p: "[BEAM=%s] " % beams[p]


# ---------------------------------------------------------------- likelihood report
def g(x):
    return "%g" % x


def f32sum(a):
    """BaseFloat += BaseFloat over the entries in order."""
    return float(np.cumsum(a, dtype=np.float32)[-1]) if len(a) else 0.0


def report_file_like(cli, tot, like_file, w_file, index):
    """The per-file lines of gmm-acc-mllt / gmm-acc-stats-twofeats: "Average like for this file", the totals, and every
    tenth file the running average."""
    with np.errstate(invalid="ignore", divide="ignore"):
        avg = np.float32(like_file) / np.float32(w_file)
    cli.log("Average like for this file is %s over %s frames." % (g(avg), g(w_file)))
    tot["like"] += like_file
    tot["t"] += w_file
    if index % 10 == 0:
        cli.log("Avg like per frame so far is " + g(tot["like"] / tot["t"] if tot["t"] else float("nan")))
