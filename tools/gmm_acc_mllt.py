#!/usr/bin/env python3
"""gmm-acc-mllt on the MI355X path: gmmbin/gmm-acc-mllt.cc's command line over the library, so that the accumulation line of
steps/train_lda_mllt.sh runs unchanged with bin/ in front of PATH:

  ali-to-post "ark:gunzip -c $dir/ali.JOB.gz|" ark:- | weight-silence-post 0.0 $silphonelist $dir/$x.mdl ark:- ark:- | \\
    gmm-acc-mllt --rand-prune=$randprune $dir/$x.mdl "$feats" ark:- $dir/$x.JOB.macc
  est-mllt $dir/$x.mat.new $dir/$x.*.macc

The usage, options, warnings, counts on stderr and exit status are the binary's (gmm-acc-mllt.cc:33-121); the .macc file is
MlltAccs::Write's to the byte (kaldi_io.write_mllt_accs) and est-mllt, which stays the reference's, reads it.

Differences from the binary.  The utterances are read in batches of at most --batch-frames stacked rows (not a reference
option; default 200000; an utterance that would take a batch over the figure starts the next one) and ONE library pass is
made per batch (api.accumulate_mllt_stats: posteriors, pruning and transfers once; the accumulation per utterance, added
into the running accumulator in double utterance by utterance), so the "Average like" lines come at the end of a batch and
the file does not depend on --batch-frames.  A frame's entries are in ascending pdf order (api.convert_posterior_to_pdfs), where the reference's
order is its unordered_map's.  RandPrune runs on the host over the batch's Gaussian posteriors strictly in utterance, frame,
entry, Gaussian order, batch after batch, with the C library's rand().  The reference binary never seeds; here that is not
enough, because the HIP runtime reseeds the C library's generator when it initialises and draws from it at some first uses.
So every batch positions the generator itself - srand(1), the state of a process that never seeded, then the draws of the
batches before discarded (api.rand_prune_at) - and the job meets the sequence the reference binary draws.  The sums of G
are the library's slice tree's per utterance (csrc/kh_mllt.hip), then the utterances in order - not the reference's
frame-by-frame SpMatrix updates; beta is added entry by entry in double as there.
--gpu (not a reference option): device ordinal, -1 = LOCAL_RANK, else 0.  --world / --rank (not reference options): rank r
is the recipe's JOB r + 1 and every JOB in the arguments becomes r + 1 (run.pl JOB=1:$nj)."""
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

PROG = "gmm-acc-mllt"
USAGE = ("Accumulate MLLT (global STC) statistics\n"
         "Usage:  gmm-acc-mllt [options] <model-in> <feature-rspecifier> <posteriors-rspecifier> <stats-out>\n"
         "e.g.: \n"
         " gmm-acc-mllt 1.mdl scp:train.scp ark:1.post 1.macc\n")
BATCH_FRAMES = 200000


def _g(x):
    return "%g" % x


def main(argv=None):
    cli = importlib.import_module("old-kaldi-git_amd.kaldi_cli")
    capi = importlib.import_module("old-kaldi-git_amd.capi")
    argv = [PROG] + list(sys.argv[1:] if argv is None else argv)
    try:
        return run(cli, argv)
    except (cli.KaldiError, ValueError, capi.KhError) as e:     # "catch(const std::exception &e) { std::cerr << e.what(); return -1; }"
        sys.stderr.write("ERROR (%s) %s\n" % (PROG, e))
        return 255
    finally:
        cli.stop_pipe_helper()


def run(cli, argv):
    cli.start_pipe_helper()               # before anything initialises the GPU
    sharding = importlib.import_module("old-kaldi-git_amd.sharding")
    po = cli.ParseOptions(USAGE)
    po.register("binary", True, "Write output in binary mode")
    po.register("rand-prune", 0.25, "Randomized pruning parameter to speed up accumulation (larger -> more pruning.  May exceed one).", float)
    po.register("batch-frames", BATCH_FRAMES, "[MI355X] stacked rows per library pass", int)
    po.register("gpu", -1, "[MI355X] device ordinal; -1: LOCAL_RANK, else 0", int)
    po.register("world", 0, "[MI355X] number of ranks sharing the job (default: WORLD_SIZE, else 1).  Rank r is the recipe's JOB r + 1: "
                "every JOB in the arguments becomes r + 1 (run.pl JOB=1:$nj)", int)
    po.register("rank", -1, "[MI355X] this process's rank (default: RANK, else 0)", int)
    w_opt = r_opt = None
    for a in argv[1:]:
        if a.startswith("--world="):
            w_opt = int(a.split("=", 1)[1])
        elif a.startswith("--rank="):
            r_opt = int(a.split("=", 1)[1])
    rank, world = sharding.tool_ranks(w_opt or 0, -1 if r_opt is None else r_opt)
    raw_pos = [a for a in argv[1:] if not a.startswith("--")]
    if world > 1:
        argv = [argv[0]] + sharding.job_substitute(argv[1:], rank)
    po.read(argv)
    cli.set_program_name(PROG)
    if po.num_args() != 4:
        po.print_usage()
        return 1
    if world > 1 and "JOB" not in raw_pos[3]:
        raise cli.KaldiError("--world=%d: the statistics file needs JOB in its name ($x.JOB.macc), or the ranks overwrite each other" % world)
    kio = importlib.import_module("old-kaldi-git_amd.kaldi_io")
    tm, am = cli.read_kaldi_object(po.get_arg(1), lambda s, b: (kio.read_transition_model(s, b), kio.read_am_diag_gmm(s, b)))
    api = importlib.import_module("old-kaldi-git_amd.api")
    rand_prune = np.float32(po["rand-prune"])                            # BaseFloat rand_prune
    if not rand_prune >= 0:
        raise cli.KaldiError("KALDI_ASSERT: rand_prune_ >= 0.0")
    tid2pdf = tm["tid2pdf"]
    n_tids = len(tid2pdf) - 1
    feature_reader = cli.SequentialTableReader(po.get_arg(2), "matrix")
    post_reader = cli.RandomAccessTableReader(po.get_arg(3), "posterior")
    n = dict(done=0, no_post=0, err=0)
    tot = dict(like=0.0, t=0.0)
    state = dict(acc=None)

    def flush(batch):
        """One library pass over the batch's stacked rows, added into the running accumulator; then the per-file figures."""
        if not batch:
            return
        import torch
        if "gmm" not in state:
            api.select_gpu(po["gpu"] if po["gpu"] >= 0 else int(os.environ.get("LOCAL_RANK", "0")))
            gconsts, _ = api.gmm_compute_gconsts(am["weights"], am["means_invvars"], am["inv_vars"])
            state["gmm"] = api.AmDiagGmm(gconsts, am["means_invvars"], am["inv_vars"], am["pdf_offsets"])
        x = torch.from_numpy(np.ascontiguousarray(np.concatenate([b["mat"] for b in batch], 0), dtype=np.float32)).cuda()
        pdf_posts = [fr for b in batch for fr in b["pdf_post"]]
        state["acc"], ent, like = api.accumulate_mllt_stats(state["gmm"], x, pdf_posts, rand_prune=float(rand_prune), seed=1, into=state["acc"],
                                                            return_entries=True,
                                                            segments=np.cumsum([0] + [b["mat"].shape[0] for b in batch]))
        w = ent["weight"]
        lw = (like * w).astype(np.float32)                                # AccumulateFromGmm(...) * weight, BaseFloat
        cli.vlog(1, "batch of %d rows / %d entries in %d utterances, %d draws so far" % (x.shape[0], len(w), len(batch), state["acc"]["draws"]))
        t0 = 0
        f32sum = lambda a: float(np.cumsum(a, dtype=np.float32)[-1]) if len(a) else 0.0     # BaseFloat += BaseFloat, in order
        for b in batch:
            e0, e1 = int(ent["feo"][t0]), int(ent["feo"][t0 + len(b["pdf_post"])])
            t0 += len(b["pdf_post"])
            like_file, w_file = f32sum(lw[e0:e1]), f32sum(w[e0:e1])
            with np.errstate(invalid="ignore", divide="ignore"):
                avg = np.float32(like_file) / np.float32(w_file)
            cli.log("Average like for this file is %s over %s frames." % (_g(avg), _g(w_file)))
            tot["like"] += like_file
            tot["t"] += w_file
            if b["index"] % 10 == 0:
                cli.log("Avg like per frame so far is " + _g(tot["like"] / tot["t"] if tot["t"] else float("nan")))

    batch, frames = [], 0
    for key, mat in feature_reader:
        if not post_reader.has_key(key):
            n["no_post"] += 1
            continue
        post = post_reader.value(key)
        if len(post) != mat.shape[0]:
            cli.warn("Posterior vector has wrong size %d vs. %d" % (len(post), mat.shape[0]))
            n["err"] += 1
            continue
        n["done"] += 1
        if mat.shape[0] == 0:
            cli.log("Average like for this file is %s over %s frames." % (_g(float("nan")), _g(0.0)))
            continue
        if mat.shape[1] != am["dim"]:
            raise cli.KaldiError("DiagGmm::ComponentLogLikelihood, dimension mismatch %d vs. %d" % (mat.shape[1], am["dim"]))
        tids = np.asarray([t for fr in post for t, _ in fr], np.int64)
        if len(tids) and (tids.min() < 1 or tids.max() > n_tids):
            raise cli.KaldiError("utterance %s: transition-id %d, the model has 1 .. %d" % (
                key, int(tids.max() if tids.min() >= 1 else tids.min()), n_tids))
        pdf_post = api.convert_posterior_to_pdfs(tid2pdf, post)
        if batch and frames + mat.shape[0] > po["batch-frames"]:         # this utterance would take the batch over: it starts the next
            flush(batch)
            batch, frames = [], 0
        batch.append(dict(key=key, mat=mat, pdf_post=pdf_post, index=n["done"]))
        frames += mat.shape[0]
    flush(batch)
    cli.log("Done %d files, %d with no posteriors, %d with other errors." % (n["done"], n["no_post"], n["err"]))
    cli.log("Overall avg like per frame (Gaussian only) = %s over %s frames." % (
        _g(tot["like"] / tot["t"] if tot["t"] else float("nan")), _g(tot["t"])))
    acc = state["acc"]
    if acc is None:                       # nothing accumulated: the zero accumulators of MlltAccs::Init
        dim = int(am["dim"])
        acc = dict(beta=0.0, G=np.zeros((dim, dim * (dim + 1) // 2)), dim=dim)
    f, kind = cli.open_output(po.get_arg(4))          # WriteKaldiObject(mllt_accs, accs_wxfilename, binary)
    if po["binary"]:
        f.write(b"\0B")
    kio.write_mllt_accs(f, acc, po["binary"])
    if kind == "stdout":
        f.flush()
    elif f.close() not in (None, 0):
        raise cli.KaldiError("Error closing output stream " + po.get_arg(4))
    cli.log("Written accs.")
    return 0 if n["done"] != 0 else 1


if __name__ == "__main__":
    sys.exit(main())
