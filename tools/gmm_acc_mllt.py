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
kt = importlib.import_module("old-kaldi-git_amd.kaldi_tool")

PROG = "gmm-acc-mllt"
USAGE = ("Accumulate MLLT (global STC) statistics\n"
         "Usage:  gmm-acc-mllt [options] <model-in> <feature-rspecifier> <posteriors-rspecifier> <stats-out>\n"
         "e.g.: \n"
         " gmm-acc-mllt 1.mdl scp:train.scp ark:1.post 1.macc\n")
BATCH_FRAMES = 200000


def main(argv=None):
    return kt.run_tool(PROG, run, argv, kt.KALDI_KH)


def run(cli, argv):
    def register(po):
        po.register("binary", True, "Write output in binary mode")
        po.register("rand-prune", 0.25, "Randomized pruning parameter to speed up accumulation (larger -> more pruning.  May exceed one).", float)
        po.register("batch-frames", BATCH_FRAMES, "[MI355X] stacked rows per library pass", int)
        kt.register_gpu(po)
        kt.register_ranks(po)
    argv, rank, world, raw_pos = kt.rank_substitute(argv)
    po = kt.parse(cli, PROG, USAGE, argv, register, 4)
    if po is None:
        return 1
    if world > 1 and "JOB" not in raw_pos[3]:
        raise cli.KaldiError("--world=%d: the statistics file needs JOB in its name ($x.JOB.macc), or the ranks overwrite each other" % world)
    kio = importlib.import_module("old-kaldi-git_amd.kaldi_io")
    tm, am = kt.read_gmm_model(cli, kio, po.get_arg(1))
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
        if "gmm" not in state:
            kt.select_gpu(api, po)
            state["gmm"] = kt.device_gmm(api, am)
        x = kt.stack_rows([b["mat"] for b in batch])
        pdf_posts = [fr for b in batch for fr in b["pdf_post"]]
        state["acc"], ent, like = api.accumulate_mllt_stats(state["gmm"], x, pdf_posts, rand_prune=float(rand_prune), seed=1, into=state["acc"],
                                                            return_entries=True,
                                                            segments=np.cumsum([0] + [b["mat"].shape[0] for b in batch]))
        w = ent["weight"]
        lw = (like * w).astype(np.float32)                                # AccumulateFromGmm(...) * weight, BaseFloat
        cli.vlog(1, "batch of %d rows / %d entries in %d utterances, %d draws so far" % (x.shape[0], len(w), len(batch), state["acc"]["draws"]))
        t0 = 0
        for b in batch:
            e0, e1 = int(ent["feo"][t0]), int(ent["feo"][t0 + len(b["pdf_post"])])
            t0 += len(b["pdf_post"])
            kt.report_file_like(cli, tot, kt.f32sum(lw[e0:e1]), kt.f32sum(w[e0:e1]), b["index"])

    def utterances():
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
                cli.log("Average like for this file is %s over %s frames." % (kt.g(float("nan")), kt.g(0.0)))
                continue
            if mat.shape[1] != am["dim"]:
                raise cli.KaldiError("DiagGmm::ComponentLogLikelihood, dimension mismatch %d vs. %d" % (mat.shape[1], am["dim"]))
            kt.check_transition_ids(cli, key, np.asarray([t for fr in post for t, _ in fr], np.int64), n_tids)
            yield dict(key=key, mat=mat, pdf_post=api.convert_posterior_to_pdfs(tid2pdf, post), index=n["done"])

    for batch in kt.batches(utterances(), lambda b: b["mat"].shape[0], po["batch-frames"], "before"):
        flush(batch)
    cli.log("Done %d files, %d with no posteriors, %d with other errors." % (n["done"], n["no_post"], n["err"]))
    cli.log("Overall avg like per frame (Gaussian only) = %s over %s frames." % (
        kt.g(tot["like"] / tot["t"] if tot["t"] else float("nan")), kt.g(tot["t"])))
    acc = state["acc"]
    if acc is None:                       # nothing accumulated: the zero accumulators of MlltAccs::Init
        dim = int(am["dim"])
        acc = dict(beta=0.0, G=np.zeros((dim, dim * (dim + 1) // 2)), dim=dim)
    # WriteKaldiObject(mllt_accs, accs_wxfilename, binary)
    cli.write_kaldi_object(po.get_arg(4), po["binary"], lambda f: kio.write_mllt_accs(f, acc, po["binary"]))
    cli.log("Written accs.")
    return 0 if n["done"] != 0 else 1


if __name__ == "__main__":
    sys.exit(main())
