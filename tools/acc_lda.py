#!/usr/bin/env python3
"""acc-lda on the MI355X path: bin/acc-lda.cc's command line over the library, so that the accumulation line of
steps/train_lda_mllt.sh (and of steps/nnet2/get_lda.sh) runs unchanged with bin/ in front of PATH:

  ali-to-post "ark:gunzip -c $alidir/ali.JOB.gz|" ark:- | weight-silence-post 0.0 $silphonelist $alidir/final.mdl ark:- ark:- | \\
    acc-lda --rand-prune=$randprune $alidir/final.mdl "$splicedfeats" ark,s,cs:- $dir/lda.JOB.acc
  est-lda --dim=$dim $dir/0.mat $dir/lda.*.acc

The usage, options, warnings, counts on stderr and exit status are the binary's (acc-lda.cc:32-127): the accumulator takes
its sizes at the first utterance that has posteriors; a posterior of the wrong length and features of another dimension
both count as failures; the file is written even when nothing was done, and the status is then 1.  Only the transition
model is read from the model file.  The file is LdaEstimate::Write's (kaldi_io.write_lda_accs) and est-lda, which stays the
reference's, reads it.

Differences from the binary.  The utterances are read in batches of at most --batch-frames stacked rows (not a reference
option; default 200000; an utterance that would take a batch over the figure starts the next one) and ONE library pass is
made per batch (api.accumulate_lda_stats with the batch's utterances as segments), each running on from the accumulators of
the batches before: the library's sum tree is per utterance, then the utterances in order (csrc/kh_lda.hip), so the file
does not depend on --batch-frames.  It is not the reference's frame-by-frame rank-one updates.  A frame's entries are in
ascending pdf order (api.convert_posterior_to_pdfs), where the reference's order is its unordered_map's.  RandPrune runs on
the host over the batch's weights strictly in utterance, frame, entry order, batch after batch, with the C library's
rand().  The reference binary never seeds; here every batch positions the generator itself - srand(1), the state of a
process that never seeded, then the draws of the batches before discarded (api.rand_prune_at) - because the HIP runtime
reseeds the C library's generator when it initialises and draws from it at some first uses.
--gpu (not a reference option): device ordinal, -1 = LOCAL_RANK, else 0.  --world / --rank (not reference options): rank r
is the recipe's JOB r + 1 and every JOB in the arguments becomes r + 1 (run.pl JOB=1:$nj)."""
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
kt = importlib.import_module("old-kaldi-git_amd.kaldi_tool")

PROG = "acc-lda"
USAGE = ("Accumulate LDA statistics based on pdf-ids.\n"
         "Usage:  acc-lda [options] <transition-gmm/model> <features-rspecifier> <posteriors-rspecifier> <lda-acc-out>\n"
         "Typical usage:\n"
         " ali-to-post ark:1.ali ark:- | lda-acc 1.mdl \"ark:splice-feats scp:train.scp|\"  ark:- ldaacc.1\n")
BATCH_FRAMES = 200000


def main(argv=None):
    return kt.run_tool(PROG, run, argv, kt.KALDI_KH)


def run(cli, argv):
    def register(po):
        po.register("binary", True, "Write accumulators in binary mode.")
        po.register("rand-prune", 0.0, "Randomized pruning threshold for posteriors", float)
        po.register("batch-frames", BATCH_FRAMES, "[MI355X] stacked rows per library pass", int)
        kt.register_gpu(po)
        kt.register_ranks(po)
    argv, rank, world, raw_pos = kt.rank_substitute(argv)
    po = kt.parse(cli, PROG, USAGE, argv, register, 4)
    if po is None:
        return 1
    if world > 1 and "JOB" not in raw_pos[3]:
        raise cli.KaldiError("--world=%d: the statistics file needs JOB in its name (lda.JOB.acc), or the ranks overwrite each other" % world)
    kio = importlib.import_module("old-kaldi-git_amd.kaldi_io")
    tm = cli.read_kaldi_object(po.get_arg(1), kio.read_transition_model)      # the rest of the file is discarded
    api = importlib.import_module("old-kaldi-git_amd.api")
    rand_prune = np.float32(po["rand-prune"])                            # BaseFloat rand_prune
    if not rand_prune >= 0:
        raise cli.KaldiError("KALDI_ASSERT: prune_thresh >= 0.0")
    tid2pdf = tm["tid2pdf"]
    n_tids = len(tid2pdf) - 1
    num_pdfs = int(tm["triples"][:, 2].max()) + 1                       # TransitionModel::NumPdfs()
    feature_reader = cli.SequentialTableReader(po.get_arg(2), "matrix")
    post_reader = cli.RandomAccessTableReader(po.get_arg(3), "posterior")
    n = dict(done=0, fail=0)
    state = dict(acc=None, dim=0, gpu=False)

    def flush(batch):
        """One library pass over the batch's stacked rows, its utterances as segments, on from the running accumulator."""
        if not state["gpu"]:
            kt.select_gpu(api, po)
            state["gpu"] = True
        x = kt.stack_rows([b["mat"] for b in batch])
        pdf_posts = [fr for b in batch for fr in b["pdf_post"]]
        state["acc"] = api.accumulate_lda_stats(x, pdf_posts, num_pdfs, rand_prune=float(rand_prune), seed=1, into=state["acc"],
                                                segments=np.cumsum([0] + [b["mat"].shape[0] for b in batch]))
        t = api.lda_last_timings()
        cli.vlog(1, "batch of %d rows / %d items in %d utterances, %d draws so far" % (x.shape[0], t["items"], len(batch), state["acc"]["draws"]))

    def utterances():
        for key, mat in feature_reader:
            if not post_reader.has_key(key):
                cli.warn("No posteriors for utterance " + key)
                n["fail"] += 1
                continue
            post = post_reader.value(key)
            if state["dim"] == 0:                                       # lda.Init(trans_model.NumPdfs(), feats.NumCols())
                state["dim"] = int(mat.shape[1])
            if mat.shape[0] != len(post):
                cli.warn("Posterior vs. feats size mismatch %d vs. %d" % (mat.shape[0], len(post)))
                n["fail"] += 1
                continue
            if state["dim"] != 0 and state["dim"] != mat.shape[1]:
                cli.warn("Feature dimension mismatch %d vs. %d" % (state["dim"], mat.shape[1]))
                n["fail"] += 1
                continue
            kt.check_transition_ids(cli, key, np.asarray([t for fr in post for t, _ in fr], np.int64), n_tids)
            n["done"] += 1
            if n["done"] % 100 == 0:
                cli.log("Done %d utterances." % n["done"])
            if mat.shape[0] == 0:
                continue
            yield dict(key=key, mat=mat, pdf_post=api.convert_posterior_to_pdfs(tid2pdf, post))

    for batch in kt.batches(utterances(), lambda b: b["mat"].shape[0], po["batch-frames"], "before"):
        flush(batch)
    cli.log("Done %d files, failed for %d" % (n["done"], n["fail"]))
    acc = state["acc"]
    if acc is None:                       # nothing accumulated: the accumulators of LdaEstimate::Init, if it was reached
        dim = state["dim"]
        nc = num_pdfs if dim else 0
        acc = dict(zero=np.zeros(nc), first=np.zeros((nc, dim)), second=np.zeros(dim * (dim + 1) // 2), dim=dim, num_classes=nc)
    # Output ko(acc_wxfilename, binary); lda.Write(ko.Stream(), binary)
    cli.write_kaldi_object(po.get_arg(4), po["binary"], lambda f: kio.write_lda_accs(f, acc, po["binary"]))
    cli.log("Written statistics.")
    return 0 if n["done"] != 0 else 1


if __name__ == "__main__":
    sys.exit(main())
