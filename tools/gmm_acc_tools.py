#!/usr/bin/env python3
"""The E-step of GMM training on the MI355X path: the reference binaries' command lines over the library, so that these
lines of steps/train_mono.sh, train_deltas.sh, train_lda_mllt.sh and train_sat.sh run unchanged with bin/ in front of PATH:

  gmm-acc-stats-ali $dir/$x.mdl "$feats" "ark,s,cs:gunzip -c $dir/ali.JOB.gz|" $dir/$x.JOB.acc
  ali-to-post "ark:gunzip -c $dir/ali.JOB.gz|" ark:- | \\
    gmm-acc-stats-twofeats $dir/$x.mdl "$feats" "$sifeats" ark,s,cs:- $dir/$x.JOB.acc
  gmm-est $dir/$x.mdl "gmm-sum-accs - $dir/$x.*.acc |" $dir/$[$x+1].mdl

Programs and the sources they restate: gmm-acc-stats-ali (gmmbin/gmm-acc-stats-ali.cc), gmm-acc-stats
(gmmbin/gmm-acc-stats.cc), gmm-acc-stats-twofeats (gmmbin/gmm-acc-stats-twofeats.cc), gmm-sum-accs (gmmbin/gmm-sum-accs.cc):
their usage, options, warnings, counts on stderr and exit status.  The .acc file is the reference's to the byte
(kaldi_io.write_gmm_accs); gmm-est reads it.  gmm-sum-accs is host code and needs no device.

Differences from the binaries.  The accumulators read the utterances in batches of at most --batch-frames stacked rows (not
a reference option; default 200000: 32 MB of 40-dimensional features on the host and on the device, and about as much again
for the Gaussian posteriors of a 5-Gaussian-per-pdf model; an utterance that would take a batch over the figure starts the
next one, and only an utterance longer than the figure is a batch above it, alone) and make ONE library pass per batch
(api.accumulate_gmm_stats), added into the running accumulator in double, so the "Processed N utterances" lines come at the end of a batch.  A frame's
entries are in ascending pdf order (api.convert_posterior_to_pdfs), where the reference's order is its unordered_map's.
The sums: a Gaussian's statistics are added per chunk of kh_gmm_acc_chunk entries of its pdf in frame order and the chunks in
chunk order, then the batches in order - not the reference's frame-by-frame BLAS rank-one updates; the totals
(<total_like>, <total_frames>, the transition accumulators) are added entry by entry in double as the reference does, per
batch.  gmm-acc-stats-twofeats answers unequal row counts of the two feature matrices with the reference's warning (the
reference asserts first).
--gpu (not a reference option): device ordinal, -1 = LOCAL_RANK, else 0.  Run through the tools/<name>.py wrappers."""
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
kt = importlib.import_module("old-kaldi-git_amd.kaldi_tool")

USAGE = {
    "gmm-acc-stats-ali": ("Accumulate stats for GMM training.\n"
                          "Usage:  gmm-acc-stats-ali [options] <model-in> <feature-rspecifier> <alignments-rspecifier> <stats-out>\n"
                          "e.g.:\n gmm-acc-stats-ali 1.mdl scp:train.scp ark:1.ali 1.acc\n"),
    "gmm-acc-stats": ("Accumulate stats for GMM training (reading in posteriors).\n"
                      "Usage:  gmm-acc-stats [options] <model-in> <feature-rspecifier><posteriors-rspecifier> <stats-out>\n"
                      "e.g.: \n"
                      " gmm-acc-stats 1.mdl scp:train.scp ark:1.post 1.acc\n"),
    "gmm-acc-stats-twofeats": ("Accumulate stats for GMM training, computing posteriors with one set of features\n"
                               "but accumulating statistics with another.\n"
                               "First features are used to get posteriors, second to accumulate stats\n"
                               "Usage:  gmm-acc-stats-twofeats [options] <model-in> <feature1-rspecifier> <feature2-rspecifier> "
                               "<posteriors-rspecifier> <stats-out>\n"
                               "e.g.: \n"
                               " gmm-acc-stats-twofeats 1.mdl 1.ali scp:train.scp scp:train_new.scp ark:1.ali 1.acc\n"),
    "gmm-sum-accs": ("Sum multiple accumulated stats files for GMM training.\n"
                     "Usage: gmm-sum-accs [options] <stats-out> <stats-in1> <stats-in2> ...\n"
                     "E.g.: gmm-sum-accs 1.acc 1.1.acc 1.2.acc\n"),
}
BATCH_FRAMES = 200000


def main(argv=None, prog="gmm-acc-stats-ali"):
    return kt.run_tool(prog, lambda cli, argv: RUN[prog](cli, argv, prog), argv, kt.KALDI_KH)


# ---------------------------------------------------------------- gmm-acc-stats-ali, gmm-acc-stats, gmm-acc-stats-twofeats
def run_acc_stats(cli, argv, prog):
    ali, two = prog == "gmm-acc-stats-ali", prog == "gmm-acc-stats-twofeats"

    def register(po):
        po.register("binary", True, "Write output in binary mode")
        if prog == "gmm-acc-stats":
            po.register("update-flags", "mvwt", "Which GMM parameters will be updated: subset of mvwt.")
        po.register("batch-frames", BATCH_FRAMES, "[MI355X] stacked rows per library pass", int)
        kt.register_gpu(po)
    po = kt.parse(cli, prog, USAGE[prog], argv, register, 5 if two else 4)
    if po is None:
        return 1
    kio = importlib.import_module("old-kaldi-git_amd.kaldi_io")
    tm, am = kt.read_gmm_model(cli, kio, po.get_arg(1))
    api = importlib.import_module("old-kaldi-git_amd.api")
    flags = api.gmm_flags(po["update-flags"] if prog == "gmm-acc-stats" else api.kGmmAll)
    tid2pdf = tm["tid2pdf"]
    n_tids = len(tid2pdf) - 1
    feature_reader = cli.SequentialTableReader(po.get_arg(2), "matrix")
    feature2_reader = cli.RandomAccessTableReader(po.get_arg(3), "matrix") if two else None
    post_reader = cli.RandomAccessTableReader(po.get_arg(4 if two else 3), "int32_vector" if ali else "posterior")
    n = dict(done=0, err=0, no2nd=0, no_post=0)
    tot = dict(like=0.0, t=0 if ali else 0.0)
    state = dict(acc=None, new_dim=0, trans=np.zeros(n_tids + 1, np.float64))       # trans_model.InitStats

    def flush(batch):
        """One library pass over the batch's stacked rows, added into the running accumulator; then the per-file figures."""
        if "gmm" not in state:
            kt.select_gpu(api, po)
            state["gmm"] = kt.device_gmm(api, am)
        pdf_posts = [fr for b in batch for fr in b["pdf_post"]]
        x1 = kt.stack_rows([b["mat"] for b in batch])
        state["acc"], ent, like = api.accumulate_gmm_stats(state["gmm"], x1, pdf_posts=pdf_posts, flags=flags, into=state["acc"],
                                                           stats_feats=kt.stack_rows([b["mat2"] for b in batch]) if two else None,
                                                           return_entries=True)
        w = ent["weight"]
        lw = (like * w).astype(np.float32)                                      # log_like * weight, BaseFloat
        t = api.gmm_acc_last_timings()
        cli.vlog(1, "batch of %d rows / %d entries: accumulate %.3f ms (kernels %.3f ms), %d groups, %d chunks" % (
            x1.shape[0], len(w), t["call_ms"], t["kernels_ms"], t["groups"], t["chunks"]))
        t0 = 0
        for b in batch:
            e0, e1 = int(ent["feo"][t0]), int(ent["feo"][t0 + len(b["pdf_post"])])
            t0 += len(b["pdf_post"])
            like_file = kt.f32sum(like[e0:e1] if ali else lw[e0:e1])
            w_file = len(b["pdf_post"]) if ali else kt.f32sum(w[e0:e1])
            np.add.at(state["trans"], b["tids"], b["tid_w"].astype(np.float64))                 # (*stats)(tid) += prob, in order
            if two:
                kt.report_file_like(cli, tot, like_file, w_file, b["index"])
                continue
            tot["like"] += like_file
            tot["t"] += w_file
            if b["index"] % 50 == 0:
                with np.errstate(invalid="ignore", divide="ignore"):
                    avg = np.float32(like_file) / np.float32(w_file)
                cli.log("Processed %d utterances; for utterance %s avg. like is %s over %s frames." % (b["index"], b["key"], kt.g(avg), kt.g(w_file)))

    def utterances():
        for key, mat in feature_reader:
            if two and not feature2_reader.has_key(key):
                cli.warn("For utterance %s, second features not present." % key)
                n["no2nd"] += 1
                continue
            if not post_reader.has_key(key):
                if ali:
                    cli.warn("No alignment for utterance " + key)
                    n["err"] += 1
                elif two:
                    n["no_post"] += 1
                else:
                    cli.warn("Could not find posteriors for utterance " + key)
                    n["err"] += 1
                continue
            post = post_reader.value(key)
            mat2 = feature2_reader.value(key) if two else None
            if len(post) != mat.shape[0]:
                cli.warn(("Alignments has wrong size %d vs. %d" if ali else "Posteriors has wrong size %d vs. %d" if two
                          else "Posterior vector has wrong size %d vs. %d") % (len(post), mat.shape[0]))
                n["err"] += 1
                continue
            if two and mat2.shape[0] != mat.shape[0]:
                cli.warn("Features have mismatched numbers of frames %d vs. %d" % (mat.shape[0], mat2.shape[0]))
                n["err"] += 1
                continue
            n["done"] += 1
            if mat.shape[0] == 0:
                continue
            if mat.shape[1] != am["dim"]:
                raise cli.KaldiError("DiagGmm::ComponentLogLikelihood, dimension mismatch %d vs. %d" % (mat.shape[1], am["dim"]))
            if two:
                if state["new_dim"] == 0:
                    state["new_dim"] = mat2.shape[1]
                elif mat2.shape[1] != state["new_dim"]:
                    raise cli.KaldiError("second features of %s have dimension %d, the accumulators %d" % (key, mat2.shape[1], state["new_dim"]))
            if ali:
                tids = np.asarray(post, np.int64).reshape(-1)
                kt.check_transition_ids(cli, key, tids, n_tids)
                tid_w = np.ones(len(tids), np.float32)
                pdf_post = [[(int(p), 1.0)] for p in tid2pdf[tids]]
            else:
                tids = np.asarray([t for fr in post for t, _ in fr], np.int64)
                kt.check_transition_ids(cli, key, tids, n_tids)
                tid_w = np.asarray([x for fr in post for _, x in fr], np.float32)
                pdf_post = api.convert_posterior_to_pdfs(tid2pdf, post)
            yield dict(key=key, mat=mat, mat2=mat2, pdf_post=pdf_post, tids=tids, tid_w=tid_w, index=n["done"])

    for batch in kt.batches(utterances(), lambda b: b["mat"].shape[0], po["batch-frames"], "before"):
        flush(batch)
    new_dim = state["new_dim"]
    if two:
        cli.log("Done %d files, %d with no posteriors, %d with no second features, %d with other errors." % (
            n["done"], n["no_post"], n["no2nd"], n["err"]))
    else:
        cli.log("Done %d files, %d with errors." % (n["done"], n["err"]))
    cli.log("Overall avg like per frame (Gaussian only) = %s over %s frames." % (
        kt.g(tot["like"] / tot["t"] if tot["t"] else float("nan")), ("%d" % tot["t"]) if ali else kt.g(tot["t"])))
    acc = state["acc"]
    if acc is None:                       # nothing accumulated: the zero accumulators of Init (twofeats: never initialised)
        off = np.asarray(am["pdf_offsets"], np.int32)
        dim = new_dim if two else am["dim"]
        ng = int(off[-1])
        acc = dict(occ=np.zeros(ng), mean_acc=np.zeros((ng, dim)) if flags & 1 else None, var_acc=np.zeros((ng, dim)) if flags & 2 else None,
                   pdf_offsets=off, dim=dim, flags=flags, total_like=0.0, total_frames=0.0)
        if two and new_dim == 0:
            acc = dict(acc, pdf_offsets=np.zeros(1, np.int32))
    acc["transition_accs"] = state["trans"]
    # Output ko(accs_wxfilename, binary); transition_accs.Write; gmm_accs.Write
    cli.write_kaldi_object(po.get_arg(5 if two else 4), po["binary"], lambda f: kio.write_gmm_accs(f, acc, po["binary"]))
    cli.log("Written accs.")
    return 0 if n["done"] != 0 else 1


# ---------------------------------------------------------------- gmm-sum-accs
def run_sum_accs(cli, argv, prog):
    po = kt.parse(cli, prog, USAGE[prog], argv, lambda po: po.register("binary", True, "Write output in binary mode"), lambda n: n >= 2)
    if po is None:
        return 1
    kio = importlib.import_module("old-kaldi-git_amd.kaldi_io")
    acc = None
    for i in range(2, po.num_args() + 1):
        acc = cli.read_kaldi_object(po.get_arg(i), lambda s, b: kio.read_gmm_accs(s, b, add_into=acc))
    cli.write_kaldi_object(po.get_arg(1), po["binary"], lambda f: kio.write_gmm_accs(f, acc, po["binary"]))
    count = np.float32(acc["total_frames"])                          # BaseFloat TotCount()
    with np.errstate(invalid="ignore", divide="ignore"):
        avg = np.float32(acc["total_like"]) / count
    cli.log("Summed %d stats, total count %s, avg like/frame %s" % (po.num_args() - 1, kt.g(count), kt.g(avg)))
    cli.log("Total count of stats is %s" % kt.g(np.float32(acc["occ"].sum())))
    cli.log("Written stats to " + po.get_arg(1))
    return 0


RUN = {"gmm-acc-stats-ali": run_acc_stats, "gmm-acc-stats": run_acc_stats, "gmm-acc-stats-twofeats": run_acc_stats,
       "gmm-sum-accs": run_sum_accs}
