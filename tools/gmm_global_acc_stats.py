#!/usr/bin/env python3
"""gmm-global-acc-stats on the MI355X path: gmmbin/gmm-global-acc-stats.cc's command line over the library, so that the
accumulation line of steps/online/nnet2/train_diag_ubm.sh runs with the binary's options and arguments.  (There is no bin/
shim for it yet: tests/test_cli_surface.py pins bin/ to the recorded tests/golden/cli_surface.json, and the shim comes with
the change that re-records it.)

  gmm-global-acc-stats "--gselect=ark,s,cs:gunzip -c $dir/gselect.JOB.gz|" $dir/$x.dubm "$feats" $dir/$x.JOB.acc

The usage, the four options, every warning and count of gmm-global-acc-stats.cc:86-115 (no weights, weights of the wrong
dimension, no gselect information, gselect of the wrong size), the two closing log lines, the "Written accs" line and the exit
status (1 when nothing was done; the file is written either way) are the binary's.  The file is AccumDiagGmm::Write's
(kaldi_io.write_global_gmm_accs) and gmm-global-sum-accs / gmm-global-est read it.
The posteriors are the library's (csrc/kh_gselect.hip: LogLikelihoodsPreselect, ApplySoftMax in list order, Scale(weight));
the sums are kh_gmm_acc_stats' (csrc/kh_gmmacc.hip) on dense posterior rows: per Gaussian the frames in order in chunks, the
chunks in order, in double.  A frame of weight 0 is skipped.  The per-file likelihood is the binary's FLOAT running sum.
Differences from the binary.  A gselect list that names a Gaussian twice in one frame makes the utterance an error, with a
warning naming it (the binary would add both posteriors; gmm-gselect never writes such a list), and so does an empty list on a
frame that is used (the binary asserts).  A list is scored as the Gaussians it names; the binary's LogLikelihoodsPreselect
scores the range front ... front + size - 1 instead whenever back + 1 - front == size (diag-gmm.cc:575), also when the list is
not that range, which happens to a frame of a score-ordered list now and then.  The utterances are read in batches of at most --batch-frames stacked rows (not a
reference option; default 200000) with ONE library pass per batch, and the batches are added in double in batch order, as
the gmm-acc tools do: a sum's grouping, not its addends, depends on the figure.  --gpu (not a reference option): device ordinal,
-1 = LOCAL_RANK, else 0.  --world / --rank (not reference options): rank r is the recipe's JOB r + 1 and every JOB in the
arguments becomes r + 1 (run.pl JOB=1:$nj); the statistics file must then carry JOB in its name."""
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
kt = importlib.import_module("old-kaldi-git_amd.kaldi_tool")

PROG = "gmm-global-acc-stats"
USAGE = ("Accumulate stats for training a diagonal-covariance GMM.\n"
         "Usage:  gmm-global-acc-stats [options] <model-in> <feature-rspecifier> <stats-out>\n"
         "e.g.: gmm-global-acc-stats 1.mdl scp:train.scp 1.acc\n")
BATCH_FRAMES = 200000


def main(argv=None):
    return kt.run_tool(PROG, run, argv, kt.KALDI_KH)


def bad_list(lists, weights, num_gauss):
    """The first frame of an utterance whose list the library would refuse -> a description, or None."""
    for i, v in enumerate(lists):
        if weights is not None and weights[i] == 0.0:
            continue
        v = np.asarray(v)
        if len(v) == 0:
            return "frame %d has an empty list" % i
        if v.min() < 0 or v.max() >= num_gauss:
            return "frame %d lists Gaussian %d, the model has %d" % (i, int(v.max() if v.min() >= 0 else v.min()), num_gauss)
        if len(np.unique(v)) != len(v):
            u, c = np.unique(v, return_counts=True)
            return "frame %d lists Gaussian %d twice" % (i, int([g for g in v if c[np.searchsorted(u, g)] > 1][0]))
    return None


def run(cli, argv):
    def register(po):
        po.register("binary", True, "Write output in binary mode")
        po.register("update-flags", "mvw", "Which GMM parameters will be updated: subset of mvw.")
        po.register("gselect", "", "rspecifier for gselect objects to limit the #Gaussians accessed on each frame.")
        po.register("weights", "", "rspecifier for a vector of floats for each utterance, that's a per-frame weight.")
        po.register("batch-frames", BATCH_FRAMES, "[MI355X] stacked rows per library pass", int)
        kt.register_gpu(po)
        kt.register_ranks(po)
    argv, rank, world, raw_pos = kt.rank_substitute(argv)
    po = kt.parse(cli, PROG, USAGE, argv, register, 3)
    if po is None:
        return 1
    if world > 1 and (len(raw_pos) < 3 or "JOB" not in raw_pos[2]):
        raise cli.KaldiError("--world=%d: the statistics file needs JOB in its name (x.JOB.acc), or the ranks overwrite each other" % world)
    kio = importlib.import_module("old-kaldi-git_amd.kaldi_io")
    api = importlib.import_module("old-kaldi-git_amd.api")
    weights_m, mi, iv = cli.read_kaldi_object(po.get_arg(1), kio.read_diag_gmm)
    num_gauss, dim = mi.shape
    flags = api.gmm_flags(po["update-flags"])
    acc = dict(occ=np.zeros(num_gauss), mean_acc=np.zeros((num_gauss, dim)) if flags & 1 else None,
               var_acc=np.zeros((num_gauss, dim)) if flags & 2 else None, dim=dim, flags=flags)
    feature_reader = cli.SequentialTableReader(po.get_arg(2), "matrix")
    use_gselect, use_weights = po["gselect"] != "", po["weights"] != ""
    gselect_reader = cli.RandomAccessTableReader(po["gselect"], "int32_vector_vector") if use_gselect else None
    weights_reader = cli.RandomAccessTableReader(po["weights"], "vector") if use_weights else None
    tot = dict(like=0.0, weight=0.0, done=0, err=0)
    state = dict(gmm=None)

    def flush(batch):
        """One library pass over the batch's stacked rows, added to the running statistics in double; then per utterance the
        binary's float totals from the frames' likelihoods."""
        rows = [b for b in batch if b["mat"].shape[0]]
        if rows:
            if state["gmm"] is None:
                kt.select_gpu(api, po)
                state["gmm"] = api.diag_gmm(weights_m, mi, iv)
            x = kt.stack_rows([b["mat"] for b in rows])
            gsel = [v for b in rows for v in b["gselect"]] if use_gselect else None
            w = np.concatenate([b["weights"] for b in rows]).astype(np.float32) if use_weights else None
            res = api.accumulate_global_gmm_stats(state["gmm"], x, gsel, w, flags, into=acc)
            frame_like = res["frame_like"]
            cli.vlog(1, "batch of %d rows in %d utterances" % (x.shape[0], len(rows)))
        at = 0
        for b in batch:
            T = b["mat"].shape[0]
            file_like, file_weight = np.float32(0.0), np.float32(0.0)
            for i in range(T):
                weight = b["weights"][i] if use_weights else np.float32(1.0)
                if weight == 0.0:
                    continue
                file_weight = np.float32(file_weight + weight)
                file_like = np.float32(file_like + np.float32(weight * frame_like[at + i]))
            at += T
            with np.errstate(invalid="ignore", divide="ignore"):
                cli.vlog(2, "File '%s': Average likelihood = %s over %s frames." % (b["key"], kt.g(file_like / file_weight), kt.g(file_weight)))
            tot["like"] += float(file_like)
            tot["weight"] += float(file_weight)
            tot["done"] += 1

    def utterances():
        for key, mat in feature_reader:
            file_frames = mat.shape[0]
            w = gsel = None
            if use_weights:
                if not weights_reader.has_key(key):
                    cli.warn("No per-frame weights available for utterance " + key)
                    tot["err"] += 1
                    continue
                w = np.asarray(weights_reader.value(key), np.float32)
                if len(w) != file_frames:
                    cli.warn("Weights for utterance %s have wrong dim %d vs. %d" % (key, len(w), file_frames))
                    tot["err"] += 1
                    continue
            if use_gselect:
                if not gselect_reader.has_key(key):
                    cli.warn("No gselect information for utterance " + key)
                    tot["err"] += 1
                    continue
                gsel = gselect_reader.value(key)
                if len(gsel) != file_frames:
                    cli.warn("gselect information for utterance %s has wrong size %d vs. %d" % (key, len(gsel), file_frames))
                    tot["err"] += 1
                    continue
                bad = bad_list(gsel, w, num_gauss)
                if bad is not None:
                    cli.warn("gselect information for utterance %s cannot be used: %s" % (key, bad))
                    tot["err"] += 1
                    continue
            yield dict(key=key, mat=mat, weights=w, gselect=gsel)

    for batch in kt.batches(utterances(), lambda b: b["mat"].shape[0], po["batch-frames"], "before"):
        flush(batch)
    cli.log("Done %d files; %d with errors." % (tot["done"], tot["err"]))
    with np.errstate(invalid="ignore", divide="ignore"):
        cli.log("Overall likelihood per frame = %s over %s (weighted) frames." % (
            kt.g(np.float64(tot["like"]) / np.float64(tot["weight"])), kt.g(tot["weight"])))
    cli.write_kaldi_object(po.get_arg(3), po["binary"], lambda f: kio.write_global_gmm_accs(f, acc, po["binary"]))
    cli.log("Written accs to " + po.get_arg(3))
    return 0 if tot["done"] != 0 else 1


if __name__ == "__main__":
    sys.exit(main())
