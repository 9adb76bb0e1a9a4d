#!/usr/bin/env python3
"""gmm-gselect on the MI355X path: gmmbin/gmm-gselect.cc's command line over the library, so that the selection line of
steps/online/nnet2/train_diag_ubm.sh (and of the SGMM and full-covariance UBM stages) runs with the binary's options and
arguments.  (There is no bin/ shim for it yet: tests/test_cli_surface.py pins bin/ to the recorded
tests/golden/cli_surface.json, and the shim comes with the change that re-records it.)

  gmm-gselect --n=$num_gselect $dir/0.dubm "$feats" "ark:|gzip -c >$dir/gselect.JOB.gz"

The usage, the three options, the "You asked for N Gaussians but GMM only has" warning and clamp, the missing-key and
wrong-size warnings counted as errors, the log line of every tenth file, the final line and the exit status (1 when nothing
was done) are the binary's (gmm-gselect.cc:32-135).  The lists are the library's (csrc/kh_gselect.hip, stated in
include/kaldi_hip.h): the n best Gaussians per frame under (score descending, index descending), which is what the binary's
nth_element / sort produce.  The per-utterance likelihood is a double sum of the frames' floats in the binary's grouping:
without --gselect the frames in order within a part of GaussianSelection's max_mem split (diag-gmm.cc:807-830) and the parts
in order; with --gselect a plain sum in frame order.
Differences from the binary.  The utterances are read in batches of at most --batch-frames stacked rows (not a reference
option; default 200000; an utterance that would take a batch over the figure starts the next one) and ONE library pass is made
per batch; the archive does not depend on the figure, byte for byte.  A frame with a NaN score (the binary's nth_element is
undefined there) is an error naming the utterance.  --gpu (not a reference option): device ordinal, -1 = LOCAL_RANK, else 0.
--world / --rank (not reference options): rank r is the recipe's JOB r + 1 and every JOB in the arguments becomes r + 1
(run.pl JOB=1:$nj); the gselect wspecifier must then carry JOB."""
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
kt = importlib.import_module("old-kaldi-git_amd.kaldi_tool")

PROG = "gmm-gselect"
USAGE = ("Precompute Gaussian indices for pruning\n"
         " (e.g. in training UBMs, SGMMs, tied-mixture systems)\n"
         " For each frame, gives a list of the n best Gaussian indices,\n"
         " sorted from best to worst.\n"
         "See also: gmm-global-get-post, fgmm-global-gselect-to-post,\n"
         "copy-gselect, fgmm-gselect\n"
         "Usage: gmm-gselect [options] <model-in> <feature-rspecifier> <gselect-wspecifier>\n"
         "The --gselect option (which takes an rspecifier) limits selection to a subset\n"
         "of indices:\n"
         "e.g.: gmm-gselect \"--gselect=ark:gunzip -c bigger.gselect.gz|\" --n=20 1.gmm \"ark:feature-command |\" \"ark,t:|gzip -c >gselect.1.gz\"\n")
BATCH_FRAMES = 200000
MAX_MEM = 10000000            # diag-gmm.cc:807


def like_in_parts(frame_like, num_gauss):
    """The double GaussianSelection(Matrix) returns: `ans += tot_loglike` within a part, `tot_ans += part` over the parts."""
    T = len(frame_like)
    mem = T * num_gauss * 4
    if mem <= MAX_MEM:
        bounds = [(0, T)]
    else:
        num_parts = (mem + MAX_MEM - 1) // MAX_MEM
        part = (T + num_parts - 1) // num_parts
        bounds = [(p * part, min(T, (p + 1) * part)) for p in range(num_parts) if p * part < T]
    tot = 0.0
    for a, b in bounds:
        ans = 0.0
        for v in frame_like[a:b]:
            ans += float(v)
        tot = ans if len(bounds) == 1 else tot + ans
    return tot


def main(argv=None):
    return kt.run_tool(PROG, run, argv, kt.KALDI_KH, assert_status=134)


def run(cli, argv):
    def register(po):
        po.register("n", 50, "Number of Gaussians to keep per frame\n", int)
        po.register("write-likes", "", "rspecifier for likelihoods per utterance")
        po.register("gselect", "", "rspecifier for gselect objects to limit the search to")
        po.register("batch-frames", BATCH_FRAMES, "[MI355X] stacked rows per library pass", int)
        kt.register_gpu(po)
        kt.register_ranks(po)
    argv, rank, world, raw_pos = kt.rank_substitute(argv)
    po = kt.parse(cli, PROG, USAGE, argv, register, 3)
    if po is None:
        return 1
    if world > 1 and (len(raw_pos) < 3 or "JOB" not in raw_pos[2]):
        raise cli.KaldiError("--world=%d: the gselect wspecifier needs JOB in its name (gselect.JOB.gz), or the ranks overwrite each other" % world)
    kio = importlib.import_module("old-kaldi-git_amd.kaldi_io")
    api = importlib.import_module("old-kaldi-git_amd.api")
    weights, mi, iv = cli.read_kaldi_object(po.get_arg(1), kio.read_diag_gmm)
    num_gselect = po["n"]
    if not num_gselect > 0:
        raise AssertionError("KALDI_ASSERT: at main:gmm-gselect.cc:66, failed: num_gselect > 0")
    num_gauss = len(weights)
    if num_gselect > num_gauss:
        cli.warn("You asked for %d Gaussians but GMM only has %d, returning this many. Note: this means the Gaussian selection "
                 "is pointless." % (num_gselect, num_gauss))
        num_gselect = num_gauss
    feature_reader = cli.SequentialTableReader(po.get_arg(2), "matrix")
    gselect_writer = cli.TableWriter(po.get_arg(3), "int32_vector_vector")
    use_pre = po["gselect"] != ""
    gselect_reader = cli.RandomAccessTableReader(po["gselect"], "int32_vector_vector") if use_pre else None
    likelihood_writer = cli.TableWriter(po["write-likes"], "base_float")
    tot = dict(like=0.0, t=0, done=0, err=0)
    state = dict(gmm=None)

    def finish(utt, lists, frame_like):
        """The tail of the binary's loop for one utterance."""
        T = len(lists)
        like = sum_plain(frame_like) if use_pre else like_in_parts(frame_like, num_gauss)
        gselect_writer.write(utt, lists)
        if tot["done"] % 10 == 0:
            with np.errstate(invalid="ignore", divide="ignore"):
                cli.log("For %d'th file, average UBM likelihood over %d frames is %s" % (tot["done"], T, kt.g(np.float64(like) / T)))
        tot["t"] += T
        tot["like"] += like
        if likelihood_writer.is_open():
            likelihood_writer.write(utt, like)
        tot["done"] += 1

    def sum_plain(frame_like):
        s = 0.0
        for v in frame_like:
            s += float(v)
        return s

    def flush(batch):
        """One library pass over the batch's stacked rows; an utterance without a frame writes an empty table entry."""
        rows = [b for b in batch if b["mat"].shape[0]]
        res = None
        if rows:
            if state["gmm"] is None:
                kt.select_gpu(api, po)
                state["gmm"] = api.diag_gmm(weights, mi, iv)
            x = kt.stack_rows([b["mat"] for b in rows])
            pre = [v for b in rows for v in b["pre"]] if use_pre else None
            res = api.gmm_gselect(state["gmm"], x, num_gselect, pre)
            t = api.gselect_last_timings()
            cli.vlog(1, "batch of %d rows in %d utterances: scores %.3f ms, selection %.3f ms" % (
                x.shape[0], len(rows), t["score_kernels_ms"], t["select_kernels_ms"]))
        at = 0
        for b in batch:
            T = b["mat"].shape[0]
            if T and res["status"][at:at + T].any():
                raise cli.KaldiError("utterance %s: frame %d has a score that is not a number" % (
                    b["key"], int(np.nonzero(res["status"][at:at + T])[0][0])))
            finish(b["key"], res["lists"][at:at + T] if T else [], res["frame_like"][at:at + T] if T else [])
            at += T

    def utterances():
        for utt, mat in feature_reader:
            pre = None
            if use_pre:
                if not gselect_reader.has_key(utt):
                    cli.warn("No gselect information for utterance " + utt)
                    tot["err"] += 1
                    continue
                pre = gselect_reader.value(utt)
                if len(pre) != mat.shape[0]:
                    cli.warn("Input gselect for utterance %s has wrong size %d vs. %d" % (utt, len(pre), mat.shape[0]))
                    tot["err"] += 1
                    continue
            yield dict(key=utt, mat=mat, pre=pre)

    for batch in kt.batches(utterances(), lambda b: b["mat"].shape[0], po["batch-frames"], "before"):
        flush(batch)
    ok = gselect_writer.close()
    likelihood_writer.close()
    with np.errstate(invalid="ignore", divide="ignore"):
        avg = np.float64(tot["like"]) / np.float64(tot["t"])
    cli.log("Done %d files, %d with errors, average UBM log-likelihood is %s over %d frames." % (tot["done"], tot["err"], kt.g(avg), tot["t"]))
    if not ok:
        raise cli.KaldiError("Error closing the gselect table " + po.get_arg(3))
    return 0 if tot["done"] != 0 else 1


if __name__ == "__main__":
    sys.exit(main())
