#!/usr/bin/env python3
"""acc-tree-stats on the MI355X path: bin/acc-tree-stats.cc's command line over the library, so that the accumulation line
of steps/train_deltas.sh (and of train_lda_mllt.sh, train_sat.sh, train_quick.sh ...) runs with the binary's options and
arguments.  (There is no bin/ shim for it yet: tests/test_cli_surface.py pins bin/ to the recorded
tests/golden/cli_surface.json, and the shim comes with the change that re-records it.)

  acc-tree-stats $context_opts --ci-phones=$ciphonelist $alidir/final.mdl "$feats" \\
    "ark:gunzip -c $alidir/ali.JOB.gz|" $dir/JOB.treeacc
  sum-tree-stats $dir/treeacc $dir/*.treeacc

The usage, the six options, the optional fourth argument (standard output without it), the warnings, the counts on stderr
and the exit status are the binary's (acc-tree-stats.cc:34-161): an utterance without an alignment is counted and not warned
about; an alignment of another length is a warning and a failure; an alignment SplitToPhones finds bad is a warning and
still counted as done; the file is written even when nothing was done, and the status is then 1.  Only the transition model
is read from the model file.  The file is WriteBuildTreeStats' (kaldi_io.write_tree_stats), the events in std::map order, and
sum-tree-stats, cluster-phones, compile-questions and build-tree read it.

The events are worked out on the host per utterance (api.tree_stats_frame_events); the sums are the library's
(csrc/kh_tree.hip): per (event, column) one chain of double adds over the event's frames in the order the binary meets them,
from the running value, so the file is the binary's byte for byte and does not depend on how the job is cut into passes.
Differences from the binary.  The utterances are read in batches of at most --batch-frames stacked rows (not a reference
option; default 200000; an utterance that would take a batch over the figure starts the next one) and ONE library pass is
made per batch.  --gpu (not a reference option): device ordinal, -1 = LOCAL_RANK, else 0.  --world / --rank (not reference
options): rank r is the recipe's JOB r + 1 and every JOB in the arguments becomes r + 1 (run.pl JOB=1:$nj); the statistics
file must then carry JOB in its name."""
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
kt = importlib.import_module("old-kaldi-git_amd.kaldi_tool")

PROG = "acc-tree-stats"
USAGE = ("Accumulate statistics for phonetic-context tree building.\n"
         "Usage:  acc-tree-stats [options] model-in features-rspecifier alignments-rspecifier [tree-accs-out]\n"
         "e.g.: \n"
         " acc-tree-stats 1.mdl scp:train.scp ark:1.ali 1.tacc\n")
BATCH_FRAMES = 200000


def main(argv=None):
    return kt.run_tool(PROG, run, argv, kt.KALDI_KH)


def run(cli, argv):
    def register(po):
        po.register("binary", True, "Write output in binary mode")
        po.register("var-floor", 0.01, "Variance floor for tree clustering.", float)
        po.register("ci-phones", "", "Colon-separated list of integer indices of context-independent phones (after mapping, if "
                    "--phone-map option is used).")
        po.register("context-width", 3, "Context window size.", int)
        po.register("central-position", 1, "Central context-window position (zero-based)", int)
        po.register("phone-map", "", "File name containing old->new phone mapping (each line is: old-integer-id new-integer-id)")
        po.register("batch-frames", BATCH_FRAMES, "[MI355X] stacked rows per library pass", int)
        kt.register_gpu(po)
        kt.register_ranks(po)
    argv, rank, world, raw_pos = kt.rank_substitute(argv)
    po = kt.parse(cli, PROG, USAGE, argv, register, range(3, 5))
    if po is None:
        return 1
    if world > 1 and (len(raw_pos) < 4 or "JOB" not in raw_pos[3]):
        raise cli.KaldiError("--world=%d: the statistics file needs JOB in its name (JOB.treeacc), or the ranks overwrite each other" % world)
    kio = importlib.import_module("old-kaldi-git_amd.kaldi_io")
    api = importlib.import_module("old-kaldi-git_amd.api")
    phone_map = None
    if po["phone-map"] != "":
        rx = po["phone-map"]
        name = "standard input" if rx in ("", "-") else rx               # PrintableRxfilename
        try:
            f, kind = cli.open_input(rx)
        except cli.KaldiError:
            raise cli.KaldiError("Error reading phone map from " + name)
        try:
            phone_map = kio.read_phone_map(f.read(), name)
        finally:
            if kind != "stdin":
                f.close()
    ci_phones = api.tree_stats_ci_phones(po["ci-phones"])
    N, P = po["context-width"], po["central-position"]
    tm = cli.read_kaldi_object(po.get_arg(1), kio.read_transition_model)      # the rest of the file is discarded
    tables = api.tree_stats_tables(tm)
    n_tids = len(tm["tid2pdf"]) - 1
    feature_reader = cli.SequentialTableReader(po.get_arg(2), "matrix")
    alignment_reader = cli.RandomAccessTableReader(po.get_arg(3), "int32_vector")
    n = dict(done=0, no_ali=0, other=0)
    state = dict(stats=None, gpu=False, dim=None)

    def flush(batch):
        """One library pass over the batch's stacked rows, on from the running statistics."""
        if not state["gpu"]:
            kt.select_gpu(api, po)
            state["gpu"] = True
        x = kt.stack_rows([b["mat"] for b in batch])
        if state["stats"] is None:
            state["stats"] = api.TreeStats(x.shape[1], po["var-floor"])
        # the utterances' event tables joined, the frames' indices moved behind one another: no tuple per frame
        starts = np.cumsum([0] + [len(b["table"]) for b in batch])
        state["stats"].accumulate(x, [ev for b in batch for ev in b["table"]],
                                  codes=np.concatenate([b["code"] + int(k) for b, k in zip(batch, starts)]))
        t = api.tree_last_timings()
        cli.vlog(1, "batch of %d rows in %d utterances: %d events, the longest %d frames" % (x.shape[0], len(batch), t["events"], t["longest"]))

    def utterances():
        for key, mat in feature_reader:
            if not alignment_reader.has_key(key):
                n["no_ali"] += 1
                continue
            ali = np.asarray(alignment_reader.value(key), np.int64)
            if len(ali) != mat.shape[0]:
                cli.warn("Alignments has wrong size %d vs. %d" % (len(ali), mat.shape[0]))
                n["other"] += 1
                continue
            kt.check_transition_ids(cli, key, ali, n_tids)
            ok, table, code = api.tree_stats_frame_events(tm, ali, N, P, ci_phones, phone_map, tables=tables, codes=True)
            if not ok:
                cli.warn("AccumulateTreeStats: alignment appears to be bad, not using it", "AccumulateTreeStats()")
            n["done"] += 1
            if n["done"] % 1000 == 0:
                cli.log("Processed %d utterances." % n["done"])
            if ok and mat.shape[0] != 0:
                if state["dim"] is None:
                    state["dim"] = mat.shape[1]
                if mat.shape[1] != state["dim"]:              # an event met at both dimensions: AddVec's assertion
                    raise cli.KaldiError("utterance %s: features of dimension %d after %d" % (key, mat.shape[1], state["dim"]))
                yield dict(mat=mat, table=table, code=code)

    for batch in kt.batches(utterances(), lambda b: b["mat"].shape[0], po["batch-frames"], "before"):
        flush(batch)
    stats = [] if state["stats"] is None else list(state["stats"].items())
    cli.write_kaldi_object(po.get_opt_arg(4), po["binary"], lambda f: kio.write_tree_stats(f, stats, po["binary"]))
    cli.log("Accumulated stats for %d files, %d failed due to no alignment, %d failed for other reasons." % (n["done"], n["no_ali"], n["other"]))
    cli.log("Number of separate stats (context-dependent states) is %d" % len(stats))
    return 0 if n["done"] != 0 else 1


if __name__ == "__main__":
    sys.exit(main())
