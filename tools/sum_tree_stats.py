#!/usr/bin/env python3
"""sum-tree-stats: bin/sum-tree-stats.cc's command line, host only: the files are read in argument order
(kaldi_io.read_tree_stats) into a map over the events; the first clusterable met for an event is kept - with its count, its
variance floor and its sums - and every later one is added to it as GaussClusterable::Add does (the count and AddMat(1.0),
in double); the map is written in std::map<EventType> order (kaldi_io.write_tree_stats).  Usage, option, log line and exit
status are the binary's: 1 when the sum holds no event."""
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
kt = importlib.import_module("old-kaldi-git_amd.kaldi_tool")

PROG = "sum-tree-stats"
USAGE = ("Sum statistics for phonetic-context tree building.\n"
         "Usage:  sum-tree-stats [options] tree-accs-out tree-accs-in1 tree-accs-in2 ...\n"
         "e.g.: \n"
         " sum-tree-stats treeacc 1.treeacc 2.treeacc 3.treeacc\n")


def main(argv=None):
    return kt.run_tool(PROG, run, argv, kt.KALDI)


def merge(tree_stats, stats_array):
    """The loop of sum-tree-stats.cc:61-72 over one file's [(event, clusterable)]."""
    for event, c in stats_array:
        if event not in tree_stats:                           # not already present: the pointer itself, NULL included
            tree_stats[event] = None if c is None else dict(count=c["count"], var_floor=c["var_floor"], stats=np.array(c["stats"], np.float64))
            continue
        have = tree_stats[event]
        if have is None or c is None:                         # map_iter->second->Add(*c) through a NULL pointer
            raise ValueError("sum-tree-stats: event %r has no statistics in one of the files" % (event,))
        if have["stats"].shape != c["stats"].shape:
            raise ValueError("KALDI_ASSERT: at AddMat:kaldi-matrix.cc, failed: A.num_rows_ == num_rows_ && A.num_cols_ == num_cols_")
        have["count"] += c["count"]
        have["stats"] += c["stats"]
    return tree_stats


def run(cli, argv):
    po = kt.parse(cli, PROG, USAGE, argv, lambda po: po.register("binary", True, "Write output in binary mode"), lambda n: n >= 2)
    if po is None:
        return 1
    kio = importlib.import_module("old-kaldi-git_amd.kaldi_io")
    tree_stats = {}
    for i in range(2, po.num_args() + 1):
        merge(tree_stats, cli.read_kaldi_object(po.get_arg(i), kio.read_tree_stats))
    stats = [(event, tree_stats[event]) for event in sorted(tree_stats)]
    cli.write_kaldi_object(po.get_arg(1), po["binary"], lambda f: kio.write_tree_stats(f, stats, po["binary"]))
    cli.log("Wrote summed accs ( %d individual stats)" % len(stats))
    return 0 if len(stats) != 0 else 1                        # DeleteBuildTreeStats frees the objects, the vector keeps its size


if __name__ == "__main__":
    sys.exit(main())
