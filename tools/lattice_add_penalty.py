#!/usr/bin/env python3
"""lattice-add-penalty: latbin/lattice-add-penalty.cc:26-68 (AddWordInsPenToCompactLattice, lat/lattice-functions.cc:1128-1149).
Host only.

  lattice-add-penalty [options] <lattice-rspecifier> <lattice-wspecifier>
   e.g.: lattice-add-penalty --word-ins-penalty=1.0 ark:- ark:-

CompactLattices in and out."""
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
kt = importlib.import_module("old-kaldi-git_amd.kaldi_tool")

PROG = "lattice-add-penalty"
USAGE = ("Add word insertion penalty to the lattice.\n"
         "Note: penalties are negative log-probs, base e, and are added to the\n"
         "'language model' part of the cost.\n"
         "\n"
         "Usage: lattice-add-penalty [options] <lattice-rspecifier> <lattice-wspecifier>\n"
         " e.g.: lattice-add-penalty --word-ins-penalty=1.0 ark:- ark:-\n")


def add_word_ins_pen(penalty, clat):
    """:1140-1143: value1 + penalty in float on every arc with a word; final weights are not touched."""
    out = dict(clat)
    g = np.asarray(clat["arc_g"], np.float32)
    word = np.asarray(clat["arc_label"]) != 0
    out["arc_g"] = np.where(word, g + np.float32(penalty), g).astype(np.float32)
    return out


def main(argv=None):
    return kt.run_tool(PROG, run, argv, kt.KALDI)


def run(cli, argv):
    po = kt.parse(cli, PROG, USAGE, argv, lambda po: po.register("word-ins-penalty", 0.0, "Word insertion penalty", float), 2)
    if po is None:
        return 1
    reader = cli.SequentialTableReader(po.get_arg(1), "compact_lattice")
    writer = cli.TableWriter(po.get_arg(2), "compact_lattice")
    n_done = 0
    for key, clat in reader:
        writer.write(key, add_word_ins_pen(po["word-ins-penalty"], clat))
        n_done += 1
    writer.close()
    cli.log("Done adding word insertion penalty to %d lattices." % n_done)
    return 0 if n_done != 0 else 1


if __name__ == "__main__":
    sys.exit(main())
