#!/usr/bin/env python3
"""lattice-depth on the MI355X path: latbin/lattice-depth.cc:28-87 (CompactLatticeDepth, lat/lattice-functions.cc:574-602).

  lattice-depth [options] <lattice-rspecifier> [<depth-wspecifier>]
   e.g.: lattice-depth ark:- ark,t:-

The plain command line is host arithmetic over the string lengths.  The sweep ([MI355X] options, not the reference's):
what steps/oracle_wer.sh runs once per pruning beam,

  lattice-prune --acoustic-scale=$acwt --beam=$beam ark:lats ark:- | lattice-depth ark:- ark,t:depth_$beam.txt

is one command that reads the archive once and takes the depth of every pruned point from the device call that also finds
the oracle path (csrc/kh_latoracle.hip):

  lattice-depth --acoustic-scale=$acwt --beams=2,4,6,8 ark:lats [ark,t:depth_BEAM.txt]

BEAM in the wspecifier stands for the beam as it was typed.  A lattice of which nothing survives has depth 1 over 0
frames, as the reference's empty lattice."""
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from tools.lattice_oracle import cxx_ratio        # noqa: E402
kt = importlib.import_module("old-kaldi-git_amd.kaldi_tool")

PROG = "lattice-depth"
USAGE = ("Compute the lattice depths in terms of the average number of arcs that\n"
         "cross a frame.  See also lattice-depth-per-frame\n"
         "Usage: lattice-depth <lattice-rspecifier> [<depth-wspecifier>]\n"
         "E.g.: lattice-depth ark:- ark,t:-\n")


def main(argv=None):
    return kt.run_tool(PROG, run, argv, kt.KALDI_KH, assert_status=134)          # KALDI_ASSERT aborts


def run(cli, argv):
    def register(po):
        po.register("acoustic-scale", 1.0, "[MI355X] with --beams: as lattice-prune --acoustic-scale in front of this program", float)
        po.register("beams", "", "[MI355X] sweep: first:last or a comma list; each value as lattice-prune --beam in front of this "
                    "program, BEAM in the wspecifier stands for it", str)
        po.register("batch-arcs", 2000000, "[MI355X] lattice arcs per device call", int)
        po.register("gpu", 0, "[MI355X] device ordinal", int)
    po = kt.parse(cli, PROG, USAGE, argv, register, range(1, 3))               # :48
    if po is None:
        return 1
    sweep = po["beams"] != ""
    beams, (specs,), tag = kt.beam_sweep(cli, po, (po.get_opt_arg(2),))
    K = len(beams)
    reader = cli.SequentialTableReader(po.get_arg(1), "compact_lattice")
    writers = [cli.TableWriter(s, "base_float") for s in specs]
    api = importlib.import_module("old-kaldi-git_amd.api")
    if sweep:
        api.select_gpu(po["gpu"])
    point = api.score_point(acoustic_scale=po["acoustic-scale"])
    num_done = 0                                                               # :59
    sum_depth, total_t = [0.0] * K, [0.0] * K                                  # :60

    def account(p, key, depth, t):
        writers[p].write(key, np.float32(depth))                               # :70-71
        sum_depth[p] += float(np.float32(depth) * np.float32(t))               # :73 (a float product)
        total_t[p] += t                                                        # :74

    def lattices():
        """The plain command line accounts for a lattice as it is read; the sweep's lattices go on to the device call."""
        nonlocal num_done
        for key, clat in reader:
            num_done += 1                                                      # :75
            if not sweep:
                depth, t = api.compact_lattice_depth(clat)                     # :65-68
                account(0, key, depth, t)
                continue
            yield key, clat

    for batch in kt.batches(lattices(), lambda b: len(b[1]["arc_src"]), po["batch-arcs"], "after"):
        res = api.compact_lattice_oracle([c for _, c in batch], [[] for _ in batch], (), points=[point], beams=[float(b) for b in beams])
        for (key, _), row in zip(batch, res):
            for p, r in enumerate(row):
                account(p, key, r["depth"], r["num_frames"])
    for w in writers:
        w.close()
    cli.log("Done %d lattices." % num_done)                                    # :77
    for p in range(K):
        # steps/oracle_wer.sh parses the next line by field number
        cli.log("%sOverall density is %s over %g frames." % (tag(p), cxx_ratio(sum_depth[p], total_t[p]), total_t[p]))   # :79-80
    return 0 if num_done != 0 else 1                                           # :81-82


if __name__ == "__main__":
    sys.exit(main())
