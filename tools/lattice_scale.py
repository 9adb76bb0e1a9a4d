#!/usr/bin/env python3
"""lattice-scale: latbin/lattice-scale.cc:28-96.  Host only (a scale is two multiplications per weight and the archive is
read and written once); the batched search over many scales at once is lattice-best-path's sweep (tools/lattice_best_path.py).

  lattice-scale [options] lattice-rspecifier lattice-wspecifier
   e.g.: lattice-scale --lm-scale=0.0 ark:1.lats ark:scaled.lats

CompactLattices in and out."""
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
kt = importlib.import_module("old-kaldi-git_amd.kaldi_tool")

PROG = "lattice-scale"
USAGE = ("Apply scaling to lattice weights\n"
         "Usage: lattice-scale [options] lattice-rspecifier lattice-wspecifier\n"
         " e.g.: lattice-scale --lm-scale=0.0 ark:1.lats ark:scaled.lats\n")


def scale_matrix(lm_scale, acoustic_scale, inv_acoustic_scale, acoustic2lm_scale, lm2acoustic_scale):
    """:72-82: the options are floats, the matrix holds doubles; with --inv-acoustic-scale the acoustic scale is the FLOAT
    quotient 1.0 / inv."""
    ac, inv = np.float32(acoustic_scale), np.float32(inv_acoustic_scale)
    if not (ac == np.float32(1.0) or inv == np.float32(1.0)):
        raise AssertionError("KALDI_ASSERT: at main:lattice-scale.cc:72, failed: acoustic_scale == 1.0 || inv_acoustic_scale == 1.0")
    if inv != np.float32(1.0):
        ac = np.float32(1.0) / inv
    return np.array([[np.float32(lm_scale), np.float32(acoustic2lm_scale)], [np.float32(lm2acoustic_scale), ac]], np.float64)


def scale_weights(scale, g, a):
    """ScaleTupleWeight fstext/lattice-weight.h:233-241 on arrays: Zero (value1 == +inf) stays Zero, else the products and
    the sum in double, narrowed to float."""
    g, a = np.asarray(g, np.float32), np.asarray(a, np.float32)
    zero = g == np.float32(np.inf)
    g64, a64 = np.where(zero, 0.0, g.astype(np.float64)), np.where(zero, 0.0, a.astype(np.float64))
    with np.errstate(invalid="ignore", over="ignore"):
        g2 = (scale[0, 0] * g64 + scale[0, 1] * a64).astype(np.float32)
        a2 = (scale[1, 0] * g64 + scale[1, 1] * a64).astype(np.float32)
    inf = np.float32(np.inf)
    return np.where(zero, inf, g2).astype(np.float32), np.where(zero, inf, a2).astype(np.float32)


def scale_compact_lattice(scale, clat):
    """ScaleLattice (fstext/lattice-utils-inl.h) on the dict layout of kaldi_io.read_compact_lattice: arcs and final weights."""
    out = dict(clat)
    out["arc_g"], out["arc_a"] = scale_weights(scale, clat["arc_g"], clat["arc_a"])
    out["final_g"], out["final_a"] = scale_weights(scale, clat["final_g"], clat["final_a"])
    return out


def main(argv=None):
    return kt.run_tool(PROG, run, argv, kt.KALDI, assert_status=134)             # KALDI_ASSERT aborts


def run(cli, argv):
    def register(po):
        po.register("acoustic-scale", 1.0, "Scaling factor for acoustic likelihoods", float)
        po.register("inv-acoustic-scale", 1.0, "An alternative way of setting the acoustic scale: you can set its inverse.", float)
        po.register("lm-scale", 1.0, "Scaling factor for graph/lm costs", float)
        po.register("acoustic2lm-scale", 0.0, "Add this times original acoustic costs to LM costs", float)
        po.register("lm2acoustic-scale", 0.0, "Add this times original LM costs to acoustic costs", float)
    po = kt.parse(cli, PROG, USAGE, argv, register, 2)
    if po is None:
        return 1
    reader = cli.SequentialTableReader(po.get_arg(1), "compact_lattice")
    writer = cli.TableWriter(po.get_arg(2), "compact_lattice")
    scale = scale_matrix(po["lm-scale"], po["acoustic-scale"], po["inv-acoustic-scale"], po["acoustic2lm-scale"],
                         po["lm2acoustic-scale"])
    n_done = 0
    for key, clat in reader:
        writer.write(key, scale_compact_lattice(scale, clat))
        n_done += 1
    writer.close()
    cli.log("Done %d lattices." % n_done)
    return 0 if n_done != 0 else 1


if __name__ == "__main__":
    sys.exit(main())
