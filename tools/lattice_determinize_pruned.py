#!/usr/bin/env python3
"""lattice-determinize-pruned: latbin/lattice-determinize-pruned.cc:27-119 over api.determinize_lattices (word-level
determinization only, as DeterminizeLatticePruned: phone_determinize=False, word_determinize=True).  Host code: the
determinizer is the library's host implementation (csrc/kh_determinize.hip), one lattice per host thread.

  lattice-determinize-pruned [options] lattice-rspecifier lattice-wspecifier
   e.g.: lattice-determinize-pruned --acoustic-scale=0.1 --beam=6.0 ark:in.lats ark:det.lats

The table may hold Lattices or CompactLattices (SequentialLatticeReader); CompactLattices are written.  Every lattice is
scaled by AcousticLatticeScale(acoustic_scale), determinized with the beam, and scaled back by 1.0 / acoustic_scale - the
double quotient of the float option, as the C++ expression forms it.

Differences from the binary.  The library's determinizer carries a final weight as one cost (the decoder's lattices have
no acoustic cost on a final weight): a final acoustic cost that is not zero is folded, scaled, into the graph side, with one
warning per run.  --max-loop is accepted at 0 (the binary's default) and refused otherwise: the library has no loop
detection to bound.  Warnings of a batch of lattices come when the batch is done."""
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from tools.lattice_scale import scale_weights   # noqa: E402
kt = importlib.import_module("old-kaldi-git_amd.kaldi_tool")

PROG = "lattice-determinize-pruned"
USAGE = ("Determinize lattices, keeping only the best path (sequence of acoustic states)\n"
         "for each input-symbol sequence.  This version does pruning as part of the\n"
         "determinization algorithm, which is more efficient and prevents blowup.\n"
         "See http://kaldi.sourceforge.net/lattices.html for more information on lattices.\n"
         "\n"
         "Usage: lattice-determinize-pruned [options] lattice-rspecifier lattice-wspecifier\n"
         " e.g.: lattice-determinize-pruned --acoustic-scale=0.1 --beam=6.0 ark:in.lats ark:det.lats\n")
BATCH = 64      # lattices handed to the host threads at a time


def acoustic_scale_matrix(s):
    return np.array([[1.0, 0.0], [0.0, float(s)]], np.float64)


def scaled_input(L, scale, warned, warn):
    """The Lattice dict as the determinizer takes it: acoustic costs scaled (ScaleLattice, :88), the start state numbered 0,
    a final weight as one cost."""
    n = int(L["num_states"]) if "num_states" in L else len(L["state_final"])
    out = dict(L)
    out["arc_g"], out["arc_a"] = scale_weights(scale, L["arc_g"], L["arc_a"])
    if "state_final_graph" in L:
        fg, fa = scale_weights(scale, L["state_final_graph"], L["state_final_acoustic"])
        if np.any((fg != np.inf) & (fa != 0.0)) and not warned[0]:
            warned[0] = True
            warn("a final weight has an acoustic cost: it is folded into the graph cost of the determinized final weight")
        with np.errstate(invalid="ignore"):
            out["state_final"] = np.where(fg == np.inf, np.float32(np.inf), fg + fa).astype(np.float32)
    else:
        out["state_final"] = np.asarray(L["state_final"], np.float32)
    start = int(L.get("start", 0))
    if n > 0 and start > 0:           # the library takes state 0 as the start state: exchange the two numbers
        p = np.arange(n)
        p[0], p[start] = start, 0
        out["arc_src"], out["arc_dst"] = p[np.asarray(L["arc_src"], np.int64)].astype(np.int32), p[np.asarray(L["arc_dst"], np.int64)].astype(np.int32)
        out["state_final"] = out["state_final"][p]
        out["start"] = 0
    return out


def main(argv=None):
    return kt.run_tool(PROG, run, argv, kt.KALDI_KH)


def run(cli, argv):
    def register(po):
        po.register("acoustic-scale", 1.0, "Scaling factor for acoustic likelihoods", float)
        po.register("beam", 10.0, "Pruning beam [applied after acoustic scaling].", float)
        po.register("minimize", False, "If true, push and minimize after determinization")
        po.register("delta", 2.0 ** -10, "Tolerance used in determinization", float)
        po.register("max-mem", 50000000, "Maximum approximate memory usage in determinization (real usage might be many times this)", int)
        po.register("max-loop", 0, "Option used to detect a particular type of determinization failure, typically due to invalid input "
                    "(e.g., negative-cost loops) [MI355X: only 0 is supported]", int)
        po.register("num-threads", 0, "[MI355X] host threads (0: as many as the process may use)", int)
    po = kt.parse(cli, PROG, USAGE, argv, register, 2)
    if po is None:
        return 1
    if po["max-loop"] != 0:
        raise cli.KaldiError("--max-loop=%d: the library's determinizer has no loop detection; only --max-loop=0 is supported" % po["max-loop"])
    reader = cli.SequentialTableReader(po.get_arg(1), "any_lattice")
    writer = cli.TableWriter(po.get_arg(2), "compact_lattice")
    acoustic_scale = np.float32(po["acoustic-scale"])
    if acoustic_scale == np.float32(0.0):
        raise cli.KaldiError("Do not use a zero acoustic scale (cannot be inverted)")
    scale = acoustic_scale_matrix(acoustic_scale)
    unscale = acoustic_scale_matrix(1.0 / float(acoustic_scale))          # ":106 1.0/acoustic_scale": a double
    api = importlib.import_module("old-kaldi-git_amd.api")
    n = dict(done=0, warn=0)
    warned = [False]

    def flush(batch):
        dets = api.determinize_lattices([scaled_input(L, scale, warned, cli.warn) for _, L in batch], float(np.float32(po["beam"])),
                                        float(np.float32(po["delta"])), int(po["max-mem"]), po["num-threads"],
                                        phone_determinize=False, word_determinize=True, minimize=bool(po["minimize"]))
        for (key, _), det in zip(batch, dets):
            if not det["complete"]:
                cli.warn("For key %s, determinization did not succeed(partial output will be pruned tighter than the specified beam.)" % key)
                n["warn"] += 1
            det["arc_g"], det["arc_a"] = scale_weights(unscale, det["arc_g"], det["arc_a"])
            det["final_g"], det["final_a"] = scale_weights(unscale, det["final_g"], det["final_a"])
            writer.write(key, det)
            n["done"] += 1

    for batch in kt.batches(reader, lambda b: 1, BATCH, "after"):
        flush(batch)
    writer.close()
    cli.log("Done %d lattices, determinization finished earlier than specified by the beam on %d of these." % (n["done"], n["warn"]))
    return 0 if n["done"] != 0 else 1


if __name__ == "__main__":
    sys.exit(main())
