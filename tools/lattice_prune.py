#!/usr/bin/env python3
"""lattice-prune on the MI355X path: latbin/lattice-prune.cc:28-114 over the library's batched PruneLattice
(csrc/kh_latprune.hip; lat/lattice-functions.cc:186-265).

  lattice-prune [options] lattice-rspecifier lattice-wspecifier
   e.g.: lattice-prune --acoustic-scale=0.1 --beam=4.0 ark:1.lats ark:pruned.lats

The sweep ([MI355X] options, not the reference's): what the sclite-style scoring scripts (egs/tedlium/s5/local/score_sclite.sh
and its relatives) run once per grid point in front of lattice-align-words | lattice-to-ctm-conf,

  lattice-scale --inv-acoustic-scale=LMWT ark:lats ark:- | lattice-add-penalty --word-ins-penalty=$wip ark:- ark:- | \\
    lattice-prune --beam=$beam ark:- ark:pruned/penalty_$wip/LMWT.lats

is one command that reads the archive once and prunes every batch of lattices once for all score points:

  lattice-prune --inv-acoustic-scales=9:20 --word-ins-penalties=0.0,0.5,1.0 --beam=5 ark:lats ark:pruned/penalty_WIP/LMWT.lats

LMWT and WIP in the wspecifier stand for the point's values as they were typed.  Every point's output is what the three
programs piped together write for it, byte for byte."""
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from tools.lattice_add_penalty import add_word_ins_pen                   # noqa: E402
from tools.lattice_scale import scale_compact_lattice                     # noqa: E402
kt = importlib.import_module("old-kaldi-git_amd.kaldi_tool")

PROG = "lattice-prune"
USAGE = ("Apply beam pruning to lattices\n"
         "Usage: lattice-prune [options] lattice-rspecifier lattice-wspecifier\n"
         " e.g.: lattice-prune --acoustic-scale=0.1 --beam=4.0 ark:1.lats ark:pruned.lats\n")


def acoustic_lattice_scale(acwt):
    """fst::AcousticLatticeScale (fstext/lattice-utils.h): [[1, 0], [0, acwt]] in doubles."""
    return np.array([[1.0, 0.0], [0.0, np.float64(acwt)]], np.float64)


def plain_scale(acoustic_scale, inv_acoustic_scale):
    """:59-61, :75: the options are floats and the quotient is stored to a float."""
    ac, inv = np.float32(acoustic_scale), np.float32(inv_acoustic_scale)
    if not (ac == np.float32(1.0) or inv == np.float32(1.0)):
        raise AssertionError("KALDI_ASSERT: at main:lattice-prune.cc:59, failed: acoustic_scale == 1.0 || inv_acoustic_scale == 1.0")
    if inv != np.float32(1.0):
        ac = np.float32(1.0) / inv
    return ac


def pruned_subset(clat, r):
    """The states and arcs api.compact_lattice_prune kept (r: one of its dicts), carrying clat's weights and strings: what
    PruneLattice leaves of clat (:87)."""
    if not r["ok"]:
        z, f = np.zeros(0, np.int32), np.zeros(0, np.float32)
        return dict(n_states=0, start=-1, arc_src=z, arc_dst=z, arc_label=z, arc_g=f, arc_a=f, arc_string=[], final_g=f,
                    final_a=f, final_string=[], complete=True)
    ks, ka, kept = r["kept_states"], r["kept_arcs"], r["final_kept"]
    inf, empty = np.float32(np.inf), np.zeros(0, np.int32)
    return dict(n_states=r["n_states"], start=r["start"], arc_src=r["arc_src"], arc_dst=r["arc_dst"],
                arc_label=np.asarray(clat["arc_label"], np.int32)[ka], arc_g=np.asarray(clat["arc_g"], np.float32)[ka],
                arc_a=np.asarray(clat["arc_a"], np.float32)[ka], arc_string=[clat["arc_string"][j] for j in ka],
                final_g=np.where(kept, np.asarray(clat["final_g"], np.float32)[ks], inf).astype(np.float32),
                final_a=np.where(kept, np.asarray(clat["final_a"], np.float32)[ks], inf).astype(np.float32),
                final_string=[clat["final_string"][s] if k else empty for s, k in zip(ks, kept)], complete=True)


def main(argv=None):
    return kt.run_tool(PROG, run, argv, kt.KALDI_KH, assert_status=134)          # KALDI_ASSERT aborts


def run(cli, argv):
    def register(po):
        po.register("acoustic-scale", 1.0, "Scaling factor for acoustic likelihoods", float)
        po.register("inv-acoustic-scale", 1.0, "An alternative way of setting the acoustic scale: you can set its inverse.", float)
        po.register("beam", 10.0, "Pruning beam [applied after acoustic scaling]", float)
        po.register("inv-acoustic-scales", "", "[MI355X] sweep: first:last or a comma list; each value as lattice-scale "
                    "--inv-acoustic-scale before the pruning, LMWT in the wspecifier stands for it", str)
        po.register("word-ins-penalties", "", "[MI355X] sweep: a comma list; each value as lattice-add-penalty --word-ins-penalty "
                    "before the pruning, WIP in the wspecifier stands for it", str)
        po.register("batch-arcs", 2000000, "[MI355X] lattice arcs per pruning call", int)
        po.register("gpu", 0, "[MI355X] device ordinal", int)
    po = kt.parse(cli, PROG, USAGE, argv, register, 2)
    if po is None:
        return 1
    f32 = np.float32
    beam = f32(po["beam"])
    api = importlib.import_module("old-kaldi-git_amd.api")
    sweep = po["inv-acoustic-scales"] != "" or po["word-ins-penalties"] != ""
    identity = acoustic_lattice_scale(1.0)
    if sweep:
        if f32(po["acoustic-scale"]) != 1.0 or f32(po["inv-acoustic-scale"]) != 1.0:
            raise cli.KaldiError("the sweep stands for lattice-scale | lattice-add-penalty | lattice-prune with the last one's "
                                 "scale at 1.0: do not combine it with --acoustic-scale / --inv-acoustic-scale")
        points, specs, tag = kt.score_sweep(cli, api, po, (2,))
        specs = [s[0] for s in specs]
        there, back = identity, identity
    else:
        ac = plain_scale(po["acoustic-scale"], po["inv-acoustic-scale"])
        if ac == 0.0:                                                         # :75
            raise cli.KaldiError("Do not use a zero acoustic scale (cannot be inverted)")
        there = acoustic_lattice_scale(ac)                                    # :82
        with np.errstate(all="ignore"):
            back = acoustic_lattice_scale(np.float64(1.0) / np.float64(ac))   # :98: the double quotient
        points, specs, tag = [(there.reshape(4), f32(0.0))], [po.get_arg(2)], lambda p: ""
    if not beam > 0.0:                                                        # KALDI_ASSERT(beam > 0.0), PruneLattice :192
        raise AssertionError("KALDI_ASSERT: at PruneLattice:lattice-functions.cc:192, failed: beam > 0.0")
    K = len(points)
    reader = cli.SequentialTableReader(po.get_arg(1), "compact_lattice")
    writers = [cli.TableWriter(s, "compact_lattice") for s in specs]
    api.select_gpu(po["gpu"])
    n_done, n_err = 0, [0] * K
    n_arcs_in, n_states_in, n_arcs_out, n_states_out = 0, 0, [0] * K, [0] * K

    def flush(batch):
        nonlocal n_done, n_arcs_in, n_states_in
        res = api.compact_lattice_prune([c for _, c in batch], points, beam)
        for (key, clat), row in zip(batch, res):
            narcs, nstates = len(clat["arc_src"]), int(clat["n_states"])      # :83
            n_arcs_in += narcs
            n_states_in += nstates
            for p, r in enumerate(row):
                # what lattice-prune reads (the sweep: what the two programs in front of it wrote), scaled :82
                piped = clat if not sweep else add_word_ins_pen(points[p][1], scale_compact_lattice(points[p][0].reshape(2, 2), clat))
                pruned = pruned_subset(scale_compact_lattice(there, piped), r)
                if not r["ok"]:                                                # :87-90
                    cli.warn("%sError pruning lattice for utterance %s" % (tag(p), key))
                    n_err[p] += 1
                n_arcs_out[p] += len(pruned["arc_src"])                       # :91-94
                n_states_out[p] += pruned["n_states"]
                msg = ("%sFor utterance %s, pruned #states from %d to %d and #arcs from %d to %d"
                       % (tag(p), key, nstates, pruned["n_states"], narcs, len(pruned["arc_src"])))
                if sweep:
                    cli.vlog(1, msg)
                else:
                    cli.log(msg)                                              # :95-97
                writers[p].write(key, scale_compact_lattice(back, pruned))    # :98-99: every key is written
            n_done += 1                                                       # :100

    for batch in kt.batches(reader, lambda b: len(b[1]["arc_src"]), po["batch-arcs"], "after"):
        flush(batch)
    for w in writers:
        w.close()
    den = f32(n_done) if n_done > 0 else f32(1.0)                             # :103
    avg = lambda n: cli._cxx_float(f32(n) / den)
    for p in range(K):
        cli.log("%sOverall, pruned from on average %s to %s states, and from %s to %s arcs, over %d utterances."
                % (tag(p), avg(n_states_in), avg(n_states_out[p]), avg(n_arcs_in), avg(n_arcs_out[p]), n_done))   # :104-107
    cli.log("Done %d lattices." % n_done)                                     # :108
    return 0 if n_done != 0 else 1                                            # :109


if __name__ == "__main__":
    sys.exit(main())
