#!/usr/bin/env python3
"""lattice-best-path on the MI355X path: latbin/lattice-best-path.cc:28-137 over the library's batched
CompactLatticeShortestPath (csrc/kh_latbest.hip; lat/lattice-functions.cc:1043-1126).

  lattice-best-path [options]  lattice-rspecifier [ transcriptions-wspecifier [ alignments-wspecifier] ]
   e.g.: lattice-best-path --acoustic-scale=0.1 ark:1.lats ark:1.tra ark:1.ali

The sweep ([MI355X] options, not the reference's): what local/score.sh runs as 36 pipelines

  lattice-scale --inv-acoustic-scale=LMWT ark:lats ark:- | lattice-add-penalty --word-ins-penalty=$wip ark:- ark:- | \\
    lattice-best-path ark:- ark,t:scoring/penalty_$wip/LMWT.tra

is one command that reads the archive once and searches every batch of lattices once for all score points:

  lattice-best-path --inv-acoustic-scales=9:20 --word-ins-penalties=0.0,0.5,1.0 ark:lats ark,t:scoring/penalty_WIP/LMWT.tra

LMWT and WIP in the wspecifiers stand for the point's values as they were typed.  Every point's output is what the three
programs piped together write for it, byte for byte."""
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
kt = importlib.import_module("old-kaldi-git_amd.kaldi_tool")

PROG = "lattice-best-path"
USAGE = ("Generate 1-best path through lattices; output as transcriptions and alignments\n"
         "Note: if you want output as FSTs, use lattice-1best; if you want output\n"
         "with acoustic and LM scores, use lattice-1best | nbest-to-linear\n"
         "Usage: lattice-best-path [options]  lattice-rspecifier [ transcriptions-wspecifier [ alignments-wspecifier] ]\n"
         " e.g.: lattice-best-path --acoustic-scale=0.1 ark:1.lats ark:1.tra ark:1.ali\n")


def main(argv=None):
    return kt.run_tool(PROG, run, argv, kt.KALDI_KH)


def run(cli, argv):
    def register(po):
        po.register("acoustic-scale", 1.0, "Scaling factor for acoustic likelihoods", float)
        po.register("lm-scale", 1.0, "Scaling factor for LM probabilities. Note: the ratio acoustic-scale/lm-scale is all that matters.", float)
        po.register("word-symbol-table", "", "Symbol table for words [for debug output]", str)
        po.register("inv-acoustic-scales", "", "[MI355X] sweep: first:last or a comma list; each value as lattice-scale "
                    "--inv-acoustic-scale before the search, LMWT in the wspecifiers stands for it", str)
        po.register("word-ins-penalties", "", "[MI355X] sweep: a comma list; each value as lattice-add-penalty --word-ins-penalty "
                    "before the search, WIP in the wspecifiers stands for it", str)
        po.register("batch-arcs", 2000000, "[MI355X] lattice arcs per best-path call", int)
        po.register("gpu", 0, "[MI355X] device ordinal", int)
    po = kt.parse(cli, PROG, USAGE, argv, register, range(1, 4))
    if po is None:
        return 1
    api = importlib.import_module("old-kaldi-git_amd.api")
    sweep = po["inv-acoustic-scales"] != "" or po["word-ins-penalties"] != ""
    if sweep:
        if np.float32(po["acoustic-scale"]) != 1.0 or np.float32(po["lm-scale"]) != 1.0:
            raise cli.KaldiError("the sweep stands for lattice-scale | lattice-add-penalty | lattice-best-path with the last "
                                 "one's scales at 1.0: do not combine it with --acoustic-scale / --lm-scale")
        points, specs, tag = kt.score_sweep(cli, api, po, (2, 3))
    else:
        # fst::LatticeScale(lm_scale, acoustic_scale) :85 (the options are floats, the matrix holds doubles)
        points = [api.score_point(lm_scale=po["lm-scale"], acoustic_scale=po["acoustic-scale"])]
        specs = [(po.get_opt_arg(2), po.get_opt_arg(3))]
        tag = lambda p: ""
    K = len(points)
    reader = cli.SequentialTableReader(po.get_arg(1), "compact_lattice")
    word_w = [cli.TableWriter(s[0], "int32_vector") for s in specs]
    ali_w = [cli.TableWriter(s[1], "int32_vector") for s in specs]
    word_syms = cli.read_symbol_table(po["word-symbol-table"]) if po["word-symbol-table"] != "" else None
    api.select_gpu(po["gpu"])
    f32 = np.float32
    n_done, n_fail, n_frame = [0] * K, [0] * K, [0] * K
    tot_g, tot_a = [f32(0.0)] * K, [f32(0.0)] * K        # LatticeWeight::One() :79

    def fail(key, p):
        cli.warn("%sBest-path failed for key %s" % (tag(p), key))
        n_fail[p] += 1

    def flush(batch):
        res = api.compact_lattice_best_paths([c for _, c in batch], points)
        for (key, _), row in zip(batch, res):
            for p, r in enumerate(row):
                if r is None:
                    fail(key, p)
                    continue
                g, a = f32(r["graph_cost"]), f32(r["acoustic_cost"])
                msg = ("%sFor utterance %s, best cost %s + %s = %s over %d frames."
                       % (tag(p), key, cli._cxx_float(g), cli._cxx_float(a), cli._cxx_float(g + a), len(r["alignment"])))
                if sweep:
                    cli.vlog(1, msg)
                else:
                    cli.log(msg)
                word_w[p].write(key, r["words"])
                ali_w[p].write(key, r["alignment"])
                if word_syms is not None and (not sweep or cli.verbose_level() >= 1):
                    out = [key]
                    for w in r["words"]:
                        if int(w) not in word_syms:
                            raise cli.KaldiError("Word-id %d not in symbol table." % int(w))
                        out.append(word_syms[int(w)])
                    sys.stderr.write(tag(p) + " ".join(out) + " \n")
                n_done[p] += 1
                n_frame[p] += len(r["alignment"])
                tot_g[p] = tot_g[p] + g
                tot_a[p] = tot_a[p] + a

    def lattices():
        for key, clat in reader:
            if int(clat["n_states"]) == 0 or int(clat.get("start", 0)) < 0:      # :1055: no start state, empty best path
                for p in range(K):
                    fail(key, p)
                continue
            yield key, clat

    for batch in kt.batches(lattices(), lambda b: len(b[1]["arc_src"]), po["batch-arcs"], "after"):
        flush(batch)
    for w in word_w + ali_w:
        w.close()
    with np.errstate(divide="ignore", invalid="ignore"):
        for p in range(K):
            nf = f32(n_frame[p])
            cli.log("%sOverall score per frame is %s = %s [graph] + %s [acoustic] over %d frames."
                    % (tag(p), cli._cxx_float((tot_g[p] + tot_a[p]) / nf), cli._cxx_float(tot_g[p] / nf),
                       cli._cxx_float(tot_a[p] / nf), n_frame[p]))
            cli.log("%sDone %d lattices, failed for %d" % (tag(p), n_done[p], n_fail[p]))
    return 0 if all(n != 0 for n in n_done) else 1


if __name__ == "__main__":
    sys.exit(main())
