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

USAGE = ("Generate 1-best path through lattices; output as transcriptions and alignments\n"
         "Note: if you want output as FSTs, use lattice-1best; if you want output\n"
         "with acoustic and LM scores, use lattice-1best | nbest-to-linear\n"
         "Usage: lattice-best-path [options]  lattice-rspecifier [ transcriptions-wspecifier [ alignments-wspecifier] ]\n"
         " e.g.: lattice-best-path --acoustic-scale=0.1 ark:1.lats ark:1.tra ark:1.ali\n")


def parse_sweep_list(text, what):
    """"9:20" (integers, both ends included) or "9,10.5,12" -> the tokens as typed."""
    text = text.strip()
    if ":" in text:
        lo, _, hi = text.partition(":")
        try:
            lo, hi = int(lo), int(hi)
        except ValueError:
            raise ValueError("Invalid %s range %r (expected first:last, integers)" % (what, text))
        if hi < lo:
            raise ValueError("Invalid %s range %r (empty)" % (what, text))
        return [str(v) for v in range(lo, hi + 1)]
    toks = [t.strip() for t in text.split(",")]
    for t in toks:
        try:
            float(t)
        except ValueError:
            raise ValueError("Invalid %s list %r" % (what, text))
    return toks


def substitute(wspecifier, lmwt, wip):
    return wspecifier.replace("LMWT", lmwt).replace("WIP", wip)


def main(argv=None):
    cli = importlib.import_module("old-kaldi-git_amd.kaldi_cli")
    prog = "lattice-best-path"
    capi = importlib.import_module("old-kaldi-git_amd.capi")
    argv = [prog] + list(sys.argv[1:] if argv is None else argv)
    try:
        return run(cli, argv, prog)
    except (cli.KaldiError, ValueError, capi.KhError) as e:
        sys.stderr.write("ERROR (%s) %s\n" % (prog, e))
        return 255
    finally:
        cli.stop_pipe_helper()


def run(cli, argv, prog):
    cli.start_pipe_helper()
    po = cli.ParseOptions(USAGE)
    po.register("acoustic-scale", 1.0, "Scaling factor for acoustic likelihoods", float)
    po.register("lm-scale", 1.0, "Scaling factor for LM probabilities. Note: the ratio acoustic-scale/lm-scale is all that matters.", float)
    po.register("word-symbol-table", "", "Symbol table for words [for debug output]", str)
    po.register("inv-acoustic-scales", "", "[MI355X] sweep: first:last or a comma list; each value as lattice-scale "
                "--inv-acoustic-scale before the search, LMWT in the wspecifiers stands for it", str)
    po.register("word-ins-penalties", "", "[MI355X] sweep: a comma list; each value as lattice-add-penalty --word-ins-penalty "
                "before the search, WIP in the wspecifiers stands for it", str)
    po.register("batch-arcs", 2000000, "[MI355X] lattice arcs per best-path call", int)
    po.register("gpu", 0, "[MI355X] device ordinal", int)
    po.read(argv)
    cli.set_program_name(prog)
    if po.num_args() < 1 or po.num_args() > 3:
        po.print_usage()
        return 1
    api = importlib.import_module("old-kaldi-git_amd.api")
    sweep = po["inv-acoustic-scales"] != "" or po["word-ins-penalties"] != ""
    if sweep:
        if np.float32(po["acoustic-scale"]) != 1.0 or np.float32(po["lm-scale"]) != 1.0:
            raise cli.KaldiError("the sweep stands for lattice-scale | lattice-add-penalty | lattice-best-path with the last "
                                 "one's scales at 1.0: do not combine it with --acoustic-scale / --lm-scale")
        lmwts = parse_sweep_list(po["inv-acoustic-scales"], "--inv-acoustic-scales") if po["inv-acoustic-scales"] else ["1"]
        wips = parse_sweep_list(po["word-ins-penalties"], "--word-ins-penalties") if po["word-ins-penalties"] else ["0.0"]
        names = [(l, w) for w in wips for l in lmwts]
        points = [api.score_point(inv_acoustic_scale=float(l), word_ins_penalty=float(w)) for l, w in names]
        specs = [(substitute(po.get_opt_arg(2), l, w), substitute(po.get_opt_arg(3), l, w)) for l, w in names]
        for k in (0, 1):
            used = [s[k] for s in specs if s[k] != ""]
            if len(set(used)) != len(used):
                raise cli.KaldiError("the sweep's wspecifiers must differ per point (use LMWT and WIP in them): %s" % used[0])
    else:
        # fst::LatticeScale(lm_scale, acoustic_scale) :85 (the options are floats, the matrix holds doubles)
        names = [None]
        points = [api.score_point(lm_scale=po["lm-scale"], acoustic_scale=po["acoustic-scale"])]
        specs = [(po.get_opt_arg(2), po.get_opt_arg(3))]
    K = len(points)
    reader = cli.SequentialTableReader(po.get_arg(1), "compact_lattice")
    word_w = [cli.TableWriter(s[0], "int32_vector") for s in specs]
    ali_w = [cli.TableWriter(s[1], "int32_vector") for s in specs]
    word_syms = cli.read_symbol_table(po["word-symbol-table"]) if po["word-symbol-table"] != "" else None
    api.select_gpu(po["gpu"])
    f32 = np.float32
    n_done, n_fail, n_frame = [0] * K, [0] * K, [0] * K
    tot_g, tot_a = [f32(0.0)] * K, [f32(0.0)] * K        # LatticeWeight::One() :79
    tag = lambda p: "" if names[p] is None else "[LMWT=%s WIP=%s] " % names[p]

    def fail(key, p):
        cli.warn("%sBest-path failed for key %s" % (tag(p), key))
        n_fail[p] += 1

    def flush(batch):
        if not batch:
            return
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

    batch, arcs = [], 0
    for key, clat in reader:
        if int(clat["n_states"]) == 0 or int(clat.get("start", 0)) < 0:      # :1055: no start state, empty best path
            for p in range(K):
                fail(key, p)
            continue
        batch.append((key, clat))
        arcs += len(clat["arc_src"])
        if arcs >= po["batch-arcs"]:
            flush(batch)
            batch, arcs = [], 0
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
