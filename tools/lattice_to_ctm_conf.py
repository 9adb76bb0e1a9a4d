#!/usr/bin/env python3
"""lattice-to-ctm-conf on the MI355X path: latbin/lattice-to-ctm-conf.cc:26-168 over the library's batched MinimumBayesRisk
(csrc/kh_latmbr.hip; lat/sausages.cc).

  lattice-to-ctm-conf [options]  <lattice-rspecifier> <ctm-wxfilename>
  lattice-to-ctm-conf [options]  <lattice-rspecifier> [<1best-rspecifier>] <ctm-wxfilename>
   e.g.: lattice-to-ctm-conf --acoustic-scale=0.1 ark:1.lats 1.ctm
     or: lattice-to-ctm-conf --acoustic-scale=0.1 --decode-mbr=false ark:1.lats ark:1.1best 1.ctm

The sweep ([MI355X] options, not the reference's): the tail of the recipes' sclite scoring line, run once per LM weight as

  lattice-scale --inv-acoustic-scale=LMWT ark:lats ark:- | lattice-add-penalty --word-ins-penalty=$wip ark:- ark:- | \\
    lattice-prune --beam=5 ark:- ark:- | lattice-to-ctm-conf --decode-mbr=true ark:- score_LMWT/utt.ctm

is one command (without the pruning stage) that reads the archive once and decodes every batch once for all score points:

  lattice-to-ctm-conf --inv-acoustic-scales=9:20 --word-ins-penalties=0.0 ark:lats score_LMWT_WIP/utt.ctm

LMWT and WIP in the output name stand for the point's values as they were typed.  Where best paths tie in cost the initial
hypothesis may differ from fst::ShortestPath's (see api.compact_lattice_mbr).  A lattice without a start state is skipped
with a warning."""
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

kt = importlib.import_module("old-kaldi-git_amd.kaldi_tool")

PROG = "lattice-to-ctm-conf"
USAGE = ("This tool turns a lattice into a ctm with confidences, based on the\n"
         "posterior probabilities in the lattice.  The word sequence in the\n"
         "ctm is determined as follows.  Firstly we determine the initial word\n"
         "sequence.  In the 3-argument form, we read it from the\n"
         "<1best-rspecifier> input; otherwise it is the 1-best of the lattice.\n"
         "Then, if --decode-mbr=true, we iteratively refine the hypothesis\n"
         "using Minimum Bayes Risk decoding.  If you don't need confidences,\n"
         "you can do lattice-1best and pipe to nbest-to-ctm. The ctm this\n"
         "program produces will be relative to the utterance-id; a standard\n"
         "ctm relative to the filename can be obtained using\n"
         "utils/convert_ctm.pl.  The times produced by this program will only\n"
         "be meaningful if you do lattice-align-words on the input.  The\n"
         "<1-best-rspecifier> could be the output of utils/int2sym.pl or\n"
         "nbest-to-linear.\n"
         "\n"
         "Usage: lattice-to-ctm-conf [options]  <lattice-rspecifier> \\\n"
         "                                          <ctm-wxfilename>\n"
         "Usage: lattice-to-ctm-conf [options]  <lattice-rspecifier> \\\n"
         "                     [<1best-rspecifier>] <ctm-wxfilename>\n"
         " e.g.: lattice-to-ctm-conf --acoustic-scale=0.1 ark:1.lats 1.ctm\n"
         "   or: lattice-to-ctm-conf --acoustic-scale=0.1 --decode-mbr=false\\\n"
         "                                      ark:1.lats ark:1.1best 1.ctm\n"
         "See also: lattice-mbr-decode, nbest-to-ctm, steps/get_ctm.sh,\n"
         "          steps/get_train_ctm.sh and utils/convert_ctm.sh.\n")

f32 = np.float32


def ctm_lines(key, r, frame_shift):
    """:142-147: the products are BaseFloat; the stream is std::fixed with precision 2, which is sticky, so the confidence
    is printed to two places as well."""
    frame_shift = f32(frame_shift)
    out = []
    for word, (t0, t1), conf in zip(r["words"], np.asarray(r["one_best_times"], f32).reshape(-1, 2), r["one_best_confidences"]):
        assert int(word) != 0                                                # :143
        start, dur = frame_shift * f32(t0), frame_shift * (f32(t1) - f32(t0))
        out.append("%s 1 %.2f %.2f %d %.2f\n" % (key, float(start), float(dur), int(word), float(f32(conf))))
    return out


def main(argv=None):
    return kt.run_tool(PROG, run, argv, kt.KALDI_KH)


def run(cli, argv):
    def register(po):
        po.register("acoustic-scale", 1.0, "Scaling factor for acoustic likelihoods", float)
        po.register("inv-acoustic-scale", 1.0, "An alternative way of setting the acoustic scale: you can set its inverse.", float)
        po.register("lm-scale", 1.0, "Scaling factor for language model probabilities", float)
        po.register("decode-mbr", True, "If true, do Minimum Bayes Risk decoding (else, Maximum a Posteriori)", bool)
        po.register("frame-shift", 0.01, "Time in seconds between frames.", float)
        po.register("inv-acoustic-scales", "", "[MI355X] sweep: first:last or a comma list; each value as lattice-scale "
                    "--inv-acoustic-scale before the decoding, LMWT in the output name stands for it", str)
        po.register("word-ins-penalties", "", "[MI355X] sweep: a comma list; each value as lattice-add-penalty --word-ins-penalty "
                    "before the decoding, WIP in the output name stands for it", str)
        po.register("batch-arcs", 200000, "[MI355X] lattice arcs per call", int)
        po.register("gpu", 0, "[MI355X] device ordinal", int)
    po = kt.parse(cli, PROG, USAGE, argv, register, range(2, 4))
    if po is None:
        return 1
    api = importlib.import_module("old-kaldi-git_amd.api")
    one_best_rspecifier = po.get_arg(2) if po.num_args() == 3 else ""        # :86-94
    ctm_arg = po.num_args()
    sw = kt.score_sweep(cli, api, po, (ctm_arg,), "outputs")
    if sw is not None:
        if f32(po["acoustic-scale"]) != 1.0 or f32(po["inv-acoustic-scale"]) != 1.0 or f32(po["lm-scale"]) != 1.0:
            raise cli.KaldiError("the sweep stands for lattice-scale | lattice-add-penalty | lattice-to-ctm-conf with the last "
                                 "one's scales at 1.0: do not combine it with --acoustic-scale / --inv-acoustic-scale / --lm-scale")
        points, specs, tag = sw
        outs = [s[0] for s in specs]
    else:
        # :80-82, :122 (score_point asserts acoustic_scale == 1.0 || inv_acoustic_scale == 1.0 and divides in float)
        points = [api.score_point(lm_scale=po["lm-scale"], acoustic_scale=po["acoustic-scale"], inv_acoustic_scale=po["inv-acoustic-scale"])]
        outs = [po.get_arg(ctm_arg)]
        tag = lambda p: ""
    for o in outs:
        if cli.classify_wspecifier(o)[0] is not None:                        # :96-103
            raise cli.KaldiError("The output ctm file should not be a wspecifier. Please use things like 1.ctm istead of ark:-")
    K = len(points)
    reader = cli.SequentialTableReader(po.get_arg(1), "compact_lattice")
    one_best = cli.RandomAccessTableReader(one_best_rspecifier, "int32_vector") if one_best_rspecifier != "" else None
    kos = [cli.open_output(o) for o in outs]                                 # :110 (text mode)
    api.select_gpu(po["gpu"])
    n_done, n_words, tot = [0] * K, [0] * K, [f32(0.0)] * K
    for batch in kt.batches(reader, lambda b: len(b[1]["arc_src"]), po["batch-arcs"], "after"):
        keep, given = [], []
        for key, clat in batch:
            if int(clat["n_states"]) == 0 or int(clat.get("start", 0)) < 0:
                cli.warn("Empty lattice for utterance %s" % key)
                continue
            if one_best is not None:
                if not one_best.has_key(key):                                # :129-132
                    cli.warn("No 1-best present for utterance %s" % key)
                    continue
                given.append(one_best.value(key))
            keep.append((key, clat))
        if not keep:
            continue
        res = api.compact_lattice_mbr([c for _, c in keep], points, given if one_best is not None else None, po["decode-mbr"])
        for (key, _), row in zip(keep, res):
            for p, r in enumerate(row):
                kos[p][0].write("".join(ctm_lines(key, r, po["frame-shift"])).encode())
                conf = np.asarray(r["one_best_confidences"], f32)
                with np.errstate(divide="ignore", invalid="ignore"):
                    avg = np.float64(sum(float(c) for c in conf)) / np.float64(len(conf))    # :150 (a double sum over a size_t)
                msg = "%sFor utterance %s, Bayes Risk %s, avg. confidence per-word %s" % (tag(p), key, cli._cxx_float(f32(r["bayes_risk"])),
                                                                                         cli._cxx_float(avg))
                if sw is not None:
                    cli.vlog(1, msg)
                else:
                    cli.log(msg)
                n_done[p] += 1
                n_words[p] += len(r["words"])
                tot[p] = tot[p] + f32(r["bayes_risk"])
    for f, kind in kos:
        cli._close(f, kind)
    with np.errstate(divide="ignore", invalid="ignore"):
        for p in range(K):
            cli.log("%sDone %d lattices." % (tag(p), n_done[p]))
            cli.log("%sOverall average Bayes Risk per sentence is %s and per word, %s"
                    % (tag(p), cli._cxx_float(tot[p] / f32(n_done[p])), cli._cxx_float(tot[p] / f32(n_words[p]))))
    return 0 if all(n != 0 for n in n_done) else 1


if __name__ == "__main__":
    sys.exit(main())
