#!/usr/bin/env python3
"""lattice-mbr-decode on the MI355X path: latbin/lattice-mbr-decode.cc:26-131 over the library's batched MinimumBayesRisk
(csrc/kh_latmbr.hip; lat/sausages.cc).

  lattice-mbr-decode [options]  lattice-rspecifier transcriptions-wspecifier [ bayes-risk-wspecifier
                                [ sausage-stats-wspecifier [ times-wspecifier] ] ]
   e.g.: lattice-mbr-decode --acoustic-scale=0.1 ark:1.lats ark:1.tra ark:/dev/null ark:1.sau

The sweep ([MI355X] options, not the reference's): what local/score_mbr.sh runs as one pipeline per LM weight

  lattice-scale --inv-acoustic-scale=LMWT ark:lats ark:- | lattice-add-penalty --word-ins-penalty=$wip ark:- ark:- | \\
    lattice-mbr-decode ark:- ark,t:scoring/LMWT.tra

is one command that reads the archive once and decodes every batch of lattices once for all score points:

  lattice-mbr-decode --inv-acoustic-scales=9:20 --word-ins-penalties=0.0,0.5 ark:lats ark,t:scoring/penalty_WIP/LMWT.tra

LMWT and WIP in the wspecifiers stand for the point's values as they were typed.  [MI355X] --one-best-rspecifier gives the
initial hypotheses (the class's second constructor, with the MBR update on); an utterance without one is skipped with a
warning.  Where best paths tie in cost the initial hypothesis may differ from fst::ShortestPath's (see
api.compact_lattice_mbr).  A lattice without a start state is skipped with a warning."""
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

kt = importlib.import_module("old-kaldi-git_amd.kaldi_tool")

PROG = "lattice-mbr-decode"
USAGE = ("Do Minimum Bayes Risk decoding (decoding that aims to minimize the \n"
         "expected word error rate).  Possible outputs include the 1-best path\n"
         "(i.e. the word-sequence, as a sequence of ints per utterance), the\n"
         "computed Bayes Risk for each utterance, and the sausage stats as\n"
         "(for each utterance) std::vector<std::vector<std::pair<int32, float> > >\n"
         "for which we use the same I/O routines as for posteriors (type Posterior).\n"
         "times-wspecifier writes pairs of (start-time, end-time) in frames, for\n"
         "each sausage position, or for each one-best entry if --one-best-times=true.\n"
         "Note: use ark:/dev/null or the empty string for unwanted outputs.\n"
         "Note: times will only be very meaningful if you first use lattice-word-align.\n"
         "If you need ctm-format output, don't use this program but use lattice-to-ctm-conf\n"
         "with --decode-mbr=true.\n"
         "\n"
         "Usage: lattice-mbr-decode [options]  lattice-rspecifier transcriptions-wspecifier [ bayes-risk-wspecifier "
         "[ sausage-stats-wspecifier [ times-wspecifier] ] ] \n"
         " e.g.: lattice-mbr-decode --acoustic-scale=0.1 ark:1.lats ark:1.tra ark:/dev/null ark:1.sau\n")


def main(argv=None):
    return kt.run_tool(PROG, run, argv, kt.KALDI_KH)


def run(cli, argv):
    def register(po):
        po.register("acoustic-scale", 1.0, "Scaling factor for acoustic likelihoods", float)
        po.register("lm-scale", 1.0, "Scaling factor for language model probabilities", float)
        po.register("word-symbol-table", "", "Symbol table for words [for debug output]", str)
        po.register("one-best-times", False, "If true, output times corresponding to one-best, not whole sausage.", bool)
        po.register("one-best-rspecifier", "", "[MI355X] initial hypotheses (int32 vectors) in place of the lattices' best paths", str)
        po.register("inv-acoustic-scales", "", "[MI355X] sweep: first:last or a comma list; each value as lattice-scale "
                    "--inv-acoustic-scale before the decoding, LMWT in the wspecifiers stands for it", str)
        po.register("word-ins-penalties", "", "[MI355X] sweep: a comma list; each value as lattice-add-penalty --word-ins-penalty "
                    "before the decoding, WIP in the wspecifiers stands for it", str)
        po.register("batch-arcs", 200000, "[MI355X] lattice arcs per call", int)
        po.register("gpu", 0, "[MI355X] device ordinal", int)
    po = kt.parse(cli, PROG, USAGE, argv, register, range(2, 6))
    if po is None:
        return 1
    api = importlib.import_module("old-kaldi-git_amd.api")
    sw = kt.score_sweep(cli, api, po, (2, 3, 4, 5), "outputs")
    if sw is not None:
        if np.float32(po["acoustic-scale"]) != 1.0 or np.float32(po["lm-scale"]) != 1.0:
            raise cli.KaldiError("the sweep stands for lattice-scale | lattice-add-penalty | lattice-mbr-decode with the last "
                                 "one's scales at 1.0: do not combine it with --acoustic-scale / --lm-scale")
        points, specs, tag = sw
    else:
        points = [api.score_point(lm_scale=po["lm-scale"], acoustic_scale=po["acoustic-scale"])]   # :101
        specs = [tuple(po.get_opt_arg(k) for k in (2, 3, 4, 5))]
        tag = lambda p: ""
    K = len(points)
    reader = cli.SequentialTableReader(po.get_arg(1), "compact_lattice")
    one_best = cli.RandomAccessTableReader(po["one-best-rspecifier"], "int32_vector") if po["one-best-rspecifier"] != "" else None
    trans_w = [cli.TableWriter(s[0], "int32_vector") for s in specs]
    risk_w = [cli.TableWriter(s[1], "base_float") for s in specs]
    stats_w = [cli.TableWriter(s[2], "posterior") for s in specs]
    times_w = [cli.TableWriter(s[3], "base_float_pair_vector") for s in specs]
    if po["word-symbol-table"] != "":
        cli.read_symbol_table(po["word-symbol-table"])     # :88-92 (read, and not used again by the reference either)
    api.select_gpu(po["gpu"])
    f32 = np.float32
    n_done, n_words, tot = [0] * K, [0] * K, [f32(0.0)] * K
    for batch in kt.batches(reader, lambda b: len(b[1]["arc_src"]), po["batch-arcs"], "after"):
        keep, given = [], []
        for key, clat in batch:
            if int(clat["n_states"]) == 0 or int(clat.get("start", 0)) < 0:
                cli.warn("Empty lattice for utterance %s" % key)
                continue
            if one_best is not None:
                if not one_best.has_key(key):
                    cli.warn("No 1-best present for utterance %s" % key)
                    continue
                given.append(one_best.value(key))
            keep.append((key, clat))
        if not keep:
            continue
        res = api.compact_lattice_mbr([c for _, c in keep], points, given if one_best is not None else None, True)
        for (key, _), row in zip(keep, res):
            for p, r in enumerate(row):
                trans_w[p].write(key, r["words"])                                        # :105-106
                risk_w[p].write(key, r["bayes_risk"])                                    # :107-108
                stats_w[p].write(key, r["sausage_stats"])                                # :109-110
                times_w[p].write(key, r["one_best_times"] if po["one-best-times"] else r["sausage_times"])   # :111-113
                n_done[p] += 1
                n_words[p] += len(r["words"])
                tot[p] = tot[p] + f32(r["bayes_risk"])
    for w in trans_w + risk_w + stats_w + times_w:
        w.close()
    with np.errstate(divide="ignore", invalid="ignore"):
        for p in range(K):
            cli.log("%sDone %d lattices." % (tag(p), n_done[p]))
            cli.log("%sAverage Bayes Risk per sentence is %s and per word, %s"
                    % (tag(p), cli._cxx_float(tot[p] / f32(n_done[p])), cli._cxx_float(tot[p] / f32(n_words[p]))))
    return 0 if all(n != 0 for n in n_done) else 1


if __name__ == "__main__":
    sys.exit(main())
