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

from tools.lattice_best_path import parse_sweep_list, substitute  # noqa: E402

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


def sweep_points(cli, api, po, n_specs, first_spec):
    """The score points and the output names of a run: (names [None or (LMWT, WIP) as typed], points, specs [per point the
    positional arguments first_spec .. first_spec + n_specs - 1 with LMWT / WIP replaced])."""
    if po["inv-acoustic-scales"] == "" and po["word-ins-penalties"] == "":
        return None
    lmwts = parse_sweep_list(po["inv-acoustic-scales"], "--inv-acoustic-scales") if po["inv-acoustic-scales"] else ["1"]
    wips = parse_sweep_list(po["word-ins-penalties"], "--word-ins-penalties") if po["word-ins-penalties"] else ["0.0"]
    names = [(l, w) for w in wips for l in lmwts]
    points = [api.score_point(inv_acoustic_scale=float(l), word_ins_penalty=float(w)) for l, w in names]
    specs = [tuple(substitute(po.get_opt_arg(first_spec + k), l, w) for k in range(n_specs)) for l, w in names]
    for k in range(n_specs):
        used = [s[k] for s in specs if s[k] != ""]
        if len(set(used)) != len(used):
            raise cli.KaldiError("the sweep's outputs must differ per point (use LMWT and WIP in them): %s" % used[0])
    return names, points, specs


def batches(reader, batch_arcs):
    batch, arcs = [], 0
    for key, clat in reader:
        batch.append((key, clat))
        arcs += len(clat["arc_src"])
        if arcs >= batch_arcs:
            yield batch
            batch, arcs = [], 0
    if batch:
        yield batch


def main(argv=None):
    cli = importlib.import_module("old-kaldi-git_amd.kaldi_cli")
    prog = "lattice-mbr-decode"
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
    po.read(argv)
    cli.set_program_name(prog)
    if po.num_args() < 2 or po.num_args() > 5:
        po.print_usage()
        return 1
    api = importlib.import_module("old-kaldi-git_amd.api")
    sw = sweep_points(cli, api, po, 4, 2)
    if sw is not None:
        if np.float32(po["acoustic-scale"]) != 1.0 or np.float32(po["lm-scale"]) != 1.0:
            raise cli.KaldiError("the sweep stands for lattice-scale | lattice-add-penalty | lattice-mbr-decode with the last "
                                 "one's scales at 1.0: do not combine it with --acoustic-scale / --lm-scale")
        names, points, specs = sw
    else:
        names = [None]
        points = [api.score_point(lm_scale=po["lm-scale"], acoustic_scale=po["acoustic-scale"])]   # :101
        specs = [tuple(po.get_opt_arg(k) for k in (2, 3, 4, 5))]
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
    tag = lambda p: "" if names[p] is None else "[LMWT=%s WIP=%s] " % names[p]
    for batch in batches(reader, po["batch-arcs"]):
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
