#!/usr/bin/env python3
"""lattice-oracle on the MI355X path: latbin/lattice-oracle.cc:223-435 over the library's batched oracle-path call
(csrc/kh_latoracle.hip).

  lattice-oracle [options] <test-lattice-rspecifier> <reference-rspecifier> <transcriptions-wspecifier> [<edit-distance-wspecifier>]
   e.g.: lattice-oracle ark:lat.1 'ark:sym2int.pl -f 2- data/lang/words.txt <data/test/text' ark,t:-

errors, the number of reference words and the "Overall %WER" total are the reference binary's.  Which of several equal-cost
paths is reported - the split into insertions, deletions and substitutions, and the oracle word sequence - is in the
reference the choice of fst::ShortestPath (:351-356) and is not reproduced: the rule is the one stated in
include/kaldi_hip.h.  --write-lattices is not provided.

The sweep ([MI355X] options, not the reference's): what steps/oracle_wer.sh runs once per pruning beam,

  lattice-prune --acoustic-scale=$acwt --beam=$beam ark:lats ark:- | lattice-oracle ark:- <ref> ark:oracle_$beam.tra

is one command that reads the archive once, prunes every batch at every beam on the device and scores every point:

  lattice-oracle --acoustic-scale=$acwt --beams=2,4,6,8 ark:lats <ref> ark:oracle_BEAM.tra [ark,t:edits_BEAM.txt]

BEAM in the wspecifiers stands for the beam as it was typed."""
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

kt = importlib.import_module("old-kaldi-git_amd.kaldi_tool")

PROG = "lattice-oracle"
USAGE = ("Finds the path having the smallest edit-distance between two lattices.\n"
         "For efficiency put the smallest lattices first (for example reference strings).\n"
         "Usage: lattice-oracle [options] <test-lattice-rspecifier> <reference-rspecifier> "
         "<transcriptions-wspecifier> [<edit-distance-wspecifier>]\n"
         " e.g.: lattice-oracle ark:lat.1 'ark:sym2int.pl -f 2- data/lang/words.txt <data/test/text' ark,t:-\n"
         "Note: you can use this program to compute the n-best oracle WER by first piping\n"
         "the input lattices through lattice-to-nbest and then nbest-to-lattice.\n")


def cxx_ratio(num, den):
    """operator<< of the double (100. * e) / n, n an int32: the division by zero prints as glibc prints it."""
    if den == 0:
        return "-nan" if num == 0 else "inf"
    return "%g" % (num / den)


def lattice_as_word_graph(lat):
    """A state-level Lattice dict in the CompactLattice dict's layout as far as the oracle path needs it: the words are
    the output labels (ConvertLatticeToUnweightedAcceptor :84-87 projects onto them)."""
    fg = np.asarray(lat.get("state_final_graph", lat["state_final"]), np.float32)
    fa = np.asarray(lat.get("state_final_acoustic", np.zeros(len(fg), np.float32)), np.float32)
    none = np.isinf(fg) | np.isinf(fa)
    inf = np.float32(np.inf)
    return dict(n_states=int(lat["num_states"]), start=int(lat.get("start", 0)), arc_src=np.asarray(lat["arc_src"], np.int32),
                arc_dst=np.asarray(lat["arc_dst"], np.int32), arc_label=np.asarray(lat["arc_ol"], np.int32),
                arc_g=np.asarray(lat["arc_g"], np.float32), arc_a=np.asarray(lat["arc_a"], np.float32),
                final_g=np.where(none, inf, fg), final_a=np.where(none, inf, fa))


def read_symbol_list(cli, rxfilename, word_syms):
    """ReadSymbolList :33-56."""
    by_name = {v: k for k, v in word_syms.items()}
    f, kind = cli.open_input(rxfilename)
    try:
        lines = f.read().decode().splitlines()
    finally:
        cli._close(f, kind)
    out = set()
    for line in lines:
        tok = line.split()
        if len(tok) != 1:
            raise cli.KaldiError("Bad line in symbol list: %s, file is: %s" % (line, rxfilename))
        if tok[0] not in by_name:
            raise cli.KaldiError("Can't find symbol in symbol table: %s, file is: %s" % (line, rxfilename))
        out.add(by_name[tok[0]])
    return out


def main(argv=None):
    return kt.run_tool(PROG, run, argv, kt.KALDI_KH, assert_status=134)          # KALDI_ASSERT aborts


def run(cli, argv):
    def register(po):
        po.register("word-symbol-table", "", "Symbol table for words [for debug output]", str)
        po.register("wildcard-symbols-list", "", "Filename (generally, rxfilename) for file containing text-form list of symbols that "
                    "don't count as errors; this option requires --word-symbol-table.  Deprecated; use --wildcard-symbols option.", str)
        po.register("wildcard-symbols", "", "Colon-separated list of integer ids of symbols that don't count as errors.  Preferred "
                    "alternative to deprecated option --wildcard-symbols-list.", str)
        po.register("write-lattices", "", "If supplied, write 1-best path as lattices to this wspecifier [not provided here]", str)
        po.register("acoustic-scale", 1.0, "[MI355X] with --beams: as lattice-prune --acoustic-scale in front of this program", float)
        po.register("beams", "", "[MI355X] sweep: first:last or a comma list; each value as lattice-prune --beam in front of this "
                    "program, BEAM in the wspecifiers stands for it", str)
        po.register("batch-arcs", 2000000, "[MI355X] lattice arcs per device call", int)
        po.register("gpu", 0, "[MI355X] device ordinal", int)
    po = kt.parse(cli, PROG, USAGE, argv, register, range(3, 5))               # :265
    if po is None:
        return 1
    if po["write-lattices"] != "":
        raise cli.KaldiError("--write-lattices is not provided by this implementation")
    sweep = po["beams"] != ""
    beams, (tra_specs, edit_specs), tag = kt.beam_sweep(cli, po, (po.get_arg(3), po.get_opt_arg(4)))
    K = len(beams)

    word_syms = None
    if po["word-symbol-table"] != "":                                          # :285-288
        try:
            word_syms = cli.read_symbol_table(po["word-symbol-table"])
        except Exception:
            raise cli.KaldiError("Could not read symbol table from file " + po["word-symbol-table"])
    if po["wildcard-symbols-list"] != "":                                      # :291-297
        cli.warn("--wildcard-symbols-list option deprecated.")
        if po["wildcard-symbols"] != "":
            raise AssertionError("KALDI_ASSERT: at main:lattice-oracle.cc:293, failed: wildcard_symbols.empty() && \"Do not use "
                                 "both --wildcard-symbols and --wildcard-symbols-list options.\"")
        if word_syms is None:
            raise AssertionError("KALDI_ASSERT: at main:lattice-oracle.cc:295, failed: word_syms != NULL && "
                                 "\"--wildcard-symbols-list option requires --word-symbol-table option\"")
        wildcards = read_symbol_list(cli, po["wildcard-symbols-list"], word_syms)
    else:                                                                      # :299-306
        try:
            wildcards = set(int(t) for t in po["wildcard-symbols"].split(":") if t != "")
        except ValueError:
            raise cli.KaldiError("Expected colon-separated list of integers for --wildcard-symbols option, got: " + po["wildcard-symbols"])

    reader = cli.SequentialTableReader(po.get_arg(1), "compact_lattice" if sweep else "lattice_or_compact")
    refs = cli.RandomAccessTableReader(po.get_arg(2), "int32_vector")
    tra_w = [cli.TableWriter(s, "int32_vector") for s in tra_specs]
    edit_w = [cli.TableWriter(s, "int32") for s in edit_specs]
    api = importlib.import_module("old-kaldi-git_amd.api")
    api.select_gpu(po["gpu"])
    point = api.score_point(acoustic_scale=po["acoustic-scale"])
    n_done, n_fail = [0] * K, [0] * K
    tot = [dict(correct=0, sub=0, ins=0, words=0, **{"del": 0}) for _ in range(K)]

    def flush(batch):
        clats, rws = [c for _, c, _ in batch], [r for _, _, r in batch]
        if sweep:
            res = api.compact_lattice_oracle(clats, rws, wildcards, points=[point], beams=[float(b) for b in beams])
        else:
            res = api.compact_lattice_oracle(clats, rws, wildcards)
        for (key, _, ref), row in zip(batch, res):
            for p, r in enumerate(row):
                if r["errors"] < 0:                                            # :359-361
                    cli.warn("%sBest-path failed for key %s" % (tag(p), key))
                    n_fail[p] += 1
                else:
                    num_words = r["correct"] + r["sub"] + r["del"]             # CountErrors :131-164
                    tot_errs = r["sub"] + r["ins"] + r["del"]                  # :366
                    edit_w[p].write(key, tot_errs)                             # :367-368
                    cli.log("%s%%WER %s [ %d / %d, %d insertions, %d deletions, %d sub ]"
                            % (tag(p), cxx_ratio(100.0 * tot_errs, num_words), tot_errs, num_words, r["ins"], r["del"], r["sub"]))   # :369-371
                    for k in ("correct", "sub", "ins", "del"):                 # :372-376
                        tot[p][k] += r[k]
                    tot[p]["words"] += num_words
                    cli.log("%sFor utterance %s, best cost %g" % (tag(p), key, tot_errs))   # :382
                    tra_w[p].write(key, np.asarray(r["words"], np.int32))      # :383-384
                    if word_syms is not None:                                  # :385-402
                        reference_words = [int(w) for w in ref if int(w) != 0 and int(w) not in wildcards]
                        for what, seq in (("oracle", r["words"]), ("reference", reference_words)):
                            names = []
                            for w in seq:
                                if int(w) not in word_syms:
                                    raise cli.KaldiError("Word-id %d not in symbol table." % int(w))
                                names.append(word_syms[int(w)])
                            sys.stderr.write("%s%s (%s) %s\n" % (tag(p), key, what, "".join(n + " " for n in names)))
                n_done[p] += 1                                                 # :420

    def lattices():
        for key, obj in reader:
            sys.stderr.write("Lattice %s read.\n" % key)                       # :316
            clat = obj if sweep else (obj[1] if obj[0] else lattice_as_word_graph(obj[1]))
            if not refs.has_key(key):                                          # :325-329
                cli.warn("No reference present for utterance " + key)
                for p in range(K):
                    n_fail[p] += 1
                continue
            yield key, clat, np.asarray(refs.value(key), np.int32)

    for batch in kt.batches(lattices(), lambda b: len(b[1]["arc_src"]), po["batch-arcs"], "after"):
        flush(batch)
    for w in tra_w + edit_w:
        w.close()
    for p in range(K):
        t = tot[p]
        tot_errs = t["sub"] + t["del"] + t["ins"]                              # :423
        # steps/oracle_wer.sh parses the next line by field number
        cli.log("%sOverall %%WER %s [ %d / %d, %d insertions, %d deletions, %d substitutions ]"
                % (tag(p), cxx_ratio(100.0 * tot_errs, t["words"]), tot_errs, t["words"], t["ins"], t["del"], t["sub"]))   # :425-428
        cli.log("%sScored %d lattices, %d not present in ref." % (tag(p), n_done[p], n_fail[p]))   # :429-430
    return 0


if __name__ == "__main__":
    sys.exit(main())
