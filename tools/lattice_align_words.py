#!/usr/bin/env python3
"""lattice-align-words on the MI355X path: latbin/lattice-align-words.cc:28-134 over the library's batched WordAlignLattice
(csrc/kh_latalign.hip; lat/word-align-lattice.cc).

  lattice-align-words [options] <word-boundary-file> <model> <lattice-rspecifier> <lattice-wspecifier>
   e.g.: lattice-align-words --silence-label=4320 --partial-word-label=4324 \\
           data/lang/phones/word_boundary.int final.mdl ark:1.lats ark:aligned.lats

The aligned lattices carry the states, arcs, labels, strings and weights of the reference's; their state numbering and
arc order are the library's own rule (include/kaldi_hip.h), already top-sorted.  Differences: --test=true is refused; a
lattice that exceeds --max-expand is counted as an error and NOT written (the reference writes the fragment it had
reached); a lattice whose state times are not consistent ends the program; the KALDI_ERR of :595-603 ends it at that
utterance whichever warning came before.  One warning of the library is kept per utterance (the constructor's, for input
that is not deterministic); the scans' own warnings are summed up in the status."""
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
kt = importlib.import_module("old-kaldi-git_amd.kaldi_tool")

PROG = "lattice-align-words"
USAGE = ("Convert lattices so that the arcs in the CompactLattice format correspond with\n"
         "words (i.e. aligned with word boundaries).  Note: it will generally be more\n"
         "efficient if you apply 'lattice-push' before this program.\n"
         "Usage: lattice-align-words [options] <word-boundary-file> <model> <lattice-rspecifier> <lattice-wspecifier>\n"
         " e.g.: lattice-align-words  --silence-label=4320 --partial-word-label=4324 \\\n"
         "   data/lang/phones/word_boundary.int final.mdl ark:1.lats ark:aligned.lats\n"
         "Note: word-boundary file has format (on each line):\n"
         "<integer-phone-id> [begin|end|singleton|internal|nonword]\n"
         "See also: lattice-align-words-lexicon, for use in cases where phones\n"
         "don't have word-position information.\n")


def main(argv=None):
    return kt.run_tool(PROG, run, argv, kt.KALDI_KH)


def not_deterministic(clat):
    """Properties(kIDeterministic | kIEpsilons) != kIDeterministic (:261-262): an arc with label 0, or two arcs of one state
    with the same label."""
    lab, src = np.asarray(clat["arc_label"], np.int64), np.asarray(clat["arc_src"], np.int64)
    if np.any(lab == 0):
        return True
    key = src * (int(lab.max()) + 1 if len(lab) else 1) + lab
    return len(np.unique(key)) != len(key)


def run(cli, argv):
    def register(po):
        po.register("output-error-lats", True, "Output lattices that aligned with errors (e.g. due to force-out", bool)
        po.register("test", False, "Test the algorithm while running it.", bool)
        po.register("max-expand", 0.0, "If >0, the maximum amount by which this program will expand lattices before refusing to "
                    "continue.  E.g. 10.This can be used to prevent this program consuming excessive memory if there is a mismatch "
                    "on the command-line or a 'problem' lattice.", float)
        po.register("silence-label", 0, "Numeric id of word symbol that is to be used for silence arcs in the word-aligned "
                    "lattice (zero is OK)", int)
        po.register("partial-word-label", 0, "Numeric id of word symbol that is to be used for arcs in the word-aligned lattice "
                    "corresponding to partial words at the end of \"forced-out\" utterances (zero is OK)", int)
        po.register("reorder", True, "True if the lattices were generated from graphs that had the --reorder option true, "
                    "relating to reordering self-loops (typically true)", bool)
        po.register("batch-arcs", 200000, "[MI355X] lattice arcs per call", int)
        kt.register_gpu(po)
    po = kt.parse(cli, PROG, USAGE, argv, register, 4)
    if po is None:
        return 1
    if po["test"]:
        raise cli.KaldiError("--test=true is not provided: TestWordAlignedLattice's RandEquivalent draws from the C library's "
                             "rand(); tests/test_lattice_align_words.py makes its checks on the library's result")
    kio = importlib.import_module("old-kaldi-git_amd.kaldi_io")
    api = importlib.import_module("old-kaldi-git_amd.api")
    tmodel = cli.read_kaldi_object(po.get_arg(2), kio.read_transition_model)                        # :74-75
    reader = cli.SequentialTableReader(po.get_arg(3), "compact_lattice")
    writer = cli.TableWriter(po.get_arg(4), "compact_lattice")
    f, kind = cli.open_input(po.get_arg(1))                                                        # :80, :681-683: any rxfilename
    try:
        wbinfo = kio.parse_word_boundary_info(f.read(), po["reorder"], po["silence-label"], po["partial-word-label"])
    finally:
        cli._close(f, kind)
    kt.select_gpu(api, po)
    max_expand = np.float32(po["max-expand"])
    n_done, n_err = 0, 0
    for batch in kt.batches(reader, lambda b: len(b[1]["arc_src"]), po["batch-arcs"], "after"):
        if max_expand > 0:                                                                          # :90: int32 = float
            ms = [int(np.float32(1000) + max_expand * np.float32(int(c["n_states"]))) for _, c in batch]
        else:
            ms = [0] * len(batch)
        res = api.compact_lattice_align_words([c for _, c in batch], tmodel, wbinfo, ms)
        for (key, clat), m, r in zip(batch, ms, res):
            status, aligned = r["status"], r["clat"]
            if not_deterministic(clat):                                                             # :261-266
                cli.warn("[Lattice has input epsilons and/or is not input-deterministic (in Mohri sense)]-- i.e. lattice is not "
                         "deterministic.  Word-alignment may be slow and-or blow up in memory.", "LatticeWordAligner()")
            if status == api.ALIGN_FATAL:                             # :595-603 throws; the utterances before it are written
                writer.close()
                raise cli.KaldiError("Broken silence arc at end of utterance (the phone changed); code error [utterance %s]" % key)
            if status == api.ALIGN_EMPTY:                                                           # :305-308
                cli.warn("Trying to word-align empty lattice.", "AlignLattice()")
            if status == api.ALIGN_TOO_MANY_STATES:                                                 # :315-321
                cli.warn("Number of states in lattice exceeded max-states of %d, original lattice had %d states.  Producing no "
                         "output for %s." % (m, int(clat["n_states"]), key), "AlignLattice()")
                n_err += 1
                continue
            ok = status == api.ALIGN_OK
            if not ok:                                                                              # :98-112
                n_err += 1
                if not po["output-error-lats"]:
                    cli.warn("Lattice for %s did not align correctly, producing no output." % key)
                elif aligned is not None:
                    cli.warn("Outputting partial lattice for %s" % key)
                    writer.write(key, aligned)
                else:
                    cli.warn("Empty aligned lattice for %s, producing no output." % key)
            elif aligned is None:                                                                   # :114-116
                n_err += 1
                cli.warn("Lattice was empty for key %s" % key)
            else:
                n_done += 1
                cli.vlog(2, "Aligned lattice for %s" % key)
                writer.write(key, aligned)
    writer.close()
    cli.log("Successfully aligned %d lattices; %d had errors." % (n_done, n_err))                   # :125-126
    return 0 if n_done > n_err else 1


if __name__ == "__main__":
    sys.exit(main())
