#!/usr/bin/env python3
"""gmm-rescore-lattice: gmmbin/gmm-rescore-lattice.cc:31-110 over the library - the final pass of steps/decode_fmllr.sh
(stage 4) and the head of its second fMLLR pass (stage 3), with bin/ in front of PATH:

  gmm-rescore-lattice $srcdir/final.mdl "ark:gunzip -c $dir/lat.tmp.JOB.gz|" "$feats" ark:- | \\
    lattice-determinize-pruned --acoustic-scale=$acwt --beam=$lattice_beam ark:- "ark:|gzip -c > $dir/lat.JOB.gz"

  gmm-rescore-lattice [--old-acoustic-scale=0.0] <model-in> <lattice-rspecifier> <feature-rspecifier> <lattice-wspecifier>

The lattice table is read as CompactLatticeHolder reads it (kaldi_io "compact_lattice_converted": a table of state-level
Lattices - what `gmm-latgen-faster --determinize-lattice=false` writes - is converted by ConvertLattice); the features by
random access.  ScaleLattice(AcousticLatticeScale(old_acoustic_scale)) whenever the scale is not 1.0 (double arithmetic, Zero
weights skipped: tools/lattice_scale.py), then api.gmm_rescore_compact_lattices on batches of --batch-frames frames:
DecodableAmDiagGmm's unscaled log-likelihoods added to the acoustic costs in frame order (include/kaldi_hip.h at
kh_rescore_compact_lattice).  The lattice written is in the top-sorted numbering, as the reference's argument is after
RescoreCompactLattice.

Differences from the binary.  A batch's warnings ("Rescoring empty lattice", "Features are too short ...") come when the
batch is done, not as each lattice is read.  Where the reference asserts - a lattice whose states have no consistent times,
or a start state that is not the lowest in the sort - or indexes unchecked (a transition-id the model does not have), this
warns and counts an error.  "Utterance does not seem to have a consistent length." is not printed.
--batch-frames, --gpu, --world, --rank are not reference options."""
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from tools.lattice_scale import scale_compact_lattice   # noqa: E402
kt = importlib.import_module("old-kaldi-git_amd.kaldi_tool")

PROG = "gmm-rescore-lattice"
USAGE = ("Replace the acoustic scores on a lattice using a new model.\n"
         "Usage: gmm-rescore-lattice [options] <model-in> <lattice-rspecifier> <feature-rspecifier> <lattice-wspecifier>\n"
         " e.g.: gmm-rescore-lattice 1.mdl ark:1.lats scp:trn.scp ark:2.lats\n")


def acoustic_lattice_scale(scale):
    """AcousticLatticeScale(BaseFloat): the option is a float, the matrix holds doubles (fstext/lattice-utils.h:131-138)."""
    return np.array([[1.0, 0.0], [0.0, float(np.float32(scale))]], np.float64)


def main(argv=None):
    return kt.run_tool(PROG, run, argv, kt.KALDI_KH)


def run(cli, argv):
    def register(po):
        po.register("old-acoustic-scale", 0.0, "Add in the scores in the input lattices with this scale, rather than discarding them.", float)
        po.register("batch-frames", 200000, "[MI355X] frames per library call (bounds the frame x pdf matrix)", int)
        kt.register_gpu(po)
        kt.register_ranks(po)
    argv, rank, world, raw_pos = kt.rank_substitute(argv)
    po = kt.parse(cli, PROG, USAGE, argv, register, 4)
    if po is None:
        return 1
    if world > 1 and not ("JOB" in raw_pos[1] and "JOB" in raw_pos[3]):
        raise cli.KaldiError("--world=%d: the lattice tables need JOB in their names (lat.tmp.JOB.gz, lat.JOB.gz): every rank "
                             "rescores its own job's table" % world)
    kio = importlib.import_module("old-kaldi-git_amd.kaldi_io")
    tm, am = kt.read_gmm_model(cli, kio, po.get_arg(1))
    feature_reader = cli.RandomAccessTableReader(po.get_arg(3), "matrix")
    lattice_reader = cli.SequentialTableReader(po.get_arg(2), "compact_lattice_converted")
    writer = cli.TableWriter(po.get_arg(4), "compact_lattice")
    old_scale = np.float32(po["old-acoustic-scale"])
    scale = acoustic_lattice_scale(old_scale)
    tot = dict(done=0, err=0, frames=0)
    state = {}

    def flush(batch):
        api = importlib.import_module("old-kaldi-git_amd.api")
        if "gmm" not in state:
            kt.select_gpu(api, po)
            state["gmm"] = kt.device_gmm(api, am)
        feats = kt.stack_rows([m for _, _, m in batch if m.shape[0] > 0], am["dim"])
        rows = np.concatenate([[0], np.cumsum([m.shape[0] for _, _, m in batch])]).astype(np.int64)
        res = api.gmm_rescore_compact_lattices(state["gmm"], feats, rows, [c for _, c, _ in batch], tm["tid2pdf"])
        where = "RescoreCompactLatticeInternal()"
        for (key, clat, m), r in zip(batch, res):
            st = r["status"]
            if st == api.RESCORE_OK:
                out = r["clat"]
                if not np.any(~((out["final_g"] == np.inf) & (out["final_a"] == np.inf))):
                    cli.warn("Utterance does not have a final-state.", "CompactLatticeStateTimes()")
                writer.write(key, out)
                tot["done"] += 1
                tot["frames"] += m.shape[0]
                continue
            tot["err"] += 1
            if st == api.RESCORE_EMPTY:
                cli.warn("Rescoring empty lattice", where)
            elif st == api.RESCORE_CYCLIC:
                cli.warn("Cycles detected in lattice.", where)
            elif st == api.RESCORE_FEATURES_TOO_SHORT:
                cli.warn("Features are too short for lattice: utt-len is %d, %d is last frame" % (r["utt_len"], m.shape[0] - 1), where)
            elif st == api.RESCORE_MISMATCH:
                cli.warn("There appears to be lattice/feature mismatch, aborting.", where)
            elif st == api.RESCORE_INCONSISTENT_TIMES:
                cli.warn("Lattice %s: its states do not have consistent times (the reference asserts here). Skipping" % key, where)
            else:
                cli.warn("Lattice %s has a transition-id outside 1..%d (the reference reads past the model here). Skipping"
                         % (key, len(tm["tid2pdf"]) - 1), where)

    def lattices():
        for key, clat in lattice_reader:
            if not feature_reader.has_key(key):
                cli.warn("No feature found for utterance %s. Skipping" % key)
                tot["err"] += 1
                continue
            feats = feature_reader.value(key)
            if feats.shape[0] > 0 and feats.shape[1] != am["dim"]:
                raise cli.KaldiError("Dim mismatch: data dim = %d vs. model dim = %d" % (feats.shape[1], am["dim"]))
            if old_scale != np.float32(1.0):
                clat = scale_compact_lattice(scale, clat)
            yield key, clat, feats

    for batch in kt.batches(lattices(), lambda b: b[2].shape[0], po["batch-frames"], "after"):
        flush(batch)
    writer.close()
    cli.log("Done %d lattices with errors on %d, #frames is %d" % (tot["done"], tot["err"], tot["frames"]))
    return 0 if tot["done"] != 0 else 1


if __name__ == "__main__":
    sys.exit(main())
