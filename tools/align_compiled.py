#!/usr/bin/env python3
"""gmm-align-compiled / nnet-align-compiled on the MI355X path: the reference binaries' command line
(gmmbin/gmm-align-compiled.cc:32-139, nnet2bin/nnet-align-compiled.cc:33-150) over the library, so that the align steps of the
recipes (steps/align_si.sh, steps/align_fmllr.sh, steps/nnet2/align.sh) run unchanged:

  gmm-align-compiled $scale_opts --beam=$beam --retry-beam=$retry_beam --careful=$careful "$mdl" \\
     "ark:gunzip -c $dir/fsts.JOB.gz|" "$feats" "ark:|gzip -c >$dir/ali.JOB.gz"

The graphs are read sequentially and the features by random access, as in the binaries; AddTransitionProbs
(hmm/hmm-utils.cc:776-830) and --careful's graph (decoder-wrappers.cc:393-420) are api.add_transition_probs and
api.modify_graph_for_careful_alignment; the scores are those of tools/latgen_faster.py's score(); the search is
api.align_compiled - FasterDecoder by the rule of include/kaldi_hip.h at kh_align_compiled - with the reference's retry, its
warnings, its three closing log lines and its exit status (0 if an utterance was aligned, 1 if none, 255 on an error).

Differences from the binaries: utterances are aligned in batches (--batch-frames, not a reference option): one scoring pass
and one search call per batch (a second one over the utterances that are retried), so a warning about an utterance comes when
its batch is done; the optional scores table holds -(w1+w2) summed along the path in path order (the reference regroups the
sum in RemoveEpsLocal).  --use-gpu is accepted and ignored.  Run through gmm_align_compiled.py / nnet_align_compiled.py."""
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
kt = importlib.import_module("old-kaldi-git_amd.kaldi_tool")

USAGE = {
    "gmm": ("Align features given [GMM-based] models.\n"
            "Usage:   gmm-align-compiled [options] model-in graphs-rspecifier feature-rspecifier alignments-wspecifier [scores-wspecifier]\n"
            "e.g.: \n"
            " gmm-align-compiled 1.mdl ark:graphs.fsts scp:train.scp ark:1.ali\n"
            "or:\n"
            " compile-train-graphs tree 1.mdl lex.fst ark:train.tra b, ark:- | \\\n"
            "   gmm-align-compiled 1.mdl ark:- scp:train.scp t, ark:1.ali\n"),
    "nnet2": ("Align features given neural-net-based model\n"
              "Usage:   nnet-align-compiled [options] model-in graphs-rspecifier feature-rspecifier alignments-wspecifier\n"
              "e.g.: \n"
              " nnet-align-compiled 1.mdl ark:graphs.fsts scp:train.scp ark:1.ali\n"
              "or:\n"
              " compile-train-graphs tree 1.mdl lex.fst ark:train.tra b, ark:- | \\\n"
              "   nnet-align-compiled 1.mdl ark:- scp:train.scp t, ark:1.ali\n"),
}
WHERE = "AlignUtteranceWrapper()"


def register_options(po, kind):
    po.register("beam", 200.0, "Decoding beam used in alignment", float)                              # AlignConfig::Register
    po.register("retry-beam", 0.0, "Decoding beam for second try at alignment", float)
    po.register("careful", False, "If true, do 'careful' alignment, which is better at detecting alignment failure (involves "
                "loop to start of decoding graph).")
    po.register("transition-scale", 1.0, "Transition-probability scale [relative to acoustics]", float)
    po.register("acoustic-scale", 1.0, "Scaling factor for acoustic likelihoods", float)
    po.register("self-loop-scale", 1.0, "Scale of self-loop versus non-self-loop log probs [relative to acoustics]", float)
    if kind == "nnet2":
        po.register("use-gpu", "yes", "yes|no|optional|wait, only has effect if compiled with CUDA")
    po.register("batch-frames", 200000, "[MI355X] frames per scoring pass / search call", int)
    kt.register_gpu(po)
    po.register("dry-run", False, "[MI355X] read the inputs, give the warnings about them, align nothing and write nothing into the "
                "tables (a plumbing test without a GPU)")


def check_beams(cli, beam, retry_beam):
    """decoder-wrappers.cc:439-443, thrown by the first utterance that reaches AlignUtteranceWrapper."""
    if (retry_beam != 0 and retry_beam <= beam) or beam <= 0.0:
        raise cli.KaldiError("Beams do not make sense: beam %g, retry-beam %g" % (beam, retry_beam))


def main(argv=None, kind="gmm"):
    prog = "gmm-align-compiled" if kind == "gmm" else "nnet-align-compiled"
    return kt.run_tool(prog, lambda cli, argv: run(cli, argv, kind, prog), argv, kt.KALDI_KH)


def run(cli, argv, kind, prog):
    po = kt.parse(cli, prog, USAGE[kind], argv, lambda po: register_options(po, kind), range(4, 6))
    if po is None:
        return 1
    model_rx, fst_rspec, feats_rspec, ali_wspec = (po.get_arg(i) for i in (1, 2, 3, 4))
    scores_wspec = po.get_opt_arg(5)
    kio = importlib.import_module("old-kaldi-git_amd.kaldi_io")
    if kind == "nnet2":
        tm, (comps, priors) = cli.read_kaldi_object(model_rx, lambda s, b: (kio.read_transition_model(s, b), kio.read_am_nnet(s, b)))
    else:
        tm, am = kt.read_gmm_model(cli, kio, model_rx)
    fst_reader = cli.SequentialTableReader(fst_rspec, "fst")
    feature_reader = cli.RandomAccessTableReader(feats_rspec, "matrix")
    ali_w = cli.TableWriter(ali_wspec, "int32_vector")
    scores_w = cli.TableWriter(scores_wspec, "base_float")
    api = importlib.import_module("old-kaldi-git_amd.api")      # (its graph functions need no device)
    beam, retry_beam, acwt = po["beam"], po["retry-beam"], po["acoustic-scale"]
    dry = po["dry-run"]
    tot = dict(done=0, err=0, retry=0, like=0.0, frames=0)
    state = dict(score=None, input_dim=None)

    def device():
        """The GPU and the scoring code of tools/latgen_faster.py, at the first batch."""
        if state["score"] is not None:
            return
        import torch  # noqa: F401
        kt.select_gpu(api, po)
        if kind == "nnet2":
            nnet = api.Nnet(comps, priors)
            state["input_dim"] = nnet.input_dim()
            state["score"] = lambda feats, off: nnet.compute(feats, off, pad_input=True, epilogue=True, prob_scale=acwt)[0]   # DecodableAmNnet
        else:
            gmm = kt.device_gmm(api, am)
            state["input_dim"] = am["dim"]

            def score(feats, off):        # DecodableAmDiagGmmScaled::LogLikelihood (decodable-am-diag-gmm.h:142-145)
                ll = gmm.pdf_log_likelihoods(feats)
                api.scale(ll, acwt)
                return ll
            state["score"] = score

    def flush(batch):
        if dry:
            return
        device()
        for utt, _, m in batch:
            if m.shape[1] != state["input_dim"]:
                raise cli.KaldiError("feature dimension %d of %s does not match the model's input %d" % (m.shape[1], utt, state["input_dim"]))
        off = np.concatenate([[0], np.cumsum([len(m) for _, _, m in batch])]).astype(np.int32)
        loglikes = state["score"](kt.stack_rows([m for _, _, m in batch]), off)
        res = api.align_compiled([g for _, g, _ in batch], loglikes, off, tm["tid2pdf"], beam, retry_beam, careful=po["careful"])
        for (utt, _, m), r in zip(batch, res):
            report(utt, len(m), r)

    def report(utt, num_frames, r):
        """decoder-wrappers.cc:462-504 behind the searches."""
        if r["retried"]:
            tot["retry"] += 1
            cli.warn("Retrying utterance %s with beam %g" % (utt, retry_beam), WHERE)
        if r["status"] in (api.ALIGNC_TOO_LARGE, api.ALIGNC_BOUND, api.ALIGNC_BAD_INPUT, api.ALIGNC_NEEDS_ROOM):
            cli.warn("The search of utterance %s ended with status %d (include/kaldi_hip.h, KH_ALIGNC_*)" % (utt, r["status"]), WHERE)
        if r["status"] != api.ALIGNC_DONE:
            cli.warn("Did not successfully decode file %s, len = %d" % (utt, num_frames), WHERE)
            tot["err"] += 1
            return
        neg = np.float32(-np.float32(r["weight"][0] + r["weight"][1]))
        like = np.float32(neg / np.float32(acwt))
        tot["done"] += 1
        tot["like"] += float(like)
        tot["frames"] += num_frames
        ali_w.write(utt, np.asarray(r["alignment"], np.int32))
        scores_w.write(utt, neg)

    def utterances():
        checked = False
        for utt, g in fst_reader:
            if not feature_reader.has_key(utt):
                tot["err"] += 1
                cli.warn("No features for utterance " + utt)
                continue
            m = feature_reader.value(utt)
            if m.shape[0] == 0:
                cli.warn("Zero-length utterance: " + utt)
                tot["err"] += 1
                continue
            g = api.add_transition_probs(g, tm, po["transition-scale"], po["self-loop-scale"])
            if not checked:
                check_beams(cli, beam, retry_beam)
                checked = True
            if int(g["num_states"]) == 0 or int(g["start"]) < 0:
                cli.warn("Empty decoding graph for " + utt, WHERE)
                tot["err"] += 1
                continue
            yield utt, g, m

    for batch in kt.batches(utterances(), lambda b: b[2].shape[0], po["batch-frames"], "after"):
        flush(batch)
    ok = ali_w.close()
    scores_w.close()
    per_frame = tot["like"] / tot["frames"] if tot["frames"] else float("nan")
    cli.log("Overall log-likelihood per frame is %g over %d frames." % (per_frame, tot["frames"]))
    cli.log("Retried %d out of %d utterances." % (tot["retry"], tot["done"] + tot["err"]))
    cli.log("Done %d, errors on %d" % (tot["done"], tot["err"]))
    if not ok:
        raise cli.KaldiError("error closing the alignment table " + ali_wspec)
    return 0 if tot["done"] != 0 else 1


if __name__ == "__main__":
    sys.exit(main())
