#!/usr/bin/env python3
"""The fMLLR stage of the speaker-adapted recipes on the MI355X path: the reference binaries' command lines over the library,
so that these lines of steps/align_fmllr.sh and steps/decode_fmllr.sh run unchanged with bin/ in front of PATH:

  ali-to-post "ark:gunzip -c $dir/pre_ali.JOB.gz|" ark:- | \\
    weight-silence-post $silence_weight $silphonelist $alimdl ark:- ark:- | \\
    gmm-post-to-gpost $alimdl "$sifeats" ark:- ark:- | \\
    gmm-est-fmllr-gpost --fmllr-update-type=$fmllr_update_type --spk2utt=ark:$sdata/JOB/spk2utt $mdl "$sifeats" ark,s,cs:- ark:$dir/trans.JOB
  ... | gmm-est-fmllr --fmllr-update-type=$fmllr_update_type --spk2utt=ark:$sdata/JOB/spk2utt $mdl "$feats" ark,s,cs:- ark:$dir/tmp_trans.JOB
  compose-transforms --b-is-affine=true ark:$dir/tmp_trans.JOB ark:$dir/pre_trans.JOB ark:$dir/trans.JOB
  feats="$sifeats transform-feats --utt2spk=ark:$sdata/JOB/utt2spk ark:$dir/trans.JOB ark:- ark:- |"

Programs and the sources they restate: ali-to-post (bin/ali-to-post.cc), weight-silence-post (bin/weight-silence-post.cc),
gmm-post-to-gpost (gmmbin/gmm-post-to-gpost.cc), gmm-est-fmllr (gmmbin/gmm-est-fmllr.cc), gmm-est-fmllr-gpost
(gmmbin/gmm-est-fmllr-gpost.cc), compose-transforms (featbin/compose-transforms.cc), transform-feats
(featbin/transform-feats.cc): their options, warnings, counts on stderr and exit status.

Differences from the binaries.  The estimators read the whole job's tables first and make one library pass over all speakers
(api.estimate_fmllr), so a speaker's log lines come after the last table is read; the per-frame entry order is ascending pdf
(api.convert_posterior_to_pdfs), where the reference's is its unordered_map's.  gmm-post-to-gpost --rand-prune > 0 is refused:
RandPrune's random stream is not reproduced.
--gpu (not a reference option): device ordinal, -1 = LOCAL_RANK, else 0.  Run through the tools/<name>.py wrappers."""
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
kt = importlib.import_module("old-kaldi-git_amd.kaldi_tool")

USAGE = {
    "ali-to-post": ("Convert alignments to posteriors\n"
                    "Usage:  ali-to-post [options] <alignments-rspecifier> <posteriors-wspecifier>\n"
                    "e.g.:\n"
                    " ali-to-post ark:1.ali ark:1.post\n"),
    "weight-silence-post": ("Apply weight to silences in posts\n"
                            "Usage:  weight-silence-post [options] <silence-weight> <silence-phones> <model> <posteriors-rspecifier> "
                            "<posteriors-wspecifier>\n"
                            "e.g.:\n"
                            " weight-silence-post 0.0 1:2:3 1.mdl ark:1.post ark:nosil.post\n"),
    "gmm-post-to-gpost": ("Convert state-level posteriors to Gaussian-level posteriors\n"
                          "Usage:  gmm-post-to-gpost [options] <model-in> <feature-rspecifier> <posteriors-rspecifier> <gpost-wspecifier>\n"
                          "e.g.: \n"
                          " gmm-post-to-gpost 1.mdl scp:train.scp ark:1.post ark:1.gpost\n"
                          "[MI355X] --rand-prune > 0 is not supported: RandPrune's random stream is not reproduced.\n"),
    "gmm-est-fmllr": ("Estimate global fMLLR transforms, either per utterance or for the supplied\n"
                      "set of speakers (spk2utt option).  Reads posteriors (on transition-ids).  Writes\n"
                      "to a table of matrices.\n"
                      "Usage: gmm-est-fmllr [options] <model-in> <feature-rspecifier> <post-rspecifier> <transform-wspecifier>\n"),
    "gmm-est-fmllr-gpost": ("Estimate global fMLLR transforms, either per utterance or for the supplied\n"
                            "set of speakers (spk2utt option).  Reads Gaussian-level posteriors.  Writes\n"
                            "to a table of matrices.\n"
                            "Usage: gmm-est-fmllr-gpost [options] <model-in> <feature-rspecifier> <gpost-rspecifier> <transform-wspecifier>\n"),
    "compose-transforms": ("Compose (affine or linear) feature transforms\n"
                           "Usage: compose-transforms [options] (<transform-A-rspecifier>|<transform-A-rxfilename>) "
                           "(<transform-B-rspecifier>|<transform-B-rxfilename>) (<transform-out-wspecifier>|<transform-out-wxfilename>)\n"
                           " Note: it does matrix multiplication (A B) so B is the transform that gets applied\n"
                           "  to the features first.  If b-is-affine = true, then assume last column of b corresponds to offset\n"
                           " e.g.: compose-transforms 1.mat 2.mat 3.mat\n"
                           "   compose-transforms 1.mat ark:2.trans ark:3.trans\n"
                           "   compose-transforms ark:1.trans ark:2.trans ark:3.trans\n"
                           " See also: transform-feats, transform-vec, extend-transform-dim, est-lda, est-pca\n"),
    "transform-feats": ("Apply transform (e.g. LDA; HLDA; fMLLR/CMLLR; MLLT/STC)\n"
                        "Linear transform if transform-num-cols == feature-dim, affine if\n"
                        "transform-num-cols == feature-dim+1 (->append 1.0 to features)\n"
                        "Per-utterance by default, or per-speaker if utt2spk option provided\n"
                        "Global if transform-rxfilename provided.\n"
                        "Usage: transform-feats [options] (<transform-rspecifier>|<transform-rxfilename>) <feats-rspecifier> <feats-wspecifier>\n"
                        "See also: transform-vec, copy-feats, compose-transforms\n"),
}


def main(argv=None, prog="gmm-est-fmllr"):
    return kt.run_tool(prog, lambda cli, argv: RUN[prog](cli, argv, prog), argv, kt.KALDI_KH)


def _api():
    return importlib.import_module("old-kaldi-git_amd.api")


def _kio():
    return importlib.import_module("old-kaldi-git_amd.kaldi_io")


def _is_rspecifier(cli, s):
    return cli.classify_rspecifier(s)[0] is not None


def _read_token_map(cli, rspecifier):
    """RandomAccessTokenReader on an utt2spk table: key -> first token."""
    return {k: v[0] for k, v in cli.SequentialTableReader(rspecifier, "token_vector") if v}


# ---------------------------------------------------------------- ali-to-post
def run_ali_to_post(cli, argv, prog):
    po = kt.parse(cli, prog, USAGE[prog], argv, None, 2)
    if po is None:
        return 1
    reader = cli.SequentialTableReader(po.get_arg(1), "int32_vector")
    writer = cli.TableWriter(po.get_arg(2), "posterior")
    n = 0
    for key, ali in reader:
        n += 1
        writer.write(key, [[(int(t), 1.0)] for t in ali])          # AlignmentToPosterior hmm/posterior.cc:276-285
    writer.close()
    cli.log("Converted %d alignments." % n)
    return 0 if n != 0 else 1


# ---------------------------------------------------------------- weight-silence-post
def run_weight_silence_post(cli, argv, prog):
    po = kt.parse(cli, prog, USAGE[prog], argv, lambda po: po.register(
        "distribute", False, "If true, rather than weighting the individual posteriors, apply the weighting to the whole frame: "
        "i.e. on time t, scale all posterior entries by p(sil)*silence-weight + p(non-sil)*1.0"), 5)
    if po is None:
        return 1
    kio = _kio()
    try:
        weight = float(po.get_arg(1))
    except ValueError:
        raise cli.KaldiError('Invalid silence-weight parameter: expected float, got "%s"' % po.get_arg(1))
    try:
        phones = [int(x) for x in po.get_arg(2).split(":")] if po.get_arg(2) != "" else []
    except ValueError:
        raise cli.KaldiError("Invalid silence-phones string " + po.get_arg(2))
    if not phones:
        cli.warn("No silence phones, this will have no effect")
    tm = cli.read_kaldi_object(po.get_arg(3), kio.read_transition_model)
    reader = cli.SequentialTableReader(po.get_arg(4), "posterior")
    writer = cli.TableWriter(po.get_arg(5), "posterior")
    api = _api()
    n = 0
    for key, post in reader:
        n += 1
        writer.write(key, api.weight_silence_post(tm["tid2phone"], phones, weight, post, distribute=po["distribute"]))
    writer.close()
    cli.log("Done %d posteriors." % n)
    return 0 if n != 0 else 1


# ---------------------------------------------------------------- gmm-post-to-gpost
def run_gmm_post_to_gpost(cli, argv, prog):
    def register(po):
        po.register("binary", True, "Write output in binary mode")
        po.register("rand-prune", 0.0, "Randomized pruning of posteriors less than this [MI355X: only 0 is supported]", float)
        po.register("batch-frames", 200000, "[MI355X] frames per library call", int)
        kt.register_gpu(po)
    po = kt.parse(cli, prog, USAGE[prog], argv, register, 4)
    if po is None:
        return 1
    if po["rand-prune"] > 0.0:
        raise cli.KaldiError("--rand-prune=%g: RandPrune's random stream is not reproduced here; only --rand-prune=0 is supported" % po["rand-prune"])
    tm, am = kt.read_gmm_model(cli, _kio(), po.get_arg(1))
    feature_reader = cli.SequentialTableReader(po.get_arg(2), "matrix")
    post_reader = cli.RandomAccessTableReader(po.get_arg(3), "posterior")
    writer = cli.TableWriter(po.get_arg(4), "gauss_post")
    api = _api()
    tot = dict(done=0, no_post=0, err=0, like=0.0, t=0.0)
    state = {}

    def flush(batch):
        if "gmm" not in state:
            kt.select_gpu(api, po)
            state["gmm"] = kt.device_gmm(api, am)
        posts = [fr for _, _, p in batch for fr in p]
        gposts, like, weight = api.gmm_post_to_gpost(state["gmm"], kt.stack_rows([m for _, m, _ in batch]), posts)
        feo = np.concatenate([[0], np.cumsum([len(fr) for fr in posts])])
        t0 = 0
        for key, m, p in batch:
            e0, e1 = int(feo[t0]), int(feo[t0 + len(p)])
            like_file, w_file = np.float32(0.0), np.float32(0.0)
            for e in range(e0, e1):                                    # tot_like_this_file += like * weight (floats) :112-113
                like_file = np.float32(like_file + np.float32(like[e] * weight[e]))
                w_file = np.float32(w_file + weight[e])
            tot["like"] += float(like_file)
            tot["t"] += float(w_file)
            writer.write(key, gposts[t0:t0 + len(p)])
            t0 += len(p)

    def utterances():
        for key, mat in feature_reader:
            if not post_reader.has_key(key):
                tot["no_post"] += 1
                continue
            post = post_reader.value(key)
            if len(post) != mat.shape[0]:
                cli.warn("Posterior vector has wrong size %d vs. %d" % (len(post), mat.shape[0]))
                tot["err"] += 1
                continue
            tot["done"] += 1
            if mat.shape[0] == 0:
                writer.write(key, [])
                continue
            if mat.shape[1] != am["dim"]:
                raise cli.KaldiError("DiagGmm::ComponentLogLikelihood, dimension mismatch %d vs. %d" % (mat.shape[1], am["dim"]))
            yield key, mat, api.convert_posterior_to_pdfs(tm["tid2pdf"], post)

    for batch in kt.batches(utterances(), lambda b: b[1].shape[0], po["batch-frames"], "after"):
        flush(batch)
    writer.close()
    cli.log("Done %d files, %d with no posteriors, %d with other errors." % (tot["done"], tot["no_post"], tot["err"]))
    cli.log("Overall avg like per frame (Gaussian only) = %g over %g frames." % (tot["like"] / tot["t"] if tot["t"] else float("nan"), tot["t"]))
    cli.log("Done converting post to gpost")
    return 0 if tot["done"] != 0 else 1


# ---------------------------------------------------------------- gmm-est-fmllr, gmm-est-fmllr-gpost
def run_est_fmllr(cli, argv, prog):
    gpost = prog == "gmm-est-fmllr-gpost"
    what = "gposts" if gpost else "posts"

    def register(po):
        po.register("spk2utt", "", "rspecifier for speaker to utterance-list map")
        po.register("fmllr-update-type", "full", 'Update type for fMLLR ("full"|"diag"|"offset"|"none")')
        po.register("fmllr-min-count", 500.0, "Minimum count required to update fMLLR", float)
        po.register("fmllr-num-iters", 40, "Number of iterations in fMLLR update phase.", int)
        kt.register_gpu(po)
    po = kt.parse(cli, prog, USAGE[prog], argv, register, 4)
    if po is None:
        return 1
    tm, am = kt.read_gmm_model(cli, _kio(), po.get_arg(1))
    post_reader = cli.RandomAccessTableReader(po.get_arg(3), "gauss_post" if gpost else "posterior")
    writer = cli.TableWriter(po.get_arg(4), "matrix")
    api = _api()
    opts = api.fmllr_options(po["fmllr-update-type"], po["fmllr-min-count"], po["fmllr-num-iters"])
    if opts["update_type"] not in ("full", "diag", "offset", "none"):
        raise cli.KaldiError('Unknown fMLLR update type %s, fmllr-update-type must be one of "full"|"diag"|"offset"|"none"' % opts["update_type"])
    n = dict(done=0, no_post=0, err=0)
    names, spk_utts, mats, posts = [], [0], [], []          # speakers in order; utterances stacked in speaker order

    def take(utt, feats, post):
        if len(post) != feats.shape[0]:
            if gpost:
                cli.warn("GaussPost %s wrong size %d vs. %d" % ("vector has" if po["spk2utt"] else "has", len(post), feats.shape[0]))
            else:
                cli.warn("Posterior %s wrong size %d vs. %d" % ("vector has" if po["spk2utt"] else "has", len(post), feats.shape[0]))
            n["err"] += 1
            return
        n["done"] += 1
        if feats.shape[0] == 0:
            return
        if feats.shape[1] != am["dim"]:
            raise cli.KaldiError("feature dimension %d of %s does not match the model's %d" % (feats.shape[1], utt, am["dim"]))
        mats.append(feats)
        posts.extend(post)

    if po["spk2utt"] != "":
        feature_reader = cli.RandomAccessTableReader(po.get_arg(2), "matrix")
        for spk, uttlist in cli.SequentialTableReader(po["spk2utt"], "token_vector"):
            for utt in uttlist:
                if not feature_reader.has_key(utt):
                    cli.warn("Did not find features for utterance " + utt)
                    n["err"] += 1
                    continue
                if not post_reader.has_key(utt):
                    cli.warn("Did not find posteriors for utterance " + utt)
                    n["no_post"] += 1
                    continue
                take(utt, feature_reader.value(utt), post_reader.value(utt))
            names.append(spk)
            spk_utts.append(len(mats))
    else:
        for utt, feats in cli.SequentialTableReader(po.get_arg(2), "matrix"):
            if not post_reader.has_key(utt):
                cli.warn("Did not find %s for utterance %s" % (what, utt))
                n["no_post"] += 1
                continue
            before = n["done"]
            take(utt, feats, post_reader.value(utt))
            if n["done"] != before:
                names.append(utt)
                spk_utts.append(len(mats))
    D = am["dim"]
    S = len(names)
    W = np.tile(np.eye(D, D + 1, dtype=np.float32), (S, 1, 1))
    impr, count, beta = np.zeros(S, np.float32), np.zeros(S, np.float32), np.zeros(S, np.float64)
    if mats:
        kt.select_gpu(api, po)
        gmm = kt.device_gmm(api, am)
        utt_rows = np.concatenate([[0], np.cumsum([len(m) for m in mats])]).astype(np.int32)
        kw = dict(gposts=posts) if gpost else dict(posts=posts, tid2pdf=tm["tid2pdf"])
        W, impr, count, stats = api.estimate_fmllr(gmm, kt.stack_rows(mats), utt_rows, np.asarray(spk_utts, np.int32), opts=opts, return_stats=True, **kw)
        beta = stats["beta"]
        t = api.fmllr_last_timings()
        cli.vlog(1, "component posteriors %.3f ms, frame stats %.3f ms, accumulate %.3f ms, update %.3f ms" % (
            t["component_posteriors_ms"], t["frame_stats_ms"], t["accumulate_ms"], t["update_ms"]))
    tot_impr = tot_t = 0.0
    label = "speaker" if po["spk2utt"] != "" else ("utterancer" if gpost else "utterance")
    for s, name in enumerate(names):
        if not float(beta[s]) > float(np.float32(opts["min_count"])):     # the library's own test (:144): the double beta
            cli.warn("Not updating fMLLR since below min-count: count is %g" % count[s], "Update()")
        writer.write(name, W[s])
        with np.errstate(invalid="ignore", divide="ignore"):
            per = np.float32(impr[s]) / np.float32(count[s])
        cli.log("For %s %s, auxf-impr from fMLLR is %g, over %g frames." % (label, name, per, count[s]))
        tot_impr += float(impr[s])
        tot_t += float(count[s])
    ok = writer.close()
    cli.log("Done %d files, %d with no %s, %d with other errors." % (n["done"], n["no_post"], what, n["err"]))
    cli.log("Overall fMLLR auxf impr per frame is %g over %g frames." % (tot_impr / tot_t if tot_t else float("nan"), tot_t))
    if not ok:
        raise cli.KaldiError("error closing the transform table " + po.get_arg(4))
    return 0 if n["done"] != 0 else 1


# ---------------------------------------------------------------- compose-transforms
def run_compose_transforms(cli, argv, prog):
    def register(po):
        po.register("utt2spk", "", "rspecifier for utterance to speaker map (if mixing utterance and speaker ids)")
        po.register("b-is-affine", False, "If true, treat last column of transform b as an offset term (only relevant if a is affine)")
        po.register("binary", True, "Write in binary mode (only relevant if output is a wxfilename)")
    po = kt.parse(cli, prog, USAGE[prog], argv, register, 3)
    if po is None:
        return 1
    kio = _kio()
    api = _api()
    a_fn, b_fn, c_fn = po.get_arg(1), po.get_arg(2), po.get_arg(3)
    a_rs, b_rs = _is_rspecifier(cli, a_fn), _is_rspecifier(cli, b_fn)
    c_ws = cli.classify_wspecifier(c_fn)[0] is not None
    aff = po["b-is-affine"]
    utt2spk = None
    if po["utt2spk"] != "":
        if not (a_rs and b_rs):
            raise cli.KaldiError("Error: utt2spk option provided compose transforms but at least one of the inputs is a global transform.")
        utt2spk = _read_token_map(cli, po["utt2spk"])
    if (a_rs or b_rs) != c_ws:
        raise cli.KaldiError("Formats of the input and output rspecifiers/rxfilenames do not match (if either a or b is an rspecifier, "
                             "then the output must be a wspecifier.")

    def compose(a, b):
        c = api.compose_transforms(a, b, aff)
        if c is None:
            cli.warn("Empty matrix in ComposeTransforms", "ComposeTransforms()")
        return c

    read_mat = lambda fn: cli.read_kaldi_object(fn, kio.read_matrix)
    if not (a_rs or b_rs):
        a, b = read_mat(a_fn), read_mat(b_fn)
        if not aff and a.shape[0] == a.shape[1] + 1 and a.shape[0] == b.shape[0] and a.shape[1] == b.shape[1]:
            cli.warn("It looks like you are trying to compose two affine transforms, but you omitted the --b-is-affine option.")
        c = compose(a, b)
        if c is None:
            return 1
        cli.write_kaldi_object(c_fn, po["binary"], lambda f: kio.write_matrix(f, c, po["binary"]))
        return 0
    writer = cli.TableWriter(c_fn, "matrix")
    if a_rs and b_rs:
        b_reader = cli.RandomAccessTableReader(b_fn, "matrix")
        for key, a in cli.SequentialTableReader(a_fn, "matrix"):
            if utt2spk is not None:
                if key not in utt2spk:
                    cli.warn("No speaker provided for utterance %s (perhaps you wrongly provided utt2spk option to  compose-transforms?)" % key)
                    continue
                if not b_reader.has_key(utt2spk[key]):
                    cli.warn("Second table does not have key " + utt2spk[key])
                    continue
            elif not b_reader.has_key(key):
                cli.warn("Second table does not have key " + key)
                continue
            c = compose(a, b_reader.value(key))        # (the reference looks b up by the utterance key in both branches)
            if c is not None:
                writer.write(key, c)
    elif a_rs:
        b = read_mat(b_fn)
        for key, a in cli.SequentialTableReader(a_fn, "matrix"):
            c = compose(a, b)
            if c is not None:
                writer.write(key, c)
    else:
        a = read_mat(a_fn)
        for key, b in cli.SequentialTableReader(b_fn, "matrix"):
            c = compose(a, b)
            if c is not None:
                writer.write(key, c)
    writer.close()
    return 0


# ---------------------------------------------------------------- transform-feats
def run_transform_feats(cli, argv, prog):
    def register(po):
        po.register("utt2spk", "", "rspecifier for utterance to speaker map")
        po.register("batch-frames", 200000, "[MI355X] frames per device pass", int)
        kt.register_gpu(po)
    po = kt.parse(cli, prog, USAGE[prog], argv, register, 3)
    if po is None:
        return 1
    kio = _kio()
    api = _api()
    t_fn = po.get_arg(1)
    glob = None
    if not _is_rspecifier(cli, t_fn):
        glob = cli.read_kaldi_object(t_fn, kio.read_matrix)
        lookup = lambda utt: glob
    else:
        table = cli.RandomAccessTableReader(t_fn, "matrix")
        utt2spk = _read_token_map(cli, po["utt2spk"]) if po["utt2spk"] != "" else None

        def lookup(utt):                       # RandomAccessTableReaderMapped: the key goes through utt2spk first
            key = utt if utt2spk is None else utt2spk.get(utt)
            return table.value(key) if key is not None and table.has_key(key) else None
    writer = cli.TableWriter(po.get_arg(3), "matrix")
    n = dict(done=0, err=0)
    state = {}
    ld = dict(type=None, t=0.0, tot=0.0, cache={})

    def logdet_stats(tr, feat):
        """transform-feats.cc:121-154: 1/2 logdet(T T^T) of the linear part, weighted by frames (float, as SpMatrix<BaseFloat>)."""
        dim = feat.shape[1]
        if ld["type"] is None:
            ld["type"] = "logdet" if tr.shape[0] == dim else ("pseudo" if tr.shape[0] < dim else "increase")
        if ld["type"] == "increase":
            return
        if id(tr) not in ld["cache"]:
            lin = np.asarray(tr[:, :dim], np.float32)
            sign, val = np.linalg.slogdet((lin @ lin.T).astype(np.float64))
            ld["cache"][id(tr)] = (tr, np.float32(0.5) * np.float32(val) if sign > 0 else np.float32("nan"))
        v = ld["cache"][id(tr)][1]
        if v != v or np.isinf(v):
            cli.warn("Matrix has bad logdet %g" % v)
        else:
            ld["t"] += feat.shape[0]
            ld["tot"] += feat.shape[0] * float(v)

    def flush(batch):
        """One device matrix per distinct transform of the batch; the utterances that share it go through one product."""
        if not batch:
            return
        import torch
        if "gpu" not in state:
            kt.select_gpu(api, po)
            state["gpu"] = True
        out = {}
        groups = {}
        for i, (utt, feat, tr) in enumerate(batch):
            groups.setdefault(id(tr), (tr, []))[1].append(i)
        for tr, idx in groups.values():
            x = kt.stack_rows([batch[i][1] for i in idx])
            y = api.transform_feats(torch.from_numpy(np.ascontiguousarray(tr, dtype=np.float32)).cuda(), x).cpu().numpy()
            r = 0
            for i in idx:
                out[i] = y[r:r + len(batch[i][1])]
                r += len(batch[i][1])
        for i, (utt, _, _) in enumerate(batch):
            writer.write(utt, out[i])

    batch, frames = [], 0
    for utt, feat in cli.SequentialTableReader(po.get_arg(2), "matrix"):
        tr = lookup(utt)
        if tr is None:
            cli.warn("No fMLLR transform available for utterance %s, producing no output for this utterance" % utt)
            n["err"] += 1
            continue
        if tr.shape[1] not in (feat.shape[1], feat.shape[1] + 1):
            cli.warn("Transform matrix for utterance %s has bad dimension %dx%d versus feat dim %d" % (utt, tr.shape[0], tr.shape[1], feat.shape[1]))
            if tr.shape[1] == feat.shape[1] + 2:
                cli.warn("[perhaps the transform was created by compose-transforms, and you forgot the --b-is-affine option?]")
            n["err"] += 1
            continue
        n["done"] += 1
        logdet_stats(tr, feat)
        if feat.shape[0] == 0:
            flush(batch)
            batch, frames = [], 0
            writer.write(utt, np.zeros((0, tr.shape[0]), np.float32))
            continue
        batch.append((utt, feat, tr))
        frames += feat.shape[0]
        if frames >= po["batch-frames"]:
            flush(batch)
            batch, frames = [], 0
    flush(batch)
    writer.close()
    if ld["type"] in ("logdet", "pseudo"):
        cli.log("Overall average %slogdet is %g over %g frames." % ("[pseudo-]" if ld["type"] == "pseudo" else "",
                                                                  ld["tot"] / ld["t"] if ld["t"] else float("nan"), ld["t"]))
    cli.log("Applied transform to %d utterances; %d had errors." % (n["done"], n["err"]))
    return 0 if n["done"] != 0 else 1


RUN = {"ali-to-post": run_ali_to_post, "weight-silence-post": run_weight_silence_post, "gmm-post-to-gpost": run_gmm_post_to_gpost,
       "gmm-est-fmllr": run_est_fmllr, "gmm-est-fmllr-gpost": run_est_fmllr, "compose-transforms": run_compose_transforms,
       "transform-feats": run_transform_feats}
