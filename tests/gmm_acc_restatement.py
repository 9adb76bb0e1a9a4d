"""The E-step of GMM training restated line by line in numpy: gmm-acc-stats-ali, gmm-acc-stats and gmm-acc-stats-twofeats
(gmmbin/*.cc) over AccumAmDiagGmm::AccumulateForGmm / AccumulateForGmmTwofeats (gmm/mle-am-diag-gmm.cc:69-97),
AccumDiagGmm::AccumulateFromDiag (gmm/mle-diag-gmm.cc:191-204) and AccumulateFromPosteriors (:171-189); gmm-sum-accs
(gmmbin/gmm-sum-accs.cc) over the Read(..., add = true) of both classes.  float32 where the reference is float, float64 where
it is double; entries are visited in frame order, a frame's entries in the order given (ascending pdf by the rule of
api.convert_posterior_to_pdfs; the reference's is its unordered_map's).  The Gaussian posteriors are
fmllr_restatement.component_posteriors' (DiagGmm::ComponentPosteriors times the weight).  The rank-one updates
(AddVecVec: the reference's BLAS dger) are numpy outer products added frame by frame: one rounding for the product p x^2
(p x is exact in double), one for each addition.

An accumulator is kaldi_io's dict: occ [NG], mean_acc / var_acc [NG, D] float64 or None, pdf_offsets, dim, flags (the augmented GmmFlagsType: m 1, v 2,
w 4, t 8), total_like, total_frames, transition_accs."""
import numpy as np

import fmllr_restatement as R

F32, F64 = np.float32, np.float64
kGmmMeans, kGmmVariances, kGmmWeights, kGmmTransitions, kGmmAll = 1, 2, 4, 8, 15


def augment_flags(flags):
    """StringToGmmFlags (gmm/model-common.cc:26-41) for a string, then AugmentGmmFlags (:52-62) as written: only valid bits,
    v adds m, m adds w, w is added to empty flags; the transition bit stays ("mvwt" and kGmmAll: 15)."""
    bits = 0
    if isinstance(flags, str):
        for c in flags:
            bits |= {"m": kGmmMeans, "v": kGmmVariances, "w": kGmmWeights, "t": kGmmTransitions, "a": kGmmAll}[c]
    else:
        bits = int(flags)
    assert (bits & ~kGmmAll) == 0                     # KALDI_ASSERT((flags & ~kGmmAll) == 0)
    if bits & kGmmVariances:
        bits |= kGmmMeans
    if bits & kGmmMeans:
        bits |= kGmmWeights
    if not bits & kGmmWeights:
        bits |= kGmmWeights                           # "Adding in kGmmWeights ("w") to empty flags."
    return bits


def init_accs(pdf_offsets, dim, flags):
    """AccumAmDiagGmm::Init (mle-am-diag-gmm.cc:41-61) over AccumDiagGmm::Resize (mle-diag-gmm.cc:106-120)."""
    off = np.asarray(pdf_offsets, np.int32)
    bits = augment_flags(flags)
    ng = int(off[-1])
    return dict(occ=np.zeros(ng, F64), mean_acc=np.zeros((ng, dim), F64) if bits & kGmmMeans else None,
                var_acc=np.zeros((ng, dim), F64) if bits & kGmmVariances else None, pdf_offsets=off, dim=int(dim), flags=bits,
                total_like=0.0, total_frames=0.0, transition_accs=None)


def accumulate_from_posteriors(acc, pdf, data, posteriors):
    """AccumDiagGmm::AccumulateFromPosteriors (mle-diag-gmm.cc:171-189) on the accumulator of `pdf`."""
    g0, g1 = int(acc["pdf_offsets"][pdf]), int(acc["pdf_offsets"][pdf + 1])
    assert len(posteriors) == g1 - g0
    post_d = np.asarray(posteriors, F32).astype(F64)                  # Vector<double> post_d(posteriors)
    acc["occ"][g0:g1] += post_d                                       # occupancy_.AddVec(1.0, post_d)
    if acc["flags"] & kGmmMeans:
        assert len(data) == acc["dim"]
        data_d = np.asarray(data, F32).astype(F64)                    # Vector<double> data_d(data)
        acc["mean_acc"][g0:g1] += np.outer(post_d, data_d)            # mean_accumulator_.AddVecVec(1.0, post_d, data_d)
        if acc["flags"] & kGmmVariances:
            data_d = data_d * data_d                                  # data_d.ApplyPow(2.0)
            acc["var_acc"][g0:g1] += np.outer(post_d, data_d)         # variance_accumulator_.AddVecVec(1.0, post_d, data_d)


def accumulate_entries(acc, stats_feats, ent, gauss_post, like=None):
    """Every entry of a CSR entry list in frame order: AccumulateFromPosteriors with the given Gaussian posteriors (already
    times the weight) on the row of stats_feats; with `like`, also total_log_like_ += fl32(log_like * weight) and
    total_frames_ += weight (mle-am-diag-gmm.cc:76-77, :94-95)."""
    for t in range(len(ent["feo"]) - 1):
        for e in range(int(ent["feo"][t]), int(ent["feo"][t + 1])):
            accumulate_from_posteriors(acc, int(ent["pdf"][e]), stats_feats[t], gauss_post[int(ent["goff"][e]):int(ent["goff"][e + 1])])
            if like is not None:
                acc["total_like"] += float(F32(F32(like[e]) * F32(ent["weight"][e])))
                acc["total_frames"] += float(F32(ent["weight"][e]))
    return acc


def accumulate_for_gmm(acc, am, feats, pdf_posts, stats_feats=None):
    """AccumulateForGmm (stats_feats None) / AccumulateForGmmTwofeats for every (frame, pdf, weight) -> (acc, ent, like, post)."""
    ent = R.entries_of(pdf_posts, am["pdf_offsets"])
    post, like = R.component_posteriors(am, feats, ent)
    accumulate_entries(acc, feats if stats_feats is None else stats_feats, ent, post, like)
    return acc, ent, like, post


def transition_accumulate(stats, tid, prob):
    stats[tid] += float(F32(prob))                                   # TransitionModel::Accumulate: (*stats)(tid) += prob


def acc_stats_ali(am, tid2pdf, utts):
    """gmm-acc-stats-ali.cc:64-122.  utts: [(features [T, D], alignment [T])].  -> (acc, tot_like, tot_t)."""
    acc = init_accs(am["pdf_offsets"], am["means_invvars"].shape[1], kGmmAll)
    acc["transition_accs"] = np.zeros(len(tid2pdf), F64)             # InitStats: NumTransitionIds() + 1
    tot_like, tot_t = 0.0, 0
    for mat, ali in utts:
        _, _, like, _ = accumulate_for_gmm(acc, am, mat, [[(int(tid2pdf[t]), 1.0)] for t in ali])
        tot_like_this_file = F32(0.0)
        for i, tid in enumerate(ali):
            transition_accumulate(acc["transition_accs"], int(tid), 1.0)
            tot_like_this_file = F32(tot_like_this_file + like[i])
        tot_like += float(tot_like_this_file)
        tot_t += len(ali)
    return acc, tot_like, tot_t


def convert_posterior_to_pdfs(tid2pdf, post):
    """ConvertPosteriorToPdfs hmm/posterior.cc:308-332, ascending pdf order."""
    out = []
    for fr in post:
        m = {}
        for tid, w in fr:
            pdf = int(tid2pdf[tid])
            m[pdf] = F32(m[pdf] + F32(w)) if pdf in m else F32(w)
        out.append([(k, float(v)) for k, v in sorted(m.items()) if v != 0.0])
    return out


def acc_stats(am, tid2pdf, utts, flags="mvwt", twofeats=False):
    """gmm-acc-stats.cc:70-141 (utts: [(features, posterior)]) and gmm-acc-stats-twofeats.cc:70-162 (utts: [(features1,
    features2, posterior)], flags kGmmAll, the accumulators of features2's dimension).  -> (acc, tot_like, tot_t)."""
    dim = utts[0][1].shape[1] if twofeats else am["means_invvars"].shape[1]
    acc = init_accs(am["pdf_offsets"], dim, kGmmAll if twofeats else flags)
    acc["transition_accs"] = np.zeros(len(tid2pdf), F64)
    tot_like, tot_t = 0.0, 0.0
    for u in utts:
        mat, mat2, post = (u[0], u[1], u[2]) if twofeats else (u[0], None, u[1])
        _, ent, like, _ = accumulate_for_gmm(acc, am, mat, convert_posterior_to_pdfs(tid2pdf, post), mat2)
        tot_like_this_file, tot_weight = F32(0.0), F32(0.0)
        for e in range(len(like)):
            tot_like_this_file = F32(tot_like_this_file + F32(like[e] * ent["weight"][e]))
            tot_weight = F32(tot_weight + ent["weight"][e])
        for fr in post:
            for tid, w in fr:
                transition_accumulate(acc["transition_accs"], int(tid), w)
        tot_like += float(tot_like_this_file)
        tot_t += float(tot_weight)
    return acc, tot_like, tot_t


def as_written(acc):
    """What a file holds: AccumDiagGmm::Write converts to float (mle-diag-gmm.cc:86-94); the totals and the transition
    accumulators stay double."""
    f = lambda a: None if a is None else a.astype(F32)
    return dict(acc, occ=f(acc["occ"]), mean_acc=f(acc["mean_acc"]), var_acc=f(acc["var_acc"]))


def sum_accs(files):
    """gmm-sum-accs.cc:45-61: the files' floats added into doubles in argument order (Read with add = true)."""
    out = None
    for a in files:
        w = as_written(a)
        if out is None:
            out = dict(w, occ=w["occ"].astype(F64), mean_acc=None if w["mean_acc"] is None else w["mean_acc"].astype(F64),
                       var_acc=None if w["var_acc"] is None else w["var_acc"].astype(F64),
                       transition_accs=np.array(w["transition_accs"], F64))
        else:
            for k in ("occ", "mean_acc", "var_acc", "transition_accs"):
                if out[k] is not None:
                    out[k] = out[k] + w[k].astype(F64)
            out["total_like"] += w["total_like"]
            out["total_frames"] += w["total_frames"]
    return out
