"""Gaussian selection and the global GMM accumulation restated line by line in numpy: float32 where the reference is float,
float64 where it is double, frames in order.

What is restated, and the reference lines:
  log_likelihoods_preselect     DiagGmm::LogLikelihoodsPreselect gmm/diag-gmm.cc:566-598 (and LogLikelihoods :528-562 when no
                                list is given)
  select                        the body the three selection functions share: nth_element, >= thresh, std::sort by
                                std::greater<pair<float, int32>>, the first n, LogAdd from -inf
  gaussian_selection_frame      DiagGmm::GaussianSelection(const VectorBase&, ...) :765-799
  gaussian_selection            DiagGmm::GaussianSelection(const MatrixBase&, ...) :801-871, with the max_mem split :807-830
  gaussian_selection_preselect  DiagGmm::GaussianSelectionPreselect :875-916
  global_acc_stats              the frame loop of gmm-global-acc-stats.cc:117-139, both branches, over
                                AccumDiagGmm::AccumulateForComponent (gmm/mle-diag-gmm.cc:140-156) and AccumulateFromDiag
                                (:191-204)

Two modes, as the other restatements have:
  "library"    the scores are the library's k-ordered fmaf chains, ll = (g + a1) + (-0.5f * a2), for a contiguous and for a
               scattered list alike; Exp, Log and Log1p are the float of the float64 function.  What kh_gmm_gselect and
               kh_gmm_preselect_posteriors are held to bit for bit.
  "reference"  the scores are accumulated in float64 and rounded to float once (the reference's order is its BLAS's; this is
               the order-free statement of it).  What the recorded output of the reference's own code is compared with.

A frame with a NaN score: the reference's nth_element has no defined result; the library gives no selection and status 1, and
so does this file.  A model is dict(gconsts [G], means_invvars [G, D], inv_vars [G, D]) float32."""
import math

import numpy as np

import fmllr_restatement as FR

F32, F64 = np.float32, np.float64
MIN_LOG_DIFF_FLOAT = F32(math.log(2.0 ** -23))      # kMinLogDiffFloat = Log(FLT_EPSILON), base/kaldi-math.h:121
MAX_MEM = 10000000                                 # diag-gmm.cc:807


def log_add(x, y):
    """LogAdd(float, float), base/kaldi-math.h:198-215."""
    x, y = F32(x), F32(y)
    with np.errstate(invalid="ignore"):
        if x < y:
            diff = F32(x - y)
            x = y
        else:
            diff = F32(y - x)
        if diff >= MIN_LOG_DIFF_FLOAT:
            e = F32(math.exp(float(diff)))                       # Exp(diff)
            return F32(x + F32(math.log1p(float(e))))            # x + Log1p(...)
    return x


def reference_scored(indices):
    """The Gaussians DiagGmm::LogLikelihoodsPreselect actually scores for a list (diag-gmm.cc:575-586): its test for "the
    indices form a contiguous range" looks at the first and the last index only, so a list like [3, 9, 5, 6] (6 + 1 - 3 == 4)
    takes the range branch and position j gets the score of Gaussian front + j, whatever the list holds there.  The lists
    gmm-gselect writes are ordered by score, so this happens to an unlucky frame now and then.  Reference mode restates it;
    the library scores the Gaussians the list names, always."""
    idx = np.asarray(indices, np.int64)
    if int(idx[-1]) + 1 - int(idx[0]) == len(idx):
        return int(idx[0]) + np.arange(len(idx))
    return idx


def log_likelihoods_preselect(gmm, x, indices=None, mode="library"):
    """The scores of the listed Gaussians (all of them without a list), float32, in list order."""
    g, mi, iv = (np.asarray(gmm[k], F32) for k in ("gconsts", "means_invvars", "inv_vars"))
    idx = np.arange(len(g)) if indices is None else np.asarray(indices, np.int64)
    x = np.asarray(x, F32)
    if mode == "library":
        return FR.scores(x, g[idx], mi[idx], iv[idx])
    assert mode == "reference"
    if indices is not None:
        idx = reference_scored(idx)
    xd = x.astype(F64)
    xx = (x * x).astype(F32).astype(F64)                         # data_sq.ApplyPow(2.0) on the float copy
    with np.errstate(invalid="ignore", over="ignore"):
        return (g[idx].astype(F64) + mi[idx].astype(F64) @ xd - 0.5 * (iv[idx].astype(F64) @ xx)).astype(F32)


def select(loglikes, ids, num_gselect):
    """-> (output list, tot_loglike float32).  loglikes float32, ids the Gaussian of every position; num_gselect <= len."""
    n_all = len(loglikes)
    if num_gselect < n_all:
        thresh = np.sort(loglikes)[n_all - num_gselect]          # nth_element(ptr, ptr + num_gauss - num_gselect, ...)
    else:
        thresh = F32(-np.inf)
    pairs = [(F32(loglikes[p]), int(ids[p])) for p in range(n_all) if loglikes[p] >= thresh]
    pairs.sort(reverse=True)                                     # std::greater<std::pair<BaseFloat, int32>>: +0 == -0
    out, tot = [], F32(-np.inf)
    for j in range(min(num_gselect, len(pairs))):
        out.append(pairs[j][1])
        tot = log_add(tot, pairs[j][0])
    assert out
    return out, tot


def gaussian_selection_frame(gmm, x, num_gselect, mode="library"):
    """-> (list, like float32, status).  num_gselect above the number of Gaussians selects them all, as thresh = -inf does."""
    ll = log_likelihoods_preselect(gmm, x, None, mode)
    if np.isnan(ll).any():
        return [], F32(np.nan), 1
    out, tot = select(ll, np.arange(len(ll)), min(num_gselect, len(ll)))
    return out, tot, 0


def gaussian_selection_preselect(gmm, x, preselect, num_gselect, mode="library"):
    ll = log_likelihoods_preselect(gmm, x, preselect, mode)
    if np.isnan(ll).any():
        return [], F32(np.nan), 1
    out, tot = select(ll, preselect, min(num_gselect, len(preselect)))    # this_num_gselect
    return out, tot, 0


def parts(num_frames, num_gauss):
    """The max_mem split of GaussianSelection(Matrix) :807-830 (it recurses at most once): [(start, end), ...]."""
    mem_needed = num_frames * num_gauss * 4
    if mem_needed <= MAX_MEM:
        return [(0, num_frames)]
    num_parts = (mem_needed + MAX_MEM - 1) // MAX_MEM
    part_frames = (num_frames + num_parts - 1) // num_parts
    return [(p * part_frames, min(num_frames, (p + 1) * part_frames)) for p in range(num_parts) if p * part_frames < num_frames]


def sum_in_parts(frame_likes, num_gauss):
    """The double the matrix form returns: `ans += tot_loglike` within a part, `tot_ans += part` over the parts."""
    tot = 0.0
    pp = parts(len(frame_likes), num_gauss)
    for a, b in pp:
        ans = 0.0
        for t in range(a, b):
            ans += float(frame_likes[t])
        tot = ans if len(pp) == 1 else tot + ans
    return tot


def gaussian_selection(gmm, feats, num_gselect, preselect=None, mode="library"):
    """Every frame -> (lists, frame_like float32 [T], status int32 [T]); preselect: a list per frame, or None."""
    lists, likes, status = [], [], []
    for t in range(len(feats)):
        if preselect is None:
            o, l, s = gaussian_selection_frame(gmm, feats[t], num_gselect, mode)
        else:
            o, l, s = gaussian_selection_preselect(gmm, feats[t], preselect[t], num_gselect, mode)
        lists.append(o); likes.append(l); status.append(s)
    return lists, np.asarray(likes, F32), np.asarray(status, np.int32)


def soft_max(f, weight, mode):
    """ApplySoftMax (kaldi-vector.cc:840-847) then Scale(weight) -> (posteriors float32, like float32)."""
    return FR.soft_max(f, weight)       # in both modes: Exp / Log as the float of the float64 function


def global_acc_stats(gmm, feats, gselect=None, weights=None, flags=7, mode="library"):
    """gmm-global-acc-stats.cc:117-139 for one utterance.  -> dict(occ, mean_acc, var_acc (float64, None where the flags
    exclude), post [used frames x G] float32 dense, used (frame indices), frame_like float32 [T] (0 where skipped),
    file_like float32, file_weight float32)."""
    G, D = np.asarray(gmm["means_invvars"]).shape
    feats = np.asarray(feats, F32)
    occ = np.zeros(G, F64)
    mean = np.zeros((G, D), F64) if flags & 1 else None
    var = np.zeros((G, D), F64) if flags & 2 else None
    file_like, file_weight = F32(0.0), F32(0.0)
    rows, used, frame_like = [], [], np.zeros(len(feats), F32)
    for i in range(len(feats)):
        weight = F32(weights[i]) if weights is not None else F32(1.0)
        if weight == 0.0:
            continue
        file_weight = F32(file_weight + weight)
        ids = np.arange(G) if gselect is None else np.asarray(gselect[i], np.int64)
        assert len(ids) > 0
        ll = log_likelihoods_preselect(gmm, feats[i], None if gselect is None else ids, mode)
        post, like = soft_max(ll, weight, mode)
        file_like = F32(file_like + F32(weight * like))
        frame_like[i] = like
        data_d = feats[i].astype(F64)
        dense = np.zeros(G, F32)
        for j, g in enumerate(ids):                               # AccumulateForComponent; AccumulateFromPosteriors adds
            wt = float(post[j])                                   # the same addends Gaussian by Gaussian
            occ[g] += wt
            if mean is not None:
                mean[g] += wt * data_d
            if var is not None:
                var[g] += wt * (data_d * data_d)
            dense[g] = F32(dense[g] + post[j]) if gselect is not None and (ids[:j] == g).any() else post[j]
        rows.append(dense)
        used.append(i)
    return dict(occ=occ, mean_acc=mean, var_acc=var, post=np.asarray(rows, F32).reshape(len(rows), G), used=np.asarray(used, np.int32),
                frame_like=frame_like, file_like=file_like, file_weight=file_weight)
