"""gmm-acc-mllt restated line by line in numpy: the binary's loop (gmmbin/gmm-acc-mllt.cc:78-117) over
MlltAccs::AccumulateFromGmm (transform/mllt.cc:162-170), AccumulateFromPosteriors (:131-160) and RandPrune
(base/kaldi-math.h:169-175) with RandUniform (:146-148) over Rand (base/kaldi-math.cc:45-63).  float32 where the reference is
float, float64 where it is double; the draws are the C library's rand() through ctypes, so a process that never calls srand
draws what the reference binary draws.  The Gaussian posteriors are fmllr_restatement's (DiagGmm::ComponentPosteriors); a
frame's entries are in ascending pdf order (the reference's order is its unordered_map's).

An accumulator is dict(beta float, G [D, Q] float64 - row j the packed lower triangle of G_[j], Q = D (D + 1) / 2 -, dim,
rand_prune float32; with a list under "trace" it records every posterior and what RandPrune made of it).  The SpMatrix
updates are numpy operations on the packed rows: tmp.AddVec2(1.0, offset_dbl) is the exact product of two widened floats, G_[j].AddSp(alpha, tmp) one rounding for alpha * tmp and one for the addition.

As a program it runs the binary's loop on a pickled job, in a process of its own whose generator nobody has seeded:
  python tests/mllt_restatement.py <job.pkl> <rand-prune> <out.pkl>"""
import ctypes
import pickle
import sys

import numpy as np

F32, F64 = np.float32, np.float64
_libc = ctypes.CDLL(None)
_libc.rand.restype = ctypes.c_int
_libc.srand.argtypes = [ctypes.c_uint]
RAND_MAX = 2147483647                                 # <stdlib.h> of the C library
DRAWS = [0]                                           # the number of rand() calls made through this module


def srand(seed):
    _libc.srand(seed)


def rand():
    DRAWS[0] += 1
    return int(_libc.rand())


def rand_uniform():
    """kaldi-math.h:146-148: static_cast<float>((Rand(state) + 1.0) / (RAND_MAX + 2.0))."""
    return F32((rand() + 1.0) / (RAND_MAX + 2.0))


def rand_prune(post, prune_thresh, log=None):
    """kaldi-math.h:169-175 with Float = BaseFloat = float.
        KALDI_ASSERT(prune_thresh >= 0.0);
        if (post == 0.0 || std::abs(post) >= prune_thresh) return post;
        return (post >= 0 ? 1.0 : -1.0) * (RandUniform(state) <= fabs(post)/prune_thresh ? prune_thresh : 0.0);
    fabs is the C library's ::fabs(double) (the header includes <cmath> only and the call is unqualified, inside namespace
    kaldi), so the quotient is a double division and the float draw is widened; the double product is returned as a float:
    a negative value pruned away is -0.0.  log: a list that takes (|post|, threshold, draw or None, quotient or None)."""
    post, prune_thresh = F32(post), F32(prune_thresh)
    assert prune_thresh >= 0.0
    if post == 0.0 or abs(post) >= prune_thresh:
        if log is not None and post != 0.0:
            log.append((float(abs(post)), float(prune_thresh), None, None))
        return post
    u = rand_uniform()
    q = abs(F64(post)) / F64(prune_thresh)
    if log is not None:
        log.append((float(abs(post)), float(prune_thresh), float(u), float(q)))
    return F32((1.0 if post >= 0 else -1.0) * (F64(prune_thresh) if F64(u) <= q else 0.0))


def packed_pairs(dim):
    """(a, b) of the packed index q = a (a + 1) / 2 + b, a >= b (SpMatrix)."""
    a, b = np.tril_indices(dim)
    return a, b


def init_accs(dim, prune):
    """MlltAccs::Init (mllt.cc:25-32)."""
    assert dim > 0
    return dict(beta=0.0, G=np.zeros((dim, dim * (dim + 1) // 2), F64), dim=int(dim), rand_prune=F32(prune))


def accumulate_from_posteriors(acc, means_invvars, inv_vars, data, posteriors, log=None):
    """mllt.cc:131-160 for one pdf's means_invvars / inv_vars [n, D], one feature row and the pdf's n posteriors."""
    D = acc["dim"]
    assert len(data) == D == means_invvars.shape[1] and len(posteriors) == means_invvars.shape[0]
    a, b = packed_pairs(D)
    data = np.asarray(data, F32)
    this_beta = F64(0.0)
    assert acc["rand_prune"] >= 0.0
    for i in range(len(posteriors)):                                     # for each mixcomp..
        posterior = rand_prune(posteriors[i], acc["rand_prune"], log)
        if "trace" in acc:                                               # (the posterior, what RandPrune made of it), slot by slot
            acc["trace"].append((F32(posteriors[i]), posterior))
        if posterior == 0.0:
            continue
        mean_invvar, inv_var = np.asarray(means_invvars[i], F32), np.asarray(inv_vars[i], F32)
        mean = (mean_invvar / inv_var).astype(F32)                       # mean.AddVecDivVec(1.0, mean_invvar, inv_var, 0.0)
        mean = (mean - data).astype(F32)                                 # mean.AddVec(-1.0, data)
        offset_dbl = mean.astype(F64)                                    # offset_dbl.CopyFromVec(mean)
        tmp = offset_dbl[a] * offset_dbl[b]                              # tmp.SetZero(); tmp.AddVec2(1.0, offset_dbl)
        alpha = (inv_var * posterior).astype(F32).astype(F64)            # inv_var(j)*posterior, BaseFloat, passed as double
        acc["G"] += alpha[:, None] * tmp[None, :]                        # G_[j].AddSp(inv_var(j)*posterior, tmp), every j
        this_beta = this_beta + F64(posterior)                           # this_beta_ += posterior
    acc["beta"] = float(F64(acc["beta"]) + this_beta)                    # beta_ += this_beta_


def accumulate_entries(acc, am, feats, ent, gauss_post, log=None):
    """AccumulateFromPosteriors for every entry of a CSR entry list in frame order, with the given (unpruned) Gaussian
    posteriors, already times the entry's weight."""
    off = np.asarray(am["pdf_offsets"], np.int64)
    mi, iv = np.asarray(am["means_invvars"], F32), np.asarray(am["inv_vars"], F32)
    for t in range(len(ent["feo"]) - 1):
        for e in range(int(ent["feo"][t]), int(ent["feo"][t + 1])):
            m0, m1 = int(off[ent["pdf"][e]]), int(off[ent["pdf"][e] + 1])
            accumulate_from_posteriors(acc, mi[m0:m1], iv[m0:m1], feats[t], gauss_post[int(ent["goff"][e]):int(ent["goff"][e + 1])], log)
    return acc


def accumulate_from_gmm(acc, am, pdf, data, weight, log=None):
    """mllt.cc:162-170: ComponentPosteriors, posteriors.Scale(weight), AccumulateFromPosteriors -> the log-likelihood."""
    import fmllr_restatement as R
    g, mi, iv, off = R.model_arrays(am)
    m0, m1 = int(off[pdf]), int(off[pdf + 1])
    posteriors, ans = R.soft_max(R.scores(data, g[m0:m1], mi[m0:m1], iv[m0:m1]), weight)
    accumulate_from_posteriors(acc, mi[m0:m1], iv[m0:m1], data, posteriors, log)
    return ans


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


def acc_mllt(am, tid2pdf, utts, prune, log=None, trace=False):
    """gmm-acc-mllt.cc:70-117.  utts: [(features [T, D], posterior over transition-ids)] of the utterances that are done.
    -> (acc, tot_like, tot_t, [(tot_like_this_file, tot_weight) per utterance])."""
    acc = init_accs(np.asarray(am["means_invvars"]).shape[1], prune)     # MlltAccs mllt_accs(am_gmm.Dim(), rand_prune)
    if trace:
        acc["trace"] = []
    tot_like, tot_t = 0.0, 0.0
    files = []
    for mat, posterior in utts:
        tot_like_this_file, tot_weight = F32(0.0), F32(0.0)
        pdf_posterior = convert_posterior_to_pdfs(tid2pdf, posterior)
        for i in range(len(posterior)):
            for pdf_id, weight in pdf_posterior[i]:
                weight = F32(weight)
                tot_like_this_file = F32(tot_like_this_file + F32(accumulate_from_gmm(acc, am, pdf_id, mat[i], weight, log) * weight))
                tot_weight = F32(tot_weight + weight)
        tot_like += float(tot_like_this_file)
        tot_t += float(tot_weight)
        files.append((float(tot_like_this_file), float(tot_weight)))
    return acc, tot_like, tot_t, files


def main(argv):
    with open(argv[0], "rb") as f:
        job = pickle.load(f)
    log = []
    acc, tot_like, tot_t, files = acc_mllt(job["am"], job["tid2pdf"], job["utts"], float(argv[1]), log, trace=True)
    acc["trace"] = np.asarray(acc["trace"], F32).reshape(-1, 2)
    with open(argv[2], "wb") as f:
        pickle.dump(dict(acc=acc, tot_like=tot_like, tot_t=tot_t, files=files, log=log, draws=DRAWS[0]), f)
    return 0


if __name__ == "__main__":
    import os
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    sys.exit(main(sys.argv[1:]))
