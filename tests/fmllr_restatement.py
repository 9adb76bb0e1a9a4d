"""The fMLLR estimation of gmm-est-fmllr / gmm-est-fmllr-gpost restated line by line in numpy: float32 where the reference
is float, float64 where it is double, frames summed in order, a frame's entries in the order given (ascending pdf by the
rule of api.convert_posterior_to_pdfs), matrix inverses by np.linalg.inv (or, for the tolerance study, a Cholesky solve).

Stages and the reference lines they restate (the library's stages of the same names, include/kaldi_hip.h):
  A1 component_posteriors   DiagGmm::ComponentPosteriors gmm/diag-gmm.cc:601-615, VectorBase::ApplySoftMax
                            matrix/kaldi-vector.cc:840-847, posterior.Scale(weight) transform/fmllr-diag-gmm.cc:108-109
  A2 frame_stats            AccumulateFromPosteriors fmllr-diag-gmm.cc:30-43, DataHasChanged / Init / Commit :542-596
  B  accumulate             CommitSingleFrameStats :562-596
  C  update                 Update :131-166, ComputeFmllrMatrixDiagGmmFull / FmllrInnerUpdate :193-273, ...Diagonal :275-348,
                            ...Offset :350-378, FmllrAuxFuncDiagGmm :481-508
The per-Gaussian scores are the k-ordered fmaf chains of kh_gmm.hip and of the oracle's DiagGmm (the reference's own order is
its BLAS's).  expf / logf are restated as the correctly rounded float of the float64 function.

An entry list is CSR over the stacked frames: feo [T + 1] int64, pdf [E] int32, weight [E] float32, goff [E + 1] int64 (the
running sum of the entries' pdf sizes)."""
import math

import numpy as np

F32, F64 = np.float32, np.float64


def fmaf(a, b, c):
    """fl32(a * b + c) with ONE rounding, elementwise on float32 arrays.  The float64 product of two floats is exact; the
    float64 sum is rounded to odd (from the TwoSum error term) so that the second rounding, to float32, cannot double-round."""
    a, b, c = np.asarray(a, F32), np.asarray(b, F32), np.asarray(c, F32)
    s = a.astype(F64) * b.astype(F64)
    c64 = c.astype(F64)
    with np.errstate(invalid="ignore", over="ignore"):
        t = s + c64
        bb = t - s
        err = (s - (t - bb)) + (c64 - bb)
        t = np.asarray(t)
        fix = np.isfinite(t) & (err != 0) & ((t.view(np.int64) & 1) == 0)
        t = np.where(fix, np.nextafter(t, np.where(err > 0, np.inf, -np.inf)), t)
        return t.astype(F32)


def scores(x, gconsts, mi, iv):
    """Per-Gaussian log-likelihoods of one frame x [D] for Gaussians mi / iv [n, D]: a1 and a2 fmaf chains over d in order,
    ll = (g + a1) + (-0.5f * a2) (kh_gmm.hip GmmLoglikesKernel; DiagGmm::LogLikelihoods diag-gmm.cc:528-543)."""
    x = np.asarray(x, F32)
    xx = (x * x).astype(F32)
    a1 = np.zeros(len(gconsts), F32)
    a2 = np.zeros(len(gconsts), F32)
    for d in range(len(x)):
        a1 = fmaf(x[d], mi[:, d], a1)
        a2 = fmaf(xx[d], iv[:, d], a2)
    return ((gconsts + a1).astype(F32) + (F32(-0.5) * a2).astype(F32)).astype(F32)


def expf(x):
    return np.exp(np.asarray(x, F32).astype(F64)).astype(F32)


def logf(x):
    return np.log(np.asarray(x, F32).astype(F64)).astype(F32)


def soft_max(f, weight):
    """ApplySoftMax then Scale(weight) on float32 scores -> (posteriors float32, like float32)."""
    mx = f.max()
    e = expf((f - mx).astype(F32))
    s = np.cumsum(e, dtype=F32)[-1]                       # sum += ..., in order, float
    inv = F32(1.0 / float(s))                            # Scale(1.0 / sum): the double quotient as a float
    p = ((e * inv).astype(F32) * F32(weight)).astype(F32)
    return p, F32(mx + logf(s))


def model_arrays(am):
    """(gconsts, mi, iv, pdf_offsets) float32 / int arrays of a dict(gconsts, means_invvars, inv_vars, pdf_offsets)."""
    return (np.asarray(am["gconsts"], F32), np.asarray(am["means_invvars"], F32), np.asarray(am["inv_vars"], F32),
            np.asarray(am["pdf_offsets"], np.int64))


def entries_of(pdf_posts, pdf_offsets):
    """CSR entry list of a Posterior over pdfs (list over the stacked frames of [(pdf, weight), ...])."""
    off = np.asarray(pdf_offsets, np.int64)
    feo = np.zeros(len(pdf_posts) + 1, np.int64)
    pdf, w = [], []
    for t, fr in enumerate(pdf_posts):
        for p, x in fr:
            pdf.append(int(p))
            w.append(x)
        feo[t + 1] = len(pdf)
    pdf = np.asarray(pdf, np.int32)
    goff = np.zeros(len(pdf) + 1, np.int64)
    goff[1:] = np.cumsum(off[pdf + 1] - off[pdf]) if len(pdf) else 0
    return dict(feo=feo, pdf=pdf, weight=np.asarray(w, F32), goff=goff)


def component_posteriors(am, feats, ent):
    """A1 -> (gauss_post float32 [goff[E]], like float32 [E])."""
    g, mi, iv, off = model_arrays(am)
    E = len(ent["pdf"])
    post, like = np.zeros(int(ent["goff"][-1]), F32), np.zeros(E, F32)
    for t in range(len(ent["feo"]) - 1):
        for e in range(int(ent["feo"][t]), int(ent["feo"][t + 1])):
            m0, m1 = int(off[ent["pdf"][e]]), int(off[ent["pdf"][e] + 1])
            f = scores(feats[t], g[m0:m1], mi[m0:m1], iv[m0:m1])
            post[int(ent["goff"][e]):int(ent["goff"][e + 1])], like[e] = soft_max(f, ent["weight"][e])
    return post, like


def merged_frames(feats, utt_row_offsets, spk_utt_offsets, feo):
    """-> (run_row, run_entry_offsets, spk_run_offsets): DataHasChanged (:542-545) seen from the calls that reach it, one per
    entry.  Within a speaker the frames that have entries are walked in order, across utterances; a frame starts a merged
    frame when some element of its row != the held row's (the first frame of a speaker always: the reference compares it with
    zeros and skips the re-initialisation when equal, which leaves the same state)."""
    run_row, run_entry, spk_run = [], [], [0]
    for s in range(len(spk_utt_offsets) - 1):
        cur = None
        for t in range(int(utt_row_offsets[spk_utt_offsets[s]]), int(utt_row_offsets[spk_utt_offsets[s + 1]])):
            if feo[t + 1] == feo[t]:
                continue
            if cur is None or bool((feats[t] != feats[cur]).any()):
                run_row.append(t)
                run_entry.append(int(feo[t]))
                cur = t
        spk_run.append(len(run_row))
    run_entry.append(int(feo[-1]))
    return np.asarray(run_row, np.int32), np.asarray(run_entry, np.int64), np.asarray(spk_run, np.int32)


def frame_stats(am, feats, utt_row_offsets, spk_utt_offsets, ent, post):
    """A2 -> dict(run_row, spk_run_offsets, a [R, D] float32, b [R, D] float32, count [R] float64).  am: the model whose
    means_invvars / inv_vars are accumulated (its pdf sizes must match the entries')."""
    _, mi, iv, off = model_arrays(am)
    run_row, run_entry, spk_run = merged_frames(feats, utt_row_offsets, spk_utt_offsets, ent["feo"])
    R, D = len(run_row), mi.shape[1]
    a, b, count = np.zeros((R, D), F32), np.zeros((R, D), F32), np.zeros(R, F64)
    for r in range(R):
        for e in range(int(run_entry[r]), int(run_entry[r + 1])):
            m0 = int(off[ent["pdf"][e]])
            p = post[int(ent["goff"][e]):int(ent["goff"][e + 1])]
            if len(p) != int(off[ent["pdf"][e] + 1]) - m0:
                raise ValueError("pdf %d: %d posteriors, %d Gaussians" % (ent["pdf"][e], len(p), int(off[ent["pdf"][e] + 1]) - m0))
            count[r] += float(F32(np.cumsum(p.astype(F64))[-1]))       # stats.count += posterior.Sum(): double sum, float value
            for k in range(len(p)):                                     # AddMatVec(1.0, M, kTrans, posterior, 1.0)
                a[r] = fmaf(p[k], mi[m0 + k], a[r])
                b[r] = fmaf(p[k], iv[m0 + k], b[r])
    return dict(run_row=run_row, spk_run_offsets=spk_run, a=a, b=b, count=count)


def packed_index(D):
    """(r, c) of the packed lower triangle of a (D + 1) x (D + 1) SpMatrix, in storage order."""
    r, c = np.tril_indices(D + 1)
    return r, c


def accumulate(feats, fs, reverse=False):
    """B -> dict(beta [S], K [S, D, D + 1], G [S, D, P]) float64, merged frames added in order (reverse: last first)."""
    D = feats.shape[1]
    pr, pc = packed_index(D)
    S = len(fs["spk_run_offsets"]) - 1
    beta, K, G = np.zeros(S, F64), np.zeros((S, D, D + 1), F64), np.zeros((S, D, len(pr)), F64)
    for s in range(S):
        rs = range(int(fs["spk_run_offsets"][s]), int(fs["spk_run_offsets"][s + 1]))
        for r in (reversed(rs) if reverse else rs):
            if fs["count"][r] == 0.0:                                    # :566
                continue
            xp = np.concatenate([feats[fs["run_row"][r]].astype(F64), [1.0]])
            beta[s] += fs["count"][r]
            K[s] += np.outer(fs["a"][r].astype(F64), xp)                 # K_.AddVecVec(1.0, a, xplus)
            scatter = xp[pr] * xp[pc]                                    # scatter.AddVec2(1.0, xplus)
            G[s] += fs["b"][r].astype(F64)[:, None] * scatter[None, :]   # G_[i].AddSp(b(i), scatter)
    return dict(beta=beta, K=K, G=G)


def full_g(Gp, D):
    """[D, P] packed -> [D, D + 1, D + 1] symmetric."""
    pr, pc = packed_index(D)
    M = np.zeros((Gp.shape[0], D + 1, D + 1), F64)
    M[:, pr, pc] = Gp
    M[:, pc, pr] = Gp
    return M


def aux(W, beta, K, Gf):
    """FmllrAuxFuncDiagGmm :496-508 (double)."""
    W = np.asarray(W, F64)
    D = W.shape[0]
    obj = beta * np.linalg.slogdet(W[:, :D])[1] + float((W * K).sum())
    for d in range(D):
        obj -= 0.5 * float(W[d] @ (Gf[d] @ W[d]))
    return obj


def approx_equal(a, b, tol=0.001):
    if a == b:
        return True
    diff = abs(a - b)
    if math.isinf(diff) or diff != diff:
        return False
    return diff <= tol * (abs(a) + abs(b))


def _inverse(M, how):
    if how == "inv":
        return np.linalg.inv(M)
    L = np.linalg.cholesky(M)                                            # the second route of the tolerance study
    Li = np.linalg.solve(L, np.eye(len(M)))
    return Li.T @ Li


def update_one(beta, K, Gp, update_type="full", min_count=500.0, num_iters=40, inverse="inv"):
    """C for one speaker from a unit transform -> (W float32 [D, D + 1], objf_impr float32, count float32)."""
    D = K.shape[0]
    W = np.zeros((D, D + 1), F32)
    W[np.arange(D), np.arange(D)] = 1.0
    if not beta > float(F32(min_count)):                                 # :144, :161-164
        return W, F32(0.0), F32(beta)
    Gf = full_g(Gp, D)
    if update_type == "full":
        inv_g = [_inverse(Gf[d], inverse) for d in range(D)]
        new = W.astype(F64)
        old_objf = F32(aux(new, beta, K, Gf))
        for _ in range(num_iters):
            for d in range(D):                                           # FmllrInnerUpdate :193-234
                cof = np.linalg.inv(new[:, :D].T) if inverse == "inv" else np.linalg.solve(new[:, :D].T, np.eye(D))
                row = np.concatenate([cof[d], [0.0]])
                row_invg = inv_g[d] @ row
                e1, e2 = float(row_invg @ row), float(row_invg @ K[d])
                discr = math.sqrt(e2 * e2 + 4 * e1 * beta)
                al1, al2 = (-e2 + discr) / (2 * e1), (-e2 - discr) / (2 * e1)
                f1 = beta * math.log(abs(al1 * e1 + e2)) - 0.5 * al1 * al1 * e1
                f2 = beta * math.log(abs(al2 * e1 + e2)) - 0.5 * al2 * al2 * e1
                alpha = al1 if f1 > f2 else al2
                new[d] = inv_g[d] @ (alpha * row + K[d])
        new_objf = F32(aux(new, beta, K, Gf))
        impr = F32(new_objf - old_objf)
        if impr < 0.0 and not approx_equal(float(new_objf), float(old_objf)):
            return W, F32(0.0), F32(beta)
        return new.astype(F32), impr, F32(beta)
    if update_type == "diag":                                            # :275-348
        old = F32(aux(W, beta, K, Gf))
        for i in range(D):
            k_ii, k_id = K[i, i], K[i, D]
            g_iii, g_idd, g_idi = Gf[i, i, i], Gf[i, D, D], Gf[i, D, i]
            a, b, c = g_idi * g_idi / g_idd - g_iii, k_ii - g_idi * k_id / g_idd, beta
            s = (-b - math.sqrt(b * b - 4 * a * c)) / (2 * a)
            assert s > 0.0
            W[i, i], W[i, D] = s, (k_id - s * g_idi) / g_idd
        return W, F32(F32(aux(W, beta, K, Gf)) - old), F32(beta)
    if update_type == "offset":                                          # :350-378
        impr = F32(0.0)
        for i in range(D):
            g_dd, g_id, k_id = Gf[i, D, D], Gf[i, i, D], K[i, D]
            b_i = float(W[i, D])
            before = F32(-0.5 * b_i * b_i * g_dd - b_i * g_id + b_i * k_id)
            W[i, D] = (k_id - g_id) / g_dd
            b_i = float(W[i, D])
            after = F32(-0.5 * b_i * b_i * g_dd - b_i * g_id + b_i * k_id)
            impr = F32(impr + F32(after - before))
        return W, impr, F32(beta)
    assert update_type == "none"
    return W, F32(0.0), F32(beta)


def update(stats, **kw):
    out = [update_one(stats["beta"][s], stats["K"][s], stats["G"][s], **kw) for s in range(len(stats["beta"]))]
    return np.stack([o[0] for o in out]), np.asarray([o[1] for o in out], F32), np.asarray([o[2] for o in out], F32)


def estimate(am, feats, utt_row_offsets, spk_utt_offsets, ent, update_kw, post=None, acc_am=None, reverse=False, perturb=None):
    """The whole chain -> dict(post, like, fs, stats, W, impr, count).  post given: the gpost route (A1 skipped).  perturb:
    a function applied to the Gaussian posteriors before A2 (the tolerance study)."""
    like = None
    if post is None:
        post, like = component_posteriors(am, feats, ent)
    if perturb is not None:
        post = perturb(post)
    fs = frame_stats(acc_am or am, feats, utt_row_offsets, spk_utt_offsets, ent, post)
    stats = accumulate(feats, fs, reverse=reverse)
    W, impr, count = update(stats, **update_kw)
    return dict(post=post, like=like, fs=fs, stats=stats, W=W, impr=impr, count=count)


# ---------------------------------------------------------------- host posterior / transform algebra
def weight_silence_post(tid2phone, silence_phones, silence_scale, post, distribute=False):
    """WeightSilencePost / WeightSilencePostDistributed hmm/posterior.cc:361-413; float weights."""
    sil = set(int(p) for p in silence_phones)
    scale = F32(silence_scale)
    out = []
    for fr in post:
        if not distribute:
            this = []
            for tid, w in fr:
                if int(tid2phone[tid]) in sil:
                    if scale != 0.0:
                        this.append((tid, float(F32(F32(w) * scale))))
                else:
                    this.append((tid, float(F32(w))))
            out.append(this)
            continue
        sw, nw = F32(0.0), F32(0.0)
        for tid, w in fr:
            if int(tid2phone[tid]) in sil:
                sw = F32(sw + F32(w))
            else:
                nw = F32(nw + F32(w))
        assert sw >= 0.0 and nw >= 0.0
        if F32(sw + nw) == 0.0:
            out.append(list(fr))                                          # `continue`: the frame is left as it is
            continue
        fscale = F32(F32(F32(sw * scale) + nw) / F32(sw + nw))
        out.append([(tid, float(F32(F32(w) * fscale))) for tid, w in fr] if fscale != 0.0 else [])
    return out


def compose_transforms(a, b, b_is_affine):
    """ComposeTransforms transform/transform-common.cc:132-166 in float64 (the product is checked to 1e-4)."""
    a, b = np.asarray(a, F64), np.asarray(b, F64)
    if b.shape[0] == 0 or a.shape[1] == 0:
        return None
    if a.shape[1] == b.shape[0]:
        return a @ b
    if a.shape[1] == b.shape[0] + 1:
        if b_is_affine:
            be = np.zeros((b.shape[0] + 1, b.shape[1]))
            be[:-1] = b
            be[-1, -1] = 1.0
        else:
            be = np.zeros((b.shape[0] + 1, b.shape[1] + 1))
            be[:-1, :-1] = b
            be[-1, -1] = 1.0
        return a @ be
    raise ValueError("ComposeTransforms: mismatched dimensions")


def transform_feats(trans, feats):
    """featbin/transform-feats.cc:123-139: linear (cols == dim), affine (cols == dim + 1), else an error."""
    trans, feats = np.asarray(trans, F64), np.asarray(feats, F64)
    if trans.shape[1] == feats.shape[1]:
        return feats @ trans.T
    if trans.shape[1] == feats.shape[1] + 1:
        return feats @ trans[:, :-1].T + trans[:, -1]
    raise ValueError("Transform matrix has bad dimension %dx%d versus feat dim %d" % (trans.shape + (feats.shape[1],)))
