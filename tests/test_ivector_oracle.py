"""CPU: pins the numpy specification of OnlineIvectorFeature (oracle/ivector_oracle.py) piece by
piece to the REFERENCE compiled into oracle/_ref (live where it is built, elsewhere its recorded answers to the
same inputs: tests/refrecord.py; the committed fixture tests/golden/ivector.npz holds reference outputs too):
  * online CMVN -> splice -> LDA through the reference's OnlineCmvn / OnlineSpliceFrames /
    OnlineTransform (feat/online-feature.cc), window shorter and longer than the utterance;
  * UBM log-likelihoods through DiagGmm::LogLikelihoods;
  * LinearCgd (matrix/optimization.cc) on the quadratic forms the extractor produces.
VectorToPosteriorEntry and AccStats are restated (hmm/posterior.cc, ivector-extractor.cc need
OpenFst headers): checked against their definitions (a posterior entry sums to one, keeps the
num_gselect largest, prunes below min_post; the estimated iVector solves quadratic x = linear)."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

from oracle import binding as B
from oracle import ivector_oracle as IO

workloads = importlib.import_module("old-kaldi-git_amd.workloads")
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ivector.npz")


def small_model(rng, **kw):
    args = dict(base_dim=10, splice=2, feat_dim=8, num_gauss=16, ivector_dim=12, prior_offset=4.0)
    args.update(kw)
    return workloads.make_ivector_extractor(rng, **args)


def _live_chain(m, X):
    lib = C.CDLL(B.REF_SO)
    T, D = X.shape
    lda = np.ascontiguousarray(m["lda_mat"], np.float32)
    gs = np.ascontiguousarray(m["global_cmvn_stats"], np.float64)
    o1, o2, o3 = (np.empty((T, lda.shape[0]), np.float32), np.empty((T, lda.shape[0]), np.float32), np.empty((T, D), np.float32))
    fp, dp = C.POINTER(C.c_float), C.POINTER(C.c_double)
    rc = lib.ref_online_cmvn_splice_lda(np.ascontiguousarray(X).ctypes.data_as(fp), T, D, gs.ctypes.data_as(dp), m["cmn_window"],
                                        m["speaker_frames"], m["global_frames"], int(m["normalize_mean"]),
                                        int(m["normalize_variance"]), m["splice_left"], m["splice_right"],
                                        lda.ctypes.data_as(fp), lda.shape[0], lda.shape[1], o1.ctypes.data_as(fp),
                                        o2.ctypes.data_as(fp), o3.ctypes.data_as(fp))
    assert rc == 0
    return o1, o2, o3


def _live_cgd(A, b, x0, iters):
    lib = C.CDLL(B.REF_SO)
    S = len(b)
    r, c = np.tril_indices(S)
    packed = np.ascontiguousarray(A[r, c], np.float64)
    x = np.ascontiguousarray(x0, np.float64).copy()
    dp = C.POINTER(C.c_double)
    k = lib.ref_linear_cgd(S, packed.ctypes.data_as(dp), np.ascontiguousarray(b, np.float64).ctypes.data_as(dp), x.ctypes.data_as(dp), iters)
    return x, k


def _live_cmvn_speaker(m, X, speaker_stats):
    lib = C.CDLL(B.REF_SO)
    T, D = X.shape
    gs = np.ascontiguousarray(m["global_cmvn_stats"], np.float64)
    out, st = np.empty((T, D), np.float32), np.empty((2, D + 1), np.float64)
    fp, dp = C.POINTER(C.c_float), C.POINTER(C.c_double)
    sp = None if speaker_stats is None else np.ascontiguousarray(speaker_stats, np.float64).ctypes.data_as(dp)
    rc = lib.ref_online_cmvn_speaker(np.ascontiguousarray(X).ctypes.data_as(fp), T, D, gs.ctypes.data_as(dp), sp, m["cmn_window"],
                                     m["speaker_frames"], m["global_frames"], int(m["normalize_mean"]), int(m["normalize_variance"]),
                                     out.ctypes.data_as(fp), st.ctypes.data_as(dp))
    assert rc == 0
    return out, st


def ref_chain(ref, m, X):
    return ref.call("online_cmvn_splice_lda", _live_chain, m, X)


def ref_cgd(ref, A, b, x0, iters):
    return ref.call("linear_cgd", _live_cgd, A, b, x0, iters)


def ref_cmvn_speaker(ref, m, X, speaker_stats):
    return ref.call("online_cmvn_speaker", _live_cmvn_speaker, m, X, speaker_stats)


def cases():
    rng = np.random.default_rng(12)
    m = small_model(rng)
    m2 = dict(m, cmn_window=30, speaker_frames=30, global_frames=10, normalize_variance=True)
    X = (rng.standard_normal((75, 10)) * 1.3 + 0.4).astype(np.float32)
    return m, m2, X


def test_feature_chain_and_solver_match_the_reference(ref_lib):
    m, m2, X = cases()
    for mm in (m, m2):
        lda, lda_n, cm = ref_chain(ref_lib, mm, X)
        np.testing.assert_allclose(IO.online_cmvn(X, mm), cm, rtol=0, atol=2e-6)
        np.testing.assert_allclose(IO.splice_lda(X, mm), lda, rtol=0, atol=2e-6)
        np.testing.assert_allclose(IO.splice_lda(IO.online_cmvn(X, mm), mm), lda_n, rtol=0, atol=5e-6)
    rng = np.random.default_rng(3)
    for S in (5, 12, 40):
        Q = rng.standard_normal((S, S))
        A = Q @ Q.T + np.eye(S)
        b = rng.standard_normal(S)
        x0 = np.zeros(S)
        x0[0] = 2.0
        for iters in (3, 15):
            want, k = ref_cgd(ref_lib, A, b, x0, iters)
            got, k2 = IO.linear_cgd(A, b, x0.copy(), iters)
            assert k == k2
            np.testing.assert_allclose(got, want, rtol=1e-10, atol=1e-12)
    # UBM log-likelihoods: the reference's DiagGmm on the normalised features
    g, mi, iv = IO.ubm_params(m)
    Fn = IO.splice_lda(IO.online_cmvn(X, m), m)
    want = ref_lib.ref_diag_gmm_loglikes(m["ubm_weights"], m["ubm_means"], m["ubm_vars"], Fn)
    got = g[None, :] + Fn @ mi.T - 0.5 * ((Fn * Fn) @ iv.T)
    np.testing.assert_allclose(got, want, rtol=0, atol=2e-4)


def test_posterior_entry_and_ivector_definitions():
    rng = np.random.default_rng(5)
    ll = (rng.standard_normal(16) * 3).astype(np.float32)
    ent, tot = IO.vector_to_posterior_entry(ll, 5, 0.025)
    p = np.exp(ll - ll.max())
    p /= p.sum()
    top = np.argsort(-p)[:5]
    assert [g for g, _ in ent] == [int(g) for g in top if p[g] >= 0.025 or g == top[0]][:len(ent)]
    assert abs(sum(float(v) for _, v in ent) - 1.0) < 1e-6
    assert abs(tot - np.log(np.exp(ll.astype(np.float64)).sum())) < 1e-5
    # the iVector of the last estimation point solves the accumulated quadratic form (15 CG steps
    # from the previous estimate: to ~1e-6 on these sizes)
    m = small_model(rng)
    X = (rng.standard_normal((41, 10)) * 1.2).astype(np.float32)
    out = IO.extract(X, m)
    assert out.shape == (41, 12) and np.isfinite(out).all()
    assert np.array_equal(out[10], out[19]) and not np.array_equal(out[9], out[10])   # one estimate per period
    # recompute the stats of frames 0..40 directly
    F, Fn = IO.splice_lda(X, m), IO.splice_lda(IO.online_cmvn(X, m), m)
    g, mi, iv = IO.ubm_params(m)
    U, SiM = IO.derived(m)
    S = 12
    r, c = np.tril_indices(S)
    quad, lin = np.eye(S), np.zeros(S)
    lin[0] = m["prior_offset"]
    for t in range(41):
        ll = (g + mi @ Fn[t] - 0.5 * (iv @ (Fn[t] ** 2))).astype(np.float32)
        for gi, w in IO.vector_to_posterior_entry(ll, 5, 0.025)[0]:
            w = float(np.float32(w * np.float32(0.1)))
            lin += w * (SiM[gi].T @ F[t].astype(np.float64))
            Ug = np.zeros((S, S))
            Ug[r, c] = U[gi]
            Ug[c, r] = U[gi]
            quad += w * Ug
    exact = np.linalg.solve(quad, lin)
    exact[0] -= m["prior_offset"]
    np.testing.assert_allclose(out[40], exact, atol=2e-3)


def test_golden_fixture_matches_the_specification():
    """tests/golden/ivector.npz = reference outputs (make_golden.py --ivector): the spec must
    reproduce them on any machine (the GPU box has no /root/reference)."""
    z = np.load(GOLD)
    m, m2, X = cases()
    np.testing.assert_allclose(IO.online_cmvn(X, m), z["cmvn_a"], atol=2e-6)
    np.testing.assert_allclose(IO.splice_lda(IO.online_cmvn(X, m2), m2), z["lda_norm_b"], atol=5e-6)
    np.testing.assert_allclose(IO.splice_lda(X, m), z["lda_a"], atol=2e-6)
    got, _ = IO.linear_cgd(z["cg_A"], z["cg_b"], z["cg_x0"].copy(), 15)
    np.testing.assert_allclose(got, z["cg_x"], rtol=1e-10, atol=1e-12)


def test_cmvn_with_speaker_state_matches_the_reference(ref_lib):
    """The adaptation state's CMVN half: OnlineCmvn started from the speaker stats of the previous
    utterances (SetState) and the stats GetState returns, chained over three utterances of a speaker."""
    m, m2, X = cases()
    for mm in (m, dict(m2, speaker_frames=20)):
        sp_ref = sp_ora = None
        for seg in (X[:40], X[40:52], X[52:]):
            want, st_ref = ref_cmvn_speaker(ref_lib, mm, seg, sp_ref)
            got, st_ora = IO.online_cmvn(seg, mm, sp_ora, True)
            np.testing.assert_allclose(got, want, rtol=0, atol=2e-6)
            np.testing.assert_allclose(st_ora, st_ref, rtol=1e-12, atol=1e-9)
            sp_ref, sp_ora = st_ref, st_ora


def test_adaptation_state_algebra():
    """Scale (ivector-extractor.cc:570-592) keeps the prior's share of the statistics; LimitFrames
    (online-ivector-feature.cc:99-117) caps the remembered counts; a fresh state is what extract() starts from."""
    rng = np.random.default_rng(8)
    for max_count in (0.0, 2.0):
        m = dict(small_model(rng), max_count=max_count, posterior_scale=0.5)
        X = (rng.standard_normal((60, 10)) + 0.2).astype(np.float32)
        a = IO.extract(X, m)
        b, st = IO.extract(X, m, IO.fresh_state(m), True)
        assert np.array_equal(a, b)
        n0 = st["num_frames"]
        S = len(st["lin"])
        data_quad = st["quad"] - np.eye(S) * (max(n0, max_count) / max_count if max_count > 0 else 1.0)
        IO.limit_frames(st, m, 10.0)
        assert abs(st["num_frames"] - 5.0) < 1e-6 and abs(st["cmvn"][0, 10] - 10.0) < 1e-5      # 10 frames x posterior_scale (the CMVN ratio is a BaseFloat)
        prior = max(st["num_frames"], max_count) / max_count if max_count > 0 else 1.0
        np.testing.assert_allclose(st["quad"], data_quad * (5.0 / n0) + np.eye(S) * prior, rtol=1e-9, atol=1e-9)
        # the next utterance of the speaker starts from it: its first rows already lean on the speaker
        c, st2 = IO.extract(X[:15], m, st, True)
        assert np.abs(c[0] - a[0]).max() > 1e-3 and st2["num_frames"] > st["num_frames"]


def test_online_ivector_feature_object_and_silence_weighting_host_logic():
    """(a) The oracle's OnlineIvectorFeature object (GetFrame frame by frame; weights supplied as deltas of 1) reproduces extract().
    (b) The product's host logic online2.OnlineSilenceWeighting (arrays) against the oracle's line-by-line restatement of
    online-ivector-feature.cc:381-580 on random tracebacks that get rewritten, with and without --max-state-duration."""
    import importlib
    from oracle import ivector_oracle as IO
    W = importlib.import_module("old-kaldi-git_amd.workloads")
    o2 = importlib.import_module("old-kaldi-git_amd.online2")
    rng = np.random.default_rng(1)
    ie = W.make_ivector_extractor(rng, base_dim=4, splice=1, feat_dim=5, num_gauss=6, ivector_dim=2, prior_offset=3.0)
    ie.update(greedy_most_recent=False, ivector_period=10, max_count=0.0)
    X = rng.standard_normal((57, 4)).astype(np.float32)
    ref = IO.extract(X, ie)
    f = IO.OnlineIvectorFeature(X, ie)
    assert np.array_equal(np.stack([f.get_frame(t) for t in range(57)]), ref)
    f2 = IO.OnlineIvectorFeature(X, ie)
    f2.update_frame_weights([(t, 1.0) for t in range(57)], 57)
    assert np.array_equal(np.stack([f2.get_frame(t) for t in range(57)]), ref)
    f3 = IO.OnlineIvectorFeature(X, ie)                    # half weight on the first 20 frames changes the estimates
    f3.update_frame_weights([(t, 0.5 if t < 20 else 1.0) for t in range(57)], 57)
    assert np.abs(np.stack([f3.get_frame(t) for t in range(57)]) - ref).max() > 1e-3
    t2p = np.concatenate([[0], rng.integers(1, 6, 30)]).astype(np.int32)
    n_deltas = 0
    for msd in (-1, 3, 5):
        for sw in (0.0, 0.25):
            a, b = IO.OnlineSilenceWeighting(t2p, [1, 2], sw, msd), o2.OnlineSilenceWeighting(t2p, "1:2", sw, msd)
            assert b.active()
            ali, ready = np.zeros(0, np.int32), 0
            for step in range(40):
                ready += int(rng.integers(0, 7))
                n = max(len(ali), min(ready, len(ali) + int(rng.integers(0, 6))))
                new = ali.copy()
                if len(new) and rng.random() < 0.4:
                    k = int(rng.integers(0, len(new)))
                    new[k:] = rng.integers(1, 31, len(new) - k)
                ext = np.repeat(rng.integers(1, 31, n), rng.integers(1, 5, n))[:n - len(new)] if n > len(new) else np.zeros(0, np.int64)
                ali = np.concatenate([new, ext]).astype(np.int32)
                a.compute_current_traceback(ali)
                b.compute_current_traceback(ali)
                da, db = a.get_delta_weights(ready), b.get_delta_weights(ready)
                assert da == db, (msd, sw, step)
                n_deltas += len(da)
    assert n_deltas > 500
    assert not o2.OnlineSilenceWeighting(t2p, "", 0.0).active() and not o2.OnlineSilenceWeighting(t2p, "1:2", 1.0).active()


def test_exact_solve_fallback_of_linear_cgd_matches_the_reference(ref_lib):
    """LinearCgd falls back to SolveQuadraticProblem when the squared residual got worse (matrix/optimization.cc:546-563,
    sp-matrix.cc:659-734: eigenvalues floored at l_max / 1e4, the step taken only if the auxiliary function does not decrease).
    Ill-conditioned systems cut off after one or two iterations trigger it; the restatement against the compiled reference."""
    rng = np.random.default_rng(7)
    before = IO.STATS["exact_solves"]
    n = 0
    for S in (6, 20, 40):
        for cond in (1e3, 1e6, 1e9):
            for iters in (1, 2):
                for trial in range(6):
                    Q, _r = np.linalg.qr(rng.standard_normal((S, S)))
                    ev = np.sort(np.exp(rng.uniform(0, np.log(cond), S)))
                    ev[0], ev[-1] = 1.0, cond
                    A = (Q * ev) @ Q.T
                    A = (A + A.T) / 2
                    x0 = rng.standard_normal(S)
                    if trial % 2 == 0:
                        # a start whose residual lies along the smallest eigenvector with a little of the largest: the first
                        # (steepest-descent) step is sized for the small eigenvalue and blows the large component up
                        r0 = Q[:, 0] + cond ** -0.75 * Q[:, -1] + 1e-9 * rng.standard_normal(S)
                        b = A @ x0 + r0
                    else:
                        b = rng.standard_normal(S) * cond ** 0.5
                    got, k = IO.linear_cgd(A, b, x0.copy(), iters)
                    want, k2 = ref_cgd(ref_lib, A, b, x0, iters)
                    assert k == k2
                    # (eigenvectors of the small eigenvalues are only determined to ~1e-16 * cond by either eigen-solver)
                    tol = max(1e-9, 1e-13 * cond)
                    np.testing.assert_allclose(got, want, rtol=tol, atol=tol * np.abs(want).max())
                    n += 1
    assert IO.STATS["exact_solves"] - before >= 10, (IO.STATS["exact_solves"] - before, n)      # the fallback did run
