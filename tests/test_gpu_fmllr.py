"""GPU: the four stages of csrc/kh_fmllr.hip and api.estimate_fmllr against tests/fmllr_restatement.py, with the bounds that
tests/fmllr_cases.py derives.  Every test here fails on a library without the kh_fmllr_* entry points."""
import math

import numpy as np
import pytest
import torch

import fmllr_cases as C
import fmllr_restatement as R

pytestmark = pytest.mark.gpu


class Am:
    """api.AmDiagGmm of a fmllr_cases model dict."""

    def __new__(cls, api, am):
        return api.AmDiagGmm(am["gconsts"], am["means_invvars"], am["inv_vars"], am["pdf_offsets"])


def dev(x):
    return torch.as_tensor(np.ascontiguousarray(x), device="cuda")


# ---------------------------------------------------------------- A1
def test_component_posteriors(api, oracle):
    am, feats, posts = C.a1_case(oracle)
    ent = R.entries_of(posts, am["pdf_offsets"])
    assert sorted(set(np.diff(ent["goff"]).tolist())) == C.A1_SIZES
    assert {1, 3, 0} <= set(np.diff(ent["feo"]).tolist()) and (ent["weight"] == 0).any()
    want_post, want_like = R.component_posteriors(am, feats, ent)
    post, like = api.gmm_component_posteriors(Am(api, am), dev(feats), ent)
    post, like = post.cpu().numpy(), like.cpu().numpy()
    pr = np.abs(post.astype(np.float64) - want_post) / C.post_bound(want_post, ent["goff"])
    lr = np.abs(like.astype(np.float64) - want_like) / C.like_bound(want_like, ent["goff"])
    print("posteriors: worst error / bound", pr.max(), "scores:", lr.max())
    assert pr.max() <= 1.0 and lr.max() <= 1.0
    z = int(np.nonzero(ent["weight"] == 0)[0][0])
    assert (post[ent["goff"][z]:ent["goff"][z + 1]] == 0).all()
    # a strided feature matrix gives the same bits
    wide = torch.zeros((feats.shape[0], feats.shape[1] + 3), device="cuda")
    wide[:, :feats.shape[1]] = dev(feats)
    post2, like2 = api.gmm_component_posteriors(Am(api, am), wide[:, :feats.shape[1]], ent)
    assert np.array_equal(post2.cpu().numpy().view(np.int32), post.view(np.int32)) and np.array_equal(like2.cpu().numpy(), like)


def test_component_posteriors_rejects_bad_entries(api, oracle):
    am, feats, posts = C.a1_case(oracle)
    ent = R.entries_of(posts, am["pdf_offsets"])
    bad = dict(ent, pdf=ent["pdf"].copy())
    bad["pdf"][0] = 1          # 2 Gaussians where the offsets say 1
    with pytest.raises(api.KhError, match="pdf 1 has 2 Gaussians"):
        api.gmm_component_posteriors(Am(api, am), dev(feats), bad)
    bad["pdf"][0] = 6
    with pytest.raises(api.KhError, match="names pdf 6"):
        api.gmm_component_posteriors(Am(api, am), dev(feats), bad)


# ---------------------------------------------------------------- A2
def _frame_stats_equal(got, want):
    assert got["run_row"].tolist() == want["run_row"].tolist()
    assert got["spk_run_offsets"].tolist() == want["spk_run_offsets"].tolist()
    for k in ("a", "b"):
        assert np.array_equal(got[k].cpu().numpy().view(np.int32), want[k].view(np.int32)), k
    assert np.array_equal(got["count"].cpu().numpy().view(np.int64), want["count"].view(np.int64))


def test_frame_stats_bit_for_bit(api, oracle):
    am, feats, utt, spk, gposts = C.a2_case(oracle)
    ent, flat = C.gpost_entries(gposts)
    want = R.frame_stats(am, feats, utt, spk, ent, flat)
    assert (want["count"] == 0).sum() == 1 and len(want["run_row"]) == 16 and (np.diff(spk) == [2, 4, 1]).all()
    got = api.fmllr_frame_stats(Am(api, am), dev(feats), utt, spk, ent, dev(flat))
    _frame_stats_equal(got, want)


def test_frame_stats_two_models_and_mismatch(api, oracle):
    am, feats, utt, spk, gposts = C.a2_case(oracle)
    ent, flat = C.gpost_entries(gposts)
    am2 = C.other_model(am, 5)
    want = R.frame_stats(am2, feats, utt, spk, ent, flat)
    got = api.fmllr_frame_stats(Am(api, am2), dev(feats), utt, spk, ent, dev(flat))
    _frame_stats_equal(got, want)
    am3 = C.model([3, 1, 5, 2], 13, 22, oracle)     # pdf 2: 5 Gaussians, the gposts carry 4
    with pytest.raises(api.KhError, match="pdf 2 has 5 Gaussians"):
        api.fmllr_frame_stats(Am(api, am3), dev(feats), utt, spk, ent, dev(flat))


# ---------------------------------------------------------------- B
def _check_b(api, feats, fs):
    dfs = dict(run_row=fs["run_row"], spk_run_offsets=fs["spk_run_offsets"], a=dev(fs["a"]), b=dev(fs["b"]), count=dev(fs["count"]))
    x = dev(feats)
    got = api.fmllr_accumulate(x, dfs)
    again = api.fmllr_accumulate(x, dfs)
    for k in ("beta", "K", "G"):
        assert np.array_equal(got[k].view(np.int64), again[k].view(np.int64)), k       # two calls, equal bits
    beta, K, G, Ka, Ga, n = C.b_reference(feats, fs)
    unit = (n + 2.0) * 2.0 ** -53
    assert np.array_equal(got["beta"], beta) or np.abs(got["beta"] - beta).max() <= (unit * np.abs(beta)).max()
    ek, eg = np.abs(got["K"] - K), np.abs(got["G"] - G)
    bk, bg = unit[:, None, None] * Ka, unit[:, None, None] * Ga
    print("D", feats.shape[1], "worst error / bound: K", (ek / np.maximum(bk, 1e-300)).max(), "G", (eg / np.maximum(bg, 1e-300)).max())
    assert (ek <= bk).all() and (eg <= bg).all()
    empty = np.nonzero(np.diff(fs["spk_run_offsets"]) == 0)[0]
    for s in empty:
        assert got["beta"][s] == 0 and not got["K"][s].any() and not got["G"][s].any()
    return got, (beta, K, G, Ka, Ga, n)


@pytest.mark.parametrize("dim", C.B_DIMS)
def test_accumulate(api, dim):
    """Speakers of 1, 3, 4, 5, chunk - 1, chunk, chunk + 1 and 2 chunks + 1 merged frames, one without any, one of 31."""
    feats, fs = C.b_case(dim, 100 + dim)
    got, (beta, K, G, Ka, Ga, n) = _check_b(api, feats, fs)
    # The issue's bound against EXACTLY ROUNDED sums (rational arithmetic on the exact addends, rounded once - what math.fsum
    # gives for addends that are doubles): every element of K and G for D <= 5, a sample of 40 G and 40 K elements above.
    from fractions import Fraction
    rng = np.random.default_rng(dim)
    pr, pc = R.packed_index(dim)
    P = len(pr)
    if dim <= 5:
        picks = [(s, i, j) for s in range(len(n)) for i in range(dim) for j in range(P + dim + 1)]
    else:
        picks = [(int(rng.integers(0, len(n))), int(rng.integers(0, dim)), int(rng.integers(0, P))) for _ in range(40)]
        picks += [(int(rng.integers(0, len(n))), int(rng.integers(0, dim)), P + int(rng.integers(0, dim + 1))) for _ in range(40)]
    xps = np.concatenate([feats.astype(np.float64), np.ones((len(feats), 1))], axis=1)
    for s, i, j in picks:              # j < P: G[s, i, j]; else K[s, i, j - P]
        r0, r1 = int(fs["spk_run_offsets"][s]), int(fs["spk_run_offsets"][s + 1])
        live = [r for r in range(r0, r1) if fs["count"][r] != 0.0]
        if j < P:
            terms = [Fraction(float(fs["b"][r, i])) * Fraction(float(xps[fs["run_row"][r], pr[j]])) * Fraction(float(xps[fs["run_row"][r], pc[j]]))
                     for r in live]
            ref, dev, mag = G[s, i, j], got["G"][s, i, j], Ga[s, i, j]
        else:
            terms = [Fraction(float(fs["a"][r, i])) * Fraction(float(xps[fs["run_row"][r], j - P])) for r in live]
            ref, dev, mag = K[s, i, j - P], got["K"][s, i, j - P], Ka[s, i, j - P]
        exact = float(sum(terms, Fraction(0)))
        assert abs(ref - exact) <= 1.001 * 2.0 ** -53 * abs(exact) + (n[s] + 2.0) * 2.0 ** -64 * mag
        assert abs(dev - exact) <= (n[s] + 2.0) * 2.0 ** -53 * mag, (s, i, j)


def test_accumulate_seventy_speakers(api):
    feats, fs = C.b_case(5, 7, frames=[3] * 69)
    assert len(fs["spk_run_offsets"]) - 1 >= 70
    _check_b(api, feats, fs)


def test_accumulate_in_groups_gives_the_same_bits(api):
    """A workspace limit that holds three partial sums: the 71 speakers go in many groups (a speaker of three chunks alone
    exceeds it and is taken alone), and every sum keeps its bits."""
    feats, fs = C.b_case(16, 9, frames=[3] * 30 + [2 * C.FRAME_CHUNK + 1] + [5] * 38)
    dfs = dict(run_row=fs["run_row"], spk_run_offsets=fs["spk_run_offsets"], a=dev(fs["a"]), b=dev(fs["b"]), count=dev(fs["count"]))
    x = dev(feats)
    whole = api.fmllr_accumulate(x, dfs)
    assert api.fmllr_last_timings()["accumulate_groups"] == 1
    S = 16 * (17 * 18 // 2) + 16 * 17
    api.fmllr_set_workspace_limit(3 * S * 8)
    try:
        parts = api.fmllr_accumulate(x, dfs)
        assert api.fmllr_last_timings()["accumulate_groups"] >= 35
    finally:
        api.fmllr_set_workspace_limit(0)
    for k in ("beta", "K", "G"):
        assert np.array_equal(whole[k].view(np.int64), parts[k].view(np.int64)), k


def test_accumulate_dimension_limit(api):
    assert api.fmllr_max_dim() == C.MAX_DIM and api.fmllr_frame_chunk() == C.FRAME_CHUNK
    feats, fs = C.b_case(C.MAX_DIM + 1, 3, frames=[2])
    dfs = dict(fs, a=dev(fs["a"]), b=dev(fs["b"]), count=dev(fs["count"]))
    with pytest.raises(api.KhError, match="supported 1 ... 63"):
        api.fmllr_accumulate(dev(feats), dfs)


# ---------------------------------------------------------------- C and end to end
@pytest.fixture(scope="module")
def e2e(oracle):
    return C.e2e_reference(oracle)


def test_stages_on_the_end_to_end_case(api, e2e):
    """A1 within its bounds, A2 bit for bit on the restatement's posteriors, B within its bound, on the larger case."""
    am, feats, utt, spk, posts, tid2pdf = e2e["case"]
    ent = e2e["ent"]
    post, like = api.gmm_component_posteriors(Am(api, am), dev(feats), ent)
    assert (np.abs(post.cpu().numpy().astype(np.float64) - e2e["post"]) <= C.post_bound(e2e["post"], ent["goff"])).all()
    assert (np.abs(like.cpu().numpy().astype(np.float64) - e2e["like"]) <= C.like_bound(e2e["like"], ent["goff"])).all()
    got = api.fmllr_frame_stats(Am(api, am), dev(feats), utt, spk, ent, dev(e2e["post"]))
    _frame_stats_equal(got, e2e["fs"])
    _check_b(api, feats, e2e["fs"])


@pytest.mark.parametrize("update_type", C.TYPES)
def test_estimate_fmllr(api, e2e, update_type):
    am, feats, utt, spk, posts, tid2pdf = e2e["case"]
    w_ref, impr_ref, count_ref = e2e["ref"][update_type]
    opts = api.fmllr_options(update_type, C.E2E_MIN_COUNT, 40)
    W, impr, count, stats = api.estimate_fmllr(Am(api, am), dev(feats), utt, spk, posts=posts, tid2pdf=tid2pdf, opts=opts, return_stats=True)
    tol = C.transform_tolerance(w_ref, update_type)
    err = np.abs(W.astype(np.float64) - w_ref)
    print(update_type, "max err", err.max(), "tolerance", tol.min(), "timings", api.fmllr_last_timings())
    assert (err <= tol).all()
    assert np.allclose(count, count_ref, rtol=1e-6) and np.allclose(impr, impr_ref, rtol=1e-4, atol=1e-3)
    assert np.array_equal(W[3], np.eye(13, 14, dtype=np.float32)) and impr[3] == 0.0       # under the min-count
    st = e2e["stats"]
    for s in range(3):
        Gf = R.full_g(st["G"][s], 13)
        f_ref = R.aux(w_ref[s], st["beta"][s], st["K"][s], Gf)
        f_got = R.aux(W[s], st["beta"][s], st["K"][s], Gf)
        assert f_got >= f_ref - C.aux_drop_allowed(w_ref[s], tol[s], st["beta"][s], st["K"][s], st["G"][s]), s
    # transform-feats on the result, the project's 1e-4
    for s in range(4):
        r0, r1 = int(utt[spk[s]]), int(utt[spk[s + 1]])
        got = api.transform_feats(dev(W[s]), dev(feats[r0:r1])).cpu().numpy()
        assert np.abs(got - R.transform_feats(w_ref[s], feats[r0:r1])).max() < 1e-4


def test_estimate_fmllr_per_utterance_and_gpost_route(api, e2e):
    am, feats, utt, spk, posts, tid2pdf = e2e["case"]
    opts = api.fmllr_options("full", C.E2E_MIN_COUNT, 40)
    dam = Am(api, am)
    # per utterance = one speaker per utterance
    per_utt = np.arange(len(utt), dtype=np.int32)
    W, impr, count = api.estimate_fmllr(dam, dev(feats), utt, per_utt, posts=posts, tid2pdf=tid2pdf, opts=opts)
    ref = R.estimate(am, feats, utt, per_utt, e2e["ent"], dict(update_type="full", min_count=C.E2E_MIN_COUNT, num_iters=40), post=e2e["post"])
    err = np.abs(W.astype(np.float64) - ref["W"])
    print("per utterance: max err", err.max(), "tolerance", C.transform_tolerance(ref["W"], "full", per_utt=True).min())
    assert (err <= C.transform_tolerance(ref["W"], "full", per_utt=True)).all()
    assert np.allclose(count, ref["count"], rtol=1e-6) and (count < C.E2E_MIN_COUNT).sum() == 3      # 84, 38 and 39 counted frames
    # the gpost route with the same model gives what the post route gives
    W1, impr1, count1 = api.estimate_fmllr(dam, dev(feats), utt, spk, posts=posts, tid2pdf=tid2pdf, opts=opts)
    gposts, like, weight = api.gmm_post_to_gpost(dam, dev(feats), api.convert_posterior_to_pdfs(tid2pdf, posts))
    W2, impr2, count2 = api.estimate_fmllr(dam, dev(feats), utt, spk, gposts=gposts, opts=opts)
    assert np.array_equal(W1, W2) and np.array_equal(impr1, impr2) and np.array_equal(count1, count2)
    # two models: the statistics come from the second one's means and variances
    am2 = C.other_model(am, 9)
    W3, _, _ = api.estimate_fmllr(dam, dev(feats), utt, spk, gposts=gposts, opts=opts, gpost_am=Am(api, am2))
    ent_g, flat = C.gpost_entries(gposts)
    ref3 = R.estimate(am, feats, utt, spk, ent_g, dict(update_type="full", min_count=C.E2E_MIN_COUNT, num_iters=40), post=flat, acc_am=am2)
    assert (np.abs(W3.astype(np.float64) - ref3["W"]) <= C.transform_tolerance(ref3["W"], "full")).all()
    assert not np.array_equal(W3, W2)


def test_transform_feats_cases(api, rng):
    feats = rng.standard_normal((37, 13)).astype(np.float32)
    for cols in (13, 14):
        tr = rng.standard_normal((9, cols)).astype(np.float32)
        got = api.transform_feats(dev(tr), dev(feats)).cpu().numpy()
        assert got.shape == (37, 9) and np.abs(got - R.transform_feats(tr, feats)).max() < 1e-4
    with pytest.raises(api.KhError, match="forgot the --b-is-affine"):
        api.transform_feats(dev(rng.standard_normal((13, 15)).astype(np.float32)), dev(feats))
    with pytest.raises(api.KhError, match="bad dimension 13x12"):
        api.transform_feats(dev(rng.standard_normal((13, 12)).astype(np.float32)), dev(feats))
