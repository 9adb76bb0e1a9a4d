"""GPU: the iVector kernels (csrc/kh_ivector.hip) at the sizes of tests/ivector_cases.py - the K-tail, scalar and mixed
tile edges of the fp64 GEMM, the scalar tail and the one-wave / two-wave edge of the solve, the split of a Gaussian's postings
into work items, several count / scatter blocks, the accepted maxima of every kernel and the LDS limit - against
oracle/ivector_oracle.py.  tests/test_ivector_cases.py asserts on the CPU that each case reaches what it is here for and that
its inputs are separated well enough for the device to select and prune as the oracle does.

Tolerances (those of tests/test_gpu_ivector.py): iVector rows 2e-4 absolute; state num_frames 1e-5; linear term and rebuilt
quadratic term rtol 1e-4, atol 5e-5; CMVN sums rtol 1e-9, atol 1e-6; batch against per-utterance accumulation 1e-6.

Per-Gaussian counts (state[lo + S:]), Gaussian by Gaussian against counts accumulated from the oracle's posteriors: over all
the runs of the table, the counts from the oracle's float32 posteriors and from a float64 recomputation of the chain differ by
at most 5.2e-6 relative (measured on the CPU, tests/test_ivector_cases.py keeps the figure); the device, float with another
summation order, is allowed 4 x that: ivector_cases.COUNT_RTOL = 2.08e-5 relative.  A Gaussian the oracle leaves at zero
is exactly zero on the device."""
import importlib

import numpy as np
import pytest
import torch

import ivector_cases as C
from oracle import ivector_oracle as IO

pytestmark = pytest.mark.gpu
api = importlib.import_module("old-kaldi-git_amd.api")
capi = importlib.import_module("old-kaldi-git_amd.capi")
TOL = 2e-4


def offsets(utts):
    return np.concatenate([[0], np.cumsum([len(u) for u in utts])]).astype(np.int32)


def device_feats(utts, stride=None):
    """The utterances row-concatenated on the device; stride: as a column block of a wider matrix whose other columns are NaN."""
    x = np.concatenate(utts, 0)
    if stride is None:
        return torch.as_tensor(x, device="cuda")
    wide = torch.full((x.shape[0], stride), float("nan"), dtype=torch.float32, device="cuda")
    view = wide[:, 3:3 + x.shape[1]]
    view.copy_(torch.as_tensor(x))
    return view


def split(out, off):
    out = out.cpu().numpy()
    return [out[off[i]:off[i + 1]] for i in range(len(off) - 1)]


def check_rows(got, run, what):
    for i, (g, (want, _)) in enumerate(zip(got, run["want"])):
        assert g.shape == want.shape
        err = np.abs(g - want).max()
        print("%s utterance %d: rows max abs err %.2e" % (what, i, err))
        np.testing.assert_allclose(g, want, rtol=0, atol=TOL, err_msg="%s utterance %d" % (what, i))


def check_stats(st, ost, want_counts, m, B, S, what, exact_count=None):
    """The OnlineIvectorEstimationStats part of a device state against the oracle's."""
    lo = 2 * (B + 1) + 2
    U, _ = IO.derived(m)
    r_, c_ = IO.packed_index(S)
    assert abs(st[lo - 2] - ost["num_frames"]) < 1e-5, what
    np.testing.assert_allclose(st[lo:lo + S], ost["lin"], rtol=1e-4, atol=5e-5, err_msg=what)
    quad = np.eye(S) * st[lo - 1]
    Q = np.zeros((S, S))
    Q[r_, c_] = st[lo + S:] @ U
    quad += Q + np.tril(Q, -1).T
    np.testing.assert_allclose(quad, ost["quad"], rtol=1e-4, atol=5e-5, err_msg=what)
    got = st[lo + S:]
    assert got.shape == want_counts.shape
    assert np.array_equal(got[want_counts == 0.0], np.zeros(int((want_counts == 0.0).sum()))), what
    nz = want_counts != 0.0
    rel = (np.abs(got - want_counts)[nz] / want_counts[nz]).max() if nz.any() else 0.0
    print("%s: counts max rel err %.2e (bound %.2e)" % (what, rel, C.COUNT_RTOL))
    assert rel <= C.COUNT_RTOL, (what, rel)
    if exact_count is not None:
        assert abs(got[0] - exact_count) <= 1e-6 * exact_count, (what, got[0], exact_count)


def check_states(states, run, prev_counts, B, S, I, what, exact=False):
    """[n x state_dim] device states after a run; prev_counts: the counts the states started from.  Returns the oracle's counts."""
    m = run["model"]
    out = []
    for j, ((_, ost), tr) in enumerate(zip(run["want"], run["traces"])):
        want_counts = C.counts(tr["post32"], I) + (prev_counts[j] if prev_counts is not None else 0.0)
        np.testing.assert_allclose(states[j, :2 * (B + 1)].reshape(2, B + 1), ost["cmvn"], rtol=1e-9, atol=1e-6)
        exact_count = float(np.float32(m["posterior_scale"])) * len(run["utts"][j]) if exact else None
        check_stats(states[j], ost, want_counts, m, B, S, "%s utterance %d" % (what, j), exact_count)
        out.append(want_counts)
    return out


def run_streams(ext, run, n_utts, S, B, I, explicit_weights, what):
    """The first n_utts utterances through OnlineIvectorStreams with all weights 1, in two get_frames calls."""
    utts = run["utts"][:n_utts]
    off = offsets(utts)
    feats = device_feats(utts)
    out = torch.zeros((int(off[-1]), S), dtype=torch.float32, device="cuda")
    streams = api.OnlineIvectorStreams(ext, feats, off, out)
    if explicit_weights:
        for i, u in enumerate(utts):
            streams.update_frame_weights(i, [(t, 1.0) for t in range(len(u))], len(u))
    first = [max(0, len(u) // 2 - 1) for u in utts]
    streams.get_frames(list(range(n_utts)), first)
    rest = [i for i, u in enumerate(utts) if first[i] < len(u) - 1]
    streams.get_frames(rest, [len(utts[i]) - 1 for i in rest])
    api.synchronize()
    sub = dict(run, utts=utts, want=run["want"][:n_utts], traces=run["traces"][:n_utts])
    check_rows(split(out, off), sub, what)
    st = streams.get_stats(np.zeros((n_utts, ext.state_dim())))
    for j in range(n_utts):
        check_stats(st[j], sub["want"][j][1], C.counts(sub["traces"][j]["post32"], I), run["model"], B, S, "%s utterance %d" % (what, j))


@pytest.mark.parametrize("name", list(C.CASES))
def test_case_matches_the_specification(name, monkeypatch):
    c = C.CASES[name]
    B, S, I = c["base"], c["S"], c["I"]
    K = C.kernel_constants()
    runs = C.oracle_runs(name)
    plain = runs[0]
    m, utts = plain["model"], plain["utts"]
    off = offsets(utts)
    feats = device_feats(utts, c["feat_stride"])
    ext = api.OnlineIvectorExtractor(m)
    # the batch path
    batch = split(ext.extract(feats, off), off)
    api.synchronize()
    check_rows(batch, plain, name + " batch")
    # ... with the state returned: the same kernels also write the statistics
    out, st = ext.extract(feats, off, state=ext.fresh_state(len(utts)), return_state=True)
    api.synchronize()
    for a, b in zip(batch, split(out, off)):
        np.testing.assert_allclose(a, b, rtol=0, atol=1e-6)
    check_states(st, plain, None, B, S, I, name + " state", exact=(I == 1))
    # in chunks of utterances (non-zero row and point offsets of a chunk)
    if c["max_rows"]:
        monkeypatch.setenv("KH_IVECTOR_MAX_ROWS", str(c["max_rows"]))
        many = split(ext.extract(feats, off), off)
        api.synchronize()
        monkeypatch.delenv("KH_IVECTOR_MAX_ROWS")
        check_rows(many, plain, name + " chunks")
        for a, b in zip(batch, many):
            np.testing.assert_allclose(a, b, rtol=0, atol=1e-6)
    # the per-utterance accumulation (a model whose share of LDS does not fit there takes the batched path)
    monkeypatch.setenv("KH_IVECTOR_SEQUENTIAL", "1")
    seq = split(ext.extract(feats, off), off)
    api.synchronize()
    monkeypatch.delenv("KH_IVECTOR_SEQUENTIAL")
    check_rows(seq, plain, name + " sequential")
    for a, b in zip(batch, seq):
        np.testing.assert_allclose(a, b, rtol=0, atol=1e-6)
    # the streams
    need = C.lds_need(K, c["feat"], S, m["num_gselect"])
    if c["streams"]:
        assert need["stream"] <= K["kLdsLimit"]
        run_streams(ext, plain, 2 if name == "multi_block" else len(utts), S, B, I, name == "odd_dims", name + " streams")
    elif need["stream"] > K["kLdsLimit"]:
        # refused at construction, with the limit named: nothing is launched
        with pytest.raises(capi.KhError, match=r"streams kernel; the limit is %d" % K["kLdsLimit"]):
            api.OnlineIvectorStreams(ext, device_feats(utts), off, torch.zeros((int(off[-1]), S), dtype=torch.float32, device="cuda"))
    # use_most_recent_ivector + greedy, max_count, the adaptation state carried over two rounds
    if c["adapt"]:
        ext_a = api.OnlineIvectorExtractor(runs[1]["model"])
        dev = ext_a.fresh_state(len(utts))
        prev = None
        for rnd, run in enumerate(runs[1:]):
            f = device_feats(run["utts"])
            o = offsets(run["utts"])
            out, st = ext_a.extract(f, o, state=dev, return_state=True)
            api.synchronize()
            check_rows(split(out, o), run, "%s round %d" % (name, rnd))
            prev = check_states(st, run, prev, B, S, I, "%s round %d" % (name, rnd))
            # LimitFrames on both sides (the oracle's states of the next round went through IO.limit_frames)
            for j, (_, ost) in enumerate(run["want"]):
                lim = float(np.float32(C.MAX_REMEMBERED) * np.float32(run["model"]["posterior_scale"]))
                if ost["num_frames"] > lim:
                    prev[j] = prev[j] * (lim / ost["num_frames"])
            dev = ext_a.limit_frames(st.copy(), C.MAX_REMEMBERED)
        assert rnd == 1


def test_the_lds_limit_is_refused_at_create_with_the_limit_named():
    """One above lds_edge's iVector dimension: IvSolveKernel's static + dynamic LDS passes the limit; create() says so."""
    c = C.CASES["lds_edge"]
    K = C.kernel_constants()
    m, _ = C.make_model(c["seed"], c["base"], c["splice"], c["feat"], c["I"], c["S"] + 1)
    need = C.lds_need(K, c["feat"], c["S"] + 1, m["num_gselect"])
    with pytest.raises(capi.KhError) as e:
        api.OnlineIvectorExtractor(m)
    msg = str(e.value)
    print(msg)
    assert "the limit is %d" % K["kLdsLimit"] in msg and "%d" % need["solve"] in msg and "ivector-dim <= %d" % c["S"] in msg


def test_streams_refuse_a_model_their_kernel_cannot_hold_at_construction():
    """ivector_dim 110, feat_dim 40, num_gselect 16: create() accepts it (the batch kernels fit), the streams kernel would
    need 67 640 B of dynamic LDS alone; OnlineIvectorStreams refuses it when constructed, not at get_frames."""
    o = C.STREAMS_OVER
    K = C.kernel_constants()
    m, rng = C.make_model(1234, o["base"], o["splice"], o["feat"], o["I"], o["S"], num_gselect=o["num_gselect"])
    ext = api.OnlineIvectorExtractor(m)
    utts = C.make_utts(rng, o["base"], [6])
    off = offsets(utts)
    out = torch.zeros((6, o["S"]), dtype=torch.float32, device="cuda")
    with pytest.raises(capi.KhError) as e:
        api.OnlineIvectorStreams(ext, device_feats(utts), off, out)
    msg = str(e.value)
    print(msg)
    assert "the limit is %d" % K["kLdsLimit"] in msg and "%d" % C.lds_need(K, o["feat"], o["S"], o["num_gselect"])["stream"] in msg


@pytest.mark.parametrize("name", list(C.FALLBACK))
def test_exact_solve_fallback_at_odd_dimensions(name, monkeypatch):
    """LinearCgd's fall-back to SolveQuadraticProblem (test_gpu_ivector.py's recipe and tolerances) at S = 13 and S = 65: the
    cyclic Jacobi sweep pairs an odd dimension's last index with a dummy that never rotates.  The oracle fell back at least
    three times (asserted on the CPU too); batch kernel, per-utterance kernel and streams; six workgroups per launch."""
    f = C.FALLBACK[name]
    S = f["S"]
    m, utts = C.build_fallback(name)
    want, n_exact = C.fallback_oracle(name)
    assert n_exact >= f["min_exact"] and len(utts) <= 8
    ext = api.OnlineIvectorExtractor(m)
    off = offsets(utts)
    feats = device_feats(utts)

    def check(got, what):
        for i, (g_, w_) in enumerate(zip(got, want)):
            print("%s %s utterance %d: max abs err %.2e (values up to %.2e)" % (name, what, i, np.abs(g_ - w_).max(), np.abs(w_).max()))
            np.testing.assert_allclose(g_, w_, rtol=2e-4, atol=2e-4 * np.abs(w_).max(), err_msg=what)

    got = split(ext.extract(feats, off), off)
    api.synchronize()
    check(got, "batch")
    monkeypatch.setenv("KH_IVECTOR_SEQUENTIAL", "1")
    got = split(ext.extract(feats, off), off)
    api.synchronize()
    monkeypatch.delenv("KH_IVECTOR_SEQUENTIAL")
    check(got, "sequential")
    out = torch.zeros((int(off[-1]), S), dtype=torch.float32, device="cuda")
    st = api.OnlineIvectorStreams(ext, feats, off, out)
    st.get_frames(list(range(len(utts))), [len(u) - 1 for u in utts])
    api.synchronize()
    check(split(out, off), "streams")
