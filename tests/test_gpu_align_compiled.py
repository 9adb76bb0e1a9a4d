"""GPU: kh_align_compiled (csrc/kh_align.hip) through api.align_compiled against library mode of tests/align_restatement.py,
bit for bit: status, alignment, words, the double total cost, every path arc's two floats and the float weight.  That library
mode and the reference agree on these inputs is tests/test_align_restatement.py's business (CPU)."""
import numpy as np
import pytest

import align_cases as C
import align_restatement as R

pytestmark = pytest.mark.gpu


def bits(x):
    return np.asarray(x, np.float32).view(np.int32).tolist()


def device_ll(cases):
    import torch
    ll = np.ascontiguousarray(np.concatenate([c["loglikes"] for c in cases]))
    ro = np.concatenate([[0], np.cumsum([len(c["loglikes"]) for c in cases])]).astype(np.int32)
    return torch.from_numpy(ll).cuda(), ro


def same(got, want, name):
    assert got["status"] == want["status"], (name, got["status"], want["status"])
    assert got["retried"] == want["retried"], name
    assert list(got["alignment"]) == want["alignment"] and list(got["words"]) == want["words"], name
    if want["status"] != R.DONE:
        return
    assert got["cost"] == want["cost"], (name, got["cost"], want["cost"])
    assert got["best_state"] == want["best_state"], name
    assert [(a[0], a[1]) for a in got["path"]] == [(a[0], a[1]) for a in want["path"]], name
    assert bits([a[2] for a in got["path"]]) == bits([a[2] for a in want["path"]]), name
    assert bits([a[3] for a in got["path"]]) == bits([a[3] for a in want["path"]]), name
    assert bits(got["weight"]) == bits(want["weight"]) and bits(got["like"]) == bits(want["like"]), name


def check(api, cases, beam, retry_beam=0.0, min_active=20, **kw):
    assert all(np.array_equal(c["tid2pdf"], cases[0]["tid2pdf"]) for c in cases)
    ll, ro = device_ll(cases)
    got = api.align_compiled([c["graph"] for c in cases], ll, ro, cases[0]["tid2pdf"], beam, retry_beam, min_active=min_active, **kw)
    want = [R.align(c["graph"], c["loglikes"], c["tid2pdf"], beam, retry_beam, "library", min_active) for c in cases]
    for c, g, w in zip(cases, got, want):
        same(g, w, c["name"])
    return got, want


def test_hand_cases_one_call(api):
    """States 1, 3, ...; frames 1, 2, 37; eps chains before frame 0, within a frame and into the only final state on the last
    frame; an eps-reachable state that a cheaper emitting arc reaches too; a path longer than frames + arcs; 70 incoming
    arcs; unequal frames and states in one call."""
    cases = [c for c in C.hand_cases() if c["name"] != "float_rounding"]
    got, want = check(api, cases, 200.0, path_room=64)
    assert all(w["status"] == R.DONE for w in want)
    t = api.align_compiled_last_timings()
    assert t["launches"] == 1 and t["utts_launched"] == len(cases) and t["workspace_cost_utts"] == 0


def test_tie_rule(api):
    c = C.tie_case()
    got, want = check(api, [c], c["beam"])
    assert want[0]["had_tie"] and got[0]["alignment"] == [1, 1, 1] and got[0]["words"] == [51, 53, 55] and got[0]["best_state"] == 3


@pytest.mark.parametrize("n_states", [63, 64, 65, 255, 256, 257, 600])
def test_state_counts(api, n_states):
    """Wave and workgroup edges, and more states than lanes; many tokens (the padding states all hold one)."""
    c = C.generate(300 + n_states, n_words=2, pad_to=n_states)
    assert c["graph"]["num_states"] == n_states
    _, want = check(api, [c], 200.0)
    assert want[0]["status"] == R.DONE and want[0]["cut_beam"] > 0


def test_batch_of_five_unequal(api):
    cases = [C.generate(400, n_words=2), C.generate(401, n_words=4, pad_to=300), C.generate(402, n_words=1),
             C.generate(403, n_words=3, pad_to=65), C.generate(404, n_words=2, frames=60)]
    assert len({len(c["loglikes"]) for c in cases}) == 5 and len({c["graph"]["num_states"] for c in cases}) == 5
    check(api, cases, 200.0)


@pytest.mark.parametrize("min_active", [0, 2, 20])
@pytest.mark.parametrize("beam", [2.0, 4.0, 8.0, 40.0])
def test_min_active_and_beams(api, beam, min_active):
    """Frames with at most min_active tokens (infinite cutoff), frames where fewer than min_active + 1 float-rounded costs lie
    inside the beam (the selection), frames with many tokens inside it."""
    cases = [C.generate(s, n_words=2, pad_to=65) for s in (204, 213, 214, 222, 226)]
    _, want = check(api, cases, beam, min_active=min_active)
    seen = {k: sum(w.get(k, 0) for w in want) for k in ("cut_inf", "cut_select", "cut_beam")}
    if min_active == 20 and beam == 8.0:
        assert all(v > 0 for v in seen.values()), seen
    if min_active == 2 and beam == 4.0:
        assert seen["cut_select"] > 0 and seen["cut_inf"] > 0, seen


def test_float_rounded_selection(api):
    c = C.float_rounding_case()
    _, want = check(api, [c], c["beam"], min_active=c["min_active"])
    assert want[0]["cut_select"] == 1 and want[0]["status"] == R.DONE


def test_retry_and_failure(api):
    """beam 2 fails and retry 40 succeeds (200); both fail (205) and the others of the batch are not affected; 201 too short
    to reach the final state at any beam."""
    short = C.generate(201, n_words=3, frames=4)
    cases = [C.generate(200, n_words=2, pad_to=65), C.generate(205, n_words=2, pad_to=65), short, C.generate(213, n_words=2, pad_to=65)]
    got, want = check(api, cases, 2.0, retry_beam=40.0, min_active=2)
    assert [w["status"] for w in want] == [R.DONE, R.NO_FINAL, R.NO_FINAL, R.DONE]
    assert [g["retried"] for g in got] == [True, True, True, True]
    got, want = check(api, cases, 40.0, min_active=2)
    assert [g["retried"] for g in got] == [False] * 4 and got[0]["status"] == R.DONE


def test_refusals(api):
    c = C.hand_cases()[0]
    ll, ro = device_ll([c])
    for beam, retry in ((0.0, 0.0), (-1.0, 0.0), (10.0, 10.0), (10.0, 5.0)):
        with pytest.raises(api.KhError):
            api.align_compiled([c["graph"]], ll, ro, c["tid2pdf"], beam, retry)
    with pytest.raises(api.KhError):      # rows beyond the matrix
        api.align_compiled([c["graph"]], ll, np.asarray([0, len(c["loglikes"]) + 1], np.int32), c["tid2pdf"], 10.0)


def test_workspace_costs_equal_lds_costs(api):
    cases = [C.generate(s, n_words=2, pad_to=p) for s, p in ((500, 0), (501, 65), (502, 257))]
    try:
        api.align_compiled_set_lds_states(64)          # the first in LDS, the others in the workspace, one launch
        check(api, cases, 200.0)
        t = api.align_compiled_last_timings()
        assert t["workspace_cost_utts"] == 2 and t["launches"] == 1
        api.align_compiled_set_lds_states(0)
        check(api, cases, 8.0, min_active=2)
        assert api.align_compiled_last_timings()["workspace_cost_utts"] == 3
    finally:
        api.align_compiled_set_lds_states(3584)
    check(api, cases, 8.0, min_active=2)
    assert api.align_compiled_last_timings()["workspace_cost_utts"] == 0


def test_workspace_limit_splits_the_batch(api):
    cases = [C.generate(600 + i, n_words=2, pad_to=65, frames=30) for i in range(6)]
    one = 4 * 31 * 65                                    # backpointers of one utterance
    check(api, cases, 200.0, workspace_limit=3 * one + 64)
    t = api.align_compiled_last_timings()
    assert t["launches"] >= 2 and t["utts_launched"] == 6
    got = api.align_compiled([c["graph"] for c in cases], *device_ll(cases), cases[0]["tid2pdf"], 200.0, workspace_limit=one - 4)
    assert [g["status"] for g in got] == [api.ALIGNC_TOO_LARGE] * 6 and all(g["alignment"] == [] for g in got)
    assert api.align_compiled_last_timings()["launches"] == 0


def test_needs_more_path_room(api):
    cases = [c for c in C.hand_cases() if c["name"] in ("eps_cycle_every_frame", "one_state_T2", "eps_chains_T37")]
    ll, ro = device_ll(cases)
    A = api.align_compiled_pack([c["graph"] for c in cases])
    r = api.align_compiled_call(A, ll, ro, cases[0]["tid2pdf"], 200.0, 20, 0.5, [2, 2, 2])
    want = [R.decode_library(c["graph"], c["loglikes"], c["tid2pdf"], 200.0) for c in cases]
    assert [c["name"] for c in cases] == ["one_state_T2", "eps_chains_T37", "eps_cycle_every_frame"]
    assert r["status"].tolist() == [R.DONE, R.NEEDS_ROOM, R.NEEDS_ROOM]
    assert r["path_len"].tolist() == [len(w["path"]) for w in want] and r["cost"].tolist() == [w["cost"] for w in want]
    check(api, cases, 200.0, path_room=2)               # the host calls again with the room that was named


def test_bad_input_is_not_launched(api):
    good = C.hand_cases()[3]
    bad_next = dict(good, graph=dict(good["graph"], nextstate=good["graph"]["nextstate"].copy()))
    bad_next["graph"]["nextstate"][1] = good["graph"]["num_states"]
    bad_label = dict(good, graph=dict(good["graph"], ilabel=good["graph"]["ilabel"].copy()))
    bad_label["graph"]["ilabel"][0] = len(good["tid2pdf"])
    cases = [bad_next, good, bad_label, C.negative_eps_cycle_case()]
    ll, ro = device_ll(cases)
    got = api.align_compiled([c["graph"] for c in cases], ll, ro, good["tid2pdf"], 200.0)
    assert [g["status"] for g in got] == [api.ALIGNC_BAD_INPUT, api.ALIGNC_DONE, api.ALIGNC_BAD_INPUT, api.ALIGNC_BOUND]
    t = api.align_compiled_last_timings()
    assert t["utts_launched"] == 2
    want = R.align(good["graph"], good["loglikes"], good["tid2pdf"], 200.0)
    same(got[1], want, "good")
    assert R.decode_library(cases[3]["graph"], cases[3]["loglikes"], good["tid2pdf"], 200.0)["status"] == R.BOUND


def test_careful(api):
    cases = [c for c in C.hand_cases() if c["name"] in ("two_finals", "eps_chains_T37")]
    ll, ro = device_ll(cases)
    got = api.align_compiled([c["graph"] for c in cases], ll, ro, cases[0]["tid2pdf"], 200.0, careful=True)
    for c, g in zip(cases, got):
        w = R.align(api.modify_graph_for_careful_alignment(c["graph"]), c["loglikes"], c["tid2pdf"], 200.0)
        same(g, w, c["name"])
        plain = R.align(c["graph"], c["loglikes"], c["tid2pdf"], 200.0)
        assert w["alignment"] == plain["alignment"] and w["words"] == plain["words"]


@pytest.mark.parametrize("kind", ["gmm", "nnet"])
def test_tools_end_to_end(api, kind, tmp_path, monkeypatch, capfd):
    """gmm-align-compiled / nnet-align-compiled on files written by kaldi_io's own writers: a tiny transition model with the
    golden AmDiagGmm / AmNnet body (5 pdfs, 6-dim features), a graphs archive, a feature archive with one key missing.
    Alignments and scores equal library mode run on the same scored matrix; log lines and exit status as the binaries'."""
    import importlib
    import os
    import sys
    import torch
    from conftest import ROOT, pkg
    kio, cli = pkg("kaldi_io"), pkg("kaldi_cli")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    tool = importlib.import_module("gmm_align_compiled" if kind == "gmm" else "nnet_align_compiled")
    monkeypatch.chdir(tmp_path)
    n_pdf, acwt = 5, 0.1
    topo = dict(phones=list(range(1, n_pdf + 1)), phone2idx=[-1] + [0] * n_pdf, entries=[[(0, [(0, 0.5), (1, 0.5)]), (-1, [])]])
    triples = [(p + 1, 0, (3 * p) % n_pdf) for p in range(n_pdf)]
    log_probs = np.concatenate([[0.0], np.log(np.tile([0.75, 0.25], n_pdf))]).astype(np.float32)
    body = "am_gmm_body_bin" if kind == "gmm" else "am_nnet_body_bin"
    with open("final.mdl", "wb") as f:
        f.write(b"\0B")
        kio.write_transition_model(f, topo, triples, log_probs, True)
        f.write(open(os.path.join(ROOT, "tests", "golden", "kaldi_io", body), "rb").read())
    rng = np.random.default_rng(77)
    graphs = {"u0": C.chain_graph(rng, 5, eps_every=3, n_pdf=10), "u1": C.chain_graph(rng, 9, eps_every=2, n_pdf=10),
              "u2": C.chain_graph(rng, 3, n_pdf=10), "u3": C.chain_graph(rng, 40, n_pdf=10), "u4": C.chain_graph(rng, 4, n_pdf=10)}
    w = cli.TableWriter("ark:graphs.ark", "fst")
    for k, g in graphs.items():
        w.write(k, g)
    w.close()
    feats = {"u0": rng.standard_normal((12, 6)).astype(np.float32), "u1": rng.standard_normal((30, 6)).astype(np.float32),
             "u3": rng.standard_normal((9, 6)).astype(np.float32), "u4": rng.standard_normal((7, 6)).astype(np.float32)}   # u2 missing; u3 too short
    with kio.TableWriter("feats.ark") as fw:
        for k, m in feats.items():
            fw.write(k, m)
    opts = ["--beam=3", "--retry-beam=60", "--acoustic-scale=%g" % acwt, "--transition-scale=1.0", "--self-loop-scale=0.1"]
    if kind == "nnet":
        opts.append("--use-gpu=no")
    rc = tool.main(opts + ["final.mdl", "ark:graphs.ark", "ark:feats.ark", "ark:ali.ark", "ark,t:scores.txt"])
    err = capfd.readouterr().err
    assert rc == 0
    # the same scores, by the tool's own scoring code on the same batch
    if kind == "gmm":
        tm, am = cli.read_kaldi_object("final.mdl", lambda s, b: (kio.read_transition_model(s, b), kio.read_am_diag_gmm(s, b)))
        gconsts, _ = api.gmm_compute_gconsts(am["weights"], am["means_invvars"], am["inv_vars"])
        gmm = api.AmDiagGmm(gconsts, am["means_invvars"], am["inv_vars"], am["pdf_offsets"])
        score = lambda x, off: gmm.pdf_log_likelihoods(x)
    else:
        tm, (comps, priors) = cli.read_kaldi_object("final.mdl", lambda s, b: (kio.read_transition_model(s, b), kio.read_am_nnet(s, b)))
        nnet = api.Nnet(comps, priors)
        score = lambda x, off: nnet.compute(x, off, pad_input=True, epilogue=True, prob_scale=acwt)[0]
    keys = list(feats)
    off = np.concatenate([[0], np.cumsum([len(feats[k]) for k in keys])]).astype(np.int32)
    ll = score(torch.from_numpy(np.concatenate([feats[k] for k in keys])).cuda(), off)
    if kind == "gmm":
        api.scale(ll, acwt)
    ll = ll.cpu().numpy()
    ali = dict(kio.read_ark("ali.ark", kind="int32_vector"))
    scores = {l.split()[0]: np.float32(l.split()[1]) for l in open("scores.txt")}
    n_done = n_retry = 0
    tot_like, tot_frames = 0.0, 0
    for i, k in enumerate(keys):
        g = api.add_transition_probs(graphs[k], tm, 1.0, 0.1)
        want = R.align(g, ll[off[i]:off[i + 1]], tm["tid2pdf"], 3.0, 60.0, "library")
        n_retry += want["retried"]
        if want["status"] != R.DONE:
            assert k not in ali and k not in scores
            assert ("Did not successfully decode file %s, len = %d" % (k, len(feats[k]))) in err
            continue
        n_done += 1
        assert ali[k].tolist() == want["alignment"], k
        terms = [abs(x) for a in want["path"] for x in (a[2], a[3])] + [abs(float(g["final"][want["best_state"]]))]
        bound = 2 * (len(want["path"]) - 1) * 2.0 ** -24 * sum(terms)
        print(kind, k, "score", scores[k], "restatement", want["like"], "bound", bound)
        assert abs(float(scores[k]) - want["like"]) <= bound, k
        tot_like += float(np.float32(np.float32(want["like"]) / np.float32(acwt)))
        tot_frames += len(feats[k])
        if want["retried"]:
            assert ("Retrying utterance %s with beam 60" % k) in err
    assert n_done >= 2 and n_retry >= 1 and n_done < len(keys)
    prog = "%s-align-compiled" % kind
    assert ("WARNING (%s:main()) No features for utterance u2" % prog) in err
    assert ("LOG (%s:main()) Overall log-likelihood per frame is %g over %d frames." % (prog, tot_like / tot_frames, tot_frames)) in err
    assert ("LOG (%s:main()) Retried %d out of %d utterances." % (prog, n_retry, len(graphs))) in err
    assert ("LOG (%s:main()) Done %d, errors on %d" % (prog, n_done, len(graphs) - n_done)) in err
