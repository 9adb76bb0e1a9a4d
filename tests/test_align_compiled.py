"""CPU: the host layers of forced alignment - api.add_transition_probs (AddTransitionProbs, hmm/hmm-utils.cc:776-830),
api.modify_graph_for_careful_alignment (decoder-wrappers.cc:393-420), the command line of tools/align_compiled.py (options,
usage, exit status, the beam refusal, the warnings about the inputs) and the base_float table.  No device."""
import importlib
import io
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, pkg

import align_cases as C
import align_restatement as R

GOLD = os.path.join(ROOT, "tests", "golden", "kaldi_io")


def tmodel():
    """Phone 1: three states, the last without a self-loop.  Phone 2: one state whose self-loop has probability 1.
    Transition-ids: 1 self / 2 forward (state 0), 3 self / 4 forward (state 1), 5 forward (state 2), 6 self / 7 forward."""
    kio = pkg("kaldi_io")
    topo = dict(phones=[1, 2], phone2idx=[-1, 0, 1],
                entries=[[(0, [(0, 0.6), (1, 0.4)]), (1, [(1, 0.7), (2, 0.3)]), (2, [(3, 1.0)]), (-1, [])],
                         [(0, [(0, 0.5), (1, 0.5)]), (-1, [])]])
    triples = [(1, 0, 0), (1, 1, 1), (1, 2, 2), (2, 0, 3)]
    log_probs = np.asarray([0.0, np.log(0.6), np.log(0.4), np.log(0.7), np.log(0.3), 0.0, 0.0, np.log(1e-3)], np.float32)
    f = io.BytesIO()
    kio.write_transition_model(f, topo, triples, log_probs, True)
    f.seek(0)
    return kio.read_transition_model(kio.Stream(f), True), log_probs.astype(np.float64)


def graph_of_all_tids():
    arcs = [(0, 0, t, 0, np.float32(0.25 * t)) for t in range(1, 8)] + [(0, 1, 0, 9, np.float32(1.5))]
    return C.make_graph(2, 0, arcs, {1: 0.0})


@pytest.mark.parametrize("ts,sl", [(1.0, 1.0), (0.5, 0.5), (1.0, 0.1), (1.0, 0.0)])
def test_add_transition_probs(ts, sl):
    api = pkg("api")
    tm, lp = tmodel()
    assert api.transition_id_to_state(tm).tolist() == [0, 1, 1, 2, 2, 3, 4, 4]
    g = graph_of_all_tids()
    out = api.add_transition_probs(g, tm, ts, sl)
    # by hand, in double: the non-self-loop log-prob of each transition-state (0 without a self-loop, log 1e-10 where the
    # self-loop takes everything), then GetScaledTransitionLogProb's two branches
    nsl = {1: np.log(1 - 0.6), 2: np.log(1 - 0.7), 3: 0.0, 4: np.log(1e-10)}
    state, self_loop = {1: 1, 2: 1, 3: 2, 4: 2, 5: 3, 6: 4, 7: 4}, {1, 3, 6}
    want = []
    for t in range(1, 8):
        if ts == sl:
            scaled = ts * lp[t]
        elif t in self_loop:
            scaled = sl * lp[t]
        else:
            scaled = sl * nsl[state[t]] + ts * (lp[t] - nsl[state[t]])
        want.append(0.25 * t - scaled)
    np.testing.assert_allclose(out["weight"][:7], want, rtol=2e-6, atol=1e-6)
    assert out["weight"][7] == np.float32(1.5)                      # the eps arc is not touched
    assert g["weight"][0] == np.float32(0.25)                       # nor the input
    for k in ("ilabel", "olabel", "nextstate", "final", "arc_offsets"):
        assert np.array_equal(out[k], g[k])
    if (ts, sl) == (1.0, 0.0):
        assert out["weight"][0] == np.float32(0.25) and out["weight"][5] == np.float32(1.5)   # self-loops cost nothing
        np.testing.assert_allclose(out["weight"][4], 1.25, rtol=1e-6)     # no self-loop: the forward arc has probability 1
        np.testing.assert_allclose(out["weight"][6], 1.75 - (np.log(1e-3) - np.log(1e-10)), rtol=1e-6)


def test_add_transition_probs_invalid_label():
    api = pkg("api")
    tm, _ = tmodel()
    g = graph_of_all_tids()
    g["ilabel"] = g["ilabel"].copy()
    g["ilabel"][2] = 8
    with pytest.raises(api.KhError, match="invalid symbol 8 on graph input side"):
        api.add_transition_probs(g, tm, 1.0, 0.1)


def test_careful_graph():
    """Two final states: each gets an eps arc with its final weight to the new state and stops being final; the copy has no
    final state and is entered from the new state, the only final one (weight One)."""
    api = pkg("api")
    c = [c for c in C.hand_cases() if c["name"] == "two_finals"][0]
    g = c["graph"]
    S = g["num_states"]
    out = api.modify_graph_for_careful_alignment(g)
    assert out["num_states"] == 2 * S + 1 and out["start"] == g["start"]
    off = out["arc_offsets"]
    arcs = {s: [(int(out["nextstate"][a]), int(out["ilabel"][a]), int(out["olabel"][a]), float(out["weight"][a])) for a in range(off[s], off[s + 1])]
            for s in range(2 * S + 1)}
    old = {s: [(int(g["nextstate"][a]), int(g["ilabel"][a]), int(g["olabel"][a]), float(g["weight"][a])) for a in range(g["arc_offsets"][s], g["arc_offsets"][s + 1])]
           for s in range(S)}
    assert arcs[0] == old[0]
    assert arcs[1] == old[1] + [(2 * S, 0, 0, 6.0)] and arcs[2] == old[2] + [(2 * S, 0, 0, 0.5)]
    for s in range(S):
        assert arcs[S + s] == [(d + S, i, o, w) for (d, i, o, w) in old[s]]
    assert arcs[2 * S] == [(S + g["start"], 0, 0, 0.0)]
    assert np.all(np.isinf(out["final"][:2 * S])) and out["final"][2 * S] == 0.0
    # what it is for: the same alignment, and a path may go round through the copy
    plain = R.align(g, c["loglikes"], c["tid2pdf"], 200.0)
    careful = R.align(out, c["loglikes"], c["tid2pdf"], 200.0)
    assert careful["status"] == R.DONE and careful["alignment"] == plain["alignment"] and careful["cost"] == plain["cost"]


def test_refusals_need_no_device():
    api = pkg("api")
    for beam, retry in ((0.0, 0.0), (-2.0, 0.0), (10.0, 10.0), (10.0, 4.0)):
        with pytest.raises(api.KhError, match="Beams do not make sense"):
            api.align_compiled([], None, [0], None, beam, retry)


def test_linear_symbol_sequence():
    api = pkg("api")
    path = [(0, 7, np.float32(0.1), np.float32(0.0)), (3, 0, np.float32(0.2), np.float32(1.5)), (4, 8, np.float32(0.3), np.float32(2.5))]
    ali, words, (g, a) = api.linear_symbol_sequence(path, np.float32(0.7))
    assert ali == [3, 4] and words == [7, 8]
    assert g == np.float32(np.float32(np.float32(np.float32(0.1) + np.float32(0.2)) + np.float32(0.3)) + np.float32(0.7)) and a == np.float32(4.0)


# ------------------------------------------------------------------------------------------------------------ the tool
@pytest.fixture
def files(tmp_path, monkeypatch):
    """A model (transition model + the golden AmDiagGmm body: 5 pdfs, 6-dim features), three graphs and a feature archive
    that lacks one key and holds one empty matrix."""
    kio, cli = pkg("kaldi_io"), pkg("kaldi_cli")
    monkeypatch.chdir(tmp_path)
    n_pdf = 5
    topo = dict(phones=list(range(1, n_pdf + 1)), phone2idx=[-1] + [0] * n_pdf, entries=[[(0, [(0, 0.5), (1, 0.5)]), (-1, [])]])
    triples = [(p + 1, 0, p) for p in range(n_pdf)]
    log_probs = np.concatenate([[0.0], np.log(np.tile([0.75, 0.25], n_pdf))]).astype(np.float32)
    with open("final.mdl", "wb") as f:
        f.write(b"\0B")
        kio.write_transition_model(f, topo, triples, log_probs, True)
        f.write(open(os.path.join(GOLD, "am_gmm_body_bin"), "rb").read())
    rng = np.random.default_rng(5)
    w = cli.TableWriter("ark:graphs.ark", "fst")
    for k in ("a", "b", "c"):
        w.write(k, C.chain_graph(rng, 4, n_pdf=2 * n_pdf))
    w.close()
    with kio.TableWriter("feats.ark") as fw:
        fw.write("a", rng.standard_normal((9, 6)).astype(np.float32))
        fw.write("c", np.zeros((0, 6), np.float32))
    return tmp_path


def tool(kind):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    return importlib.import_module("gmm_align_compiled" if kind == "gmm" else "nnet_align_compiled")


@pytest.mark.parametrize("kind", ["gmm", "nnet"])
def test_tool_usage_and_argument_counts(kind, capfd, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    t = tool(kind)
    for args in ([], ["m", "ark:g"], ["m", "ark:g", "ark:f"], ["m", "ark:g", "ark:f", "ark:a", "ark:s", "extra"]):
        assert t.main(args) == 1
        err = capfd.readouterr().err
        assert ("Usage:   %s-align-compiled [options] model-in graphs-rspecifier" % kind) in err
    with pytest.raises(SystemExit) as e:                         # ParseOptions::Read: PrintUsage(); exit(0)
        t.main(["--help"])
    assert e.value.code == 0
    err = capfd.readouterr().err
    for opt in ("--beam", "--retry-beam", "--careful", "--transition-scale", "--acoustic-scale", "--self-loop-scale"):
        assert opt in err
    assert ("--use-gpu" in err) == (kind == "nnet")
    assert "(float, default = 200)" in err
    assert t.main(["--no-such-option=1", "m", "ark:g", "ark:f", "ark:a"]) == 255
    capfd.readouterr()


def test_tool_dry_path_warnings_and_exit_status(files, capfd):
    t = tool("gmm")
    rc = t.main(["--dry-run=true", "--beam=10", "--retry-beam=40", "--transition-scale=1.0", "--self-loop-scale=0.1", "--careful=true",
                 "final.mdl", "ark:graphs.ark", "ark:feats.ark", "ark:ali.ark", "ark,t:scores.txt"])
    err = capfd.readouterr().err
    assert rc == 1                                               # nothing aligned
    assert "WARNING (gmm-align-compiled:main()) No features for utterance b" in err
    assert "WARNING (gmm-align-compiled:main()) Zero-length utterance: c" in err
    assert "LOG (gmm-align-compiled:main()) Overall log-likelihood per frame is nan over 0 frames." in err
    assert "LOG (gmm-align-compiled:main()) Retried 0 out of 2 utterances." in err
    assert "LOG (gmm-align-compiled:main()) Done 0, errors on 2" in err
    assert os.path.getsize("ali.ark") == 0 and os.path.getsize("scores.txt") == 0


def test_tool_beam_refusal(files, capfd):
    t = tool("gmm")
    for opts in (["--beam=0"], ["--beam=10", "--retry-beam=10"], ["--beam=10", "--retry-beam=5"]):
        assert t.main(["--dry-run=true"] + opts + ["final.mdl", "ark:graphs.ark", "ark:feats.ark", "ark:ali.ark"]) == 255
        assert "Beams do not make sense: beam" in capfd.readouterr().err
    # thrown by the first utterance that is aligned: with no usable utterance the binary never gets there
    with pkg("kaldi_io").TableWriter("none.ark") as fw:
        fw.write("zzz", np.zeros((3, 6), np.float32))
    assert t.main(["--dry-run=true", "--beam=0", "final.mdl", "ark:graphs.ark", "ark:none.ark", "ark:ali.ark"]) == 1
    assert "Beams do not make sense" not in capfd.readouterr().err


def test_tool_invalid_label_is_an_error(files, capfd):
    cli = pkg("kaldi_cli")
    g = C.chain_graph(np.random.default_rng(6), 3, n_pdf=10)
    g["ilabel"][0] = 11                                          # the model has 10 transition-ids
    w = cli.TableWriter("ark:bad.ark", "fst")
    w.write("a", g)
    w.close()
    assert tool("gmm").main(["--dry-run=true", "final.mdl", "ark:bad.ark", "ark:feats.ark", "ark:ali.ark"]) == 255
    assert "AddTransitionProbs: invalid symbol 11 on graph input side." in capfd.readouterr().err


def test_base_float_table(tmp_path, monkeypatch):
    """BasicHolder<BaseFloat>::Write (kaldi-holder-inl.h): binary = "\\0B", the size byte 4 and the float; text = the number
    and a newline."""
    cli = pkg("kaldi_cli")
    monkeypatch.chdir(tmp_path)
    w = cli.TableWriter("ark:scores.ark", "base_float")
    w.write("utt1", np.float32(-12.5))
    w.write("utt2", np.float32(0.25))
    w.close()
    assert open("scores.ark", "rb").read() == b"utt1 \0B\x04" + np.float32(-12.5).tobytes() + b"utt2 \0B\x04" + np.float32(0.25).tobytes()
    w = cli.TableWriter("ark,t:scores.txt", "base_float")
    w.write("utt1", np.float32(-12.5))
    w.close()
    assert open("scores.txt").read() == "utt1 -12.5 \n"       # WriteBasicType leaves a space behind the number


@pytest.mark.parametrize("name", ["gmm-align-compiled", "nnet-align-compiled"])
def test_bin_shims(name, tmp_path):
    """The reference's executable names: a wrong argument count prints the usage and exits with 1, through the shim."""
    import subprocess
    shim = os.path.join(ROOT, "bin", name)
    assert os.access(shim, os.X_OK)
    p = subprocess.run([shim, "only-one-argument"], capture_output=True, text=True, cwd=str(tmp_path), env=dict(os.environ, PYTHON=sys.executable))
    assert p.returncode == 1 and ("Usage:   %s [options] model-in graphs-rspecifier" % name) in p.stderr
