"""CPU (the determinizer is host code and loads without a device): tools/lattice_determinize_pruned.py in process and
through its bin/ shim - options, the zero-scale error, scale / unscale, the "did not succeed" warning forced with a tiny
--max-mem, text and binary tables of both lattice kinds, the closing line and the exit status."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, pkg

sys.path.insert(0, os.path.join(ROOT, "tools"))
F = np.float32


def tool():
    return importlib.import_module("lattice_determinize_pruned")


def word_lattice(seed, n_frames=6, width=3, n_words=4):
    """A time-synchronous state-level lattice: one transition-id per arc, a word on some of them, final costs on the last
    frame's states.  Dyadic weights, so that a power-of-two acoustic scale is exact."""
    rng = np.random.default_rng(seed)
    states, n = [[0]], 1
    for _ in range(n_frames):
        k = int(rng.integers(1, width + 1))
        states.append(list(range(n, n + k)))
        n += k
    arcs = []
    for t in range(n_frames):
        for s in states[t]:
            for d in states[t + 1]:
                if rng.random() < 0.75 or s == states[t][0] or d == states[t + 1][0]:
                    w = int(rng.integers(1, n_words + 1)) if rng.random() < 0.4 else 0
                    arcs.append((s, d, int(rng.integers(1, 30)), w, float(rng.integers(0, 48)) / 16, float(rng.integers(0, 48)) / 16))
    A = np.array(arcs)
    fg = np.full(n, np.inf, F)
    for s in states[n_frames]:
        fg[s] = F(rng.integers(0, 32)) / F(16)
    fa = np.where(fg == np.inf, F(np.inf), F(0.0)).astype(F)
    return dict(num_states=n, start=0, state_frame=np.zeros(n, np.int32), arc_src=A[:, 0].astype(np.int32), arc_dst=A[:, 1].astype(np.int32),
                arc_il=A[:, 2].astype(np.int32), arc_ol=A[:, 3].astype(np.int32), arc_g=A[:, 4].astype(F), arc_a=A[:, 5].astype(F),
                state_final=fg.copy(), state_final_graph=fg, state_final_acoustic=fa)


def write_table(path, kind, keyed, text=False):
    cli = pkg("kaldi_cli")
    w = cli.TableWriter("ark%s:%s" % (",t" if text else "", path), kind)
    for k, x in keyed:
        w.write(k, x)
    w.close()


def read_clats(path):
    return list(pkg("kaldi_cli").SequentialTableReader("ark:%s" % path, "compact_lattice"))


def same(got, want):
    assert int(got["n_states"]) == int(want["n_states"])
    for k in ("arc_src", "arc_dst", "arc_label"):
        assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), k
    for k in ("arc_g", "arc_a", "final_g", "final_a"):
        assert np.asarray(got[k], F).tobytes() == np.asarray(want[k], F).tobytes(), k
    for k in ("arc_string", "final_string"):
        assert [list(map(int, x)) for x in got[k]] == [list(map(int, x)) for x in want[k]], k


def in_process(L, acoustic_scale, beam, **kw):
    """What the tool computes, from the library call alone: scale, determinize, scale back by the double 1.0 / float."""
    api = pkg("api")
    s = float(F(acoustic_scale))
    S = dict(L)
    S["arc_a"] = (s * np.asarray(L["arc_a"], np.float64)).astype(F)
    det = api.determinize_lattice_pruned(S, beam, phone_determinize=False, word_determinize=True, **kw)
    inv = 1.0 / s
    det["arc_a"] = (inv * np.asarray(det["arc_a"], np.float64)).astype(F)
    fa = np.asarray(det["final_a"], F)
    with np.errstate(invalid="ignore"):
        det["final_a"] = np.where(np.asarray(det["final_g"], F) == np.inf, F(np.inf), (inv * fa.astype(np.float64)).astype(F)).astype(F)
    return det


@pytest.fixture
def lats(tmp_path):
    keyed = [("utt%d" % i, word_lattice(40 + i)) for i in range(4)]
    write_table(tmp_path / "in.ark", "lattice", keyed)
    return tmp_path, keyed


def test_options_and_usage(lats, capfd):
    d, _ = lats
    t = tool()
    assert t.main(["ark:%s" % (d / "in.ark")]) == 1                               # two arguments, or the usage
    assert "Usage: lattice-determinize-pruned [options] lattice-rspecifier lattice-wspecifier" in capfd.readouterr().err
    assert t.main(["--max-loop=500000", "ark:%s" % (d / "in.ark"), "ark:%s" % (d / "o.ark")]) == 255
    assert "--max-loop=500000" in capfd.readouterr().err
    assert t.main(["--max-loop=0", "--delta=0.0009765625", "--max-mem=50000000", "--minimize=false", "--beam=6.0", "--acoustic-scale=0.1",
                   "ark:%s" % (d / "in.ark"), "ark:%s" % (d / "o.ark")]) == 0
    err = capfd.readouterr().err
    assert "LOG (lattice-determinize-pruned:main()) Done 4 lattices, determinization finished earlier than specified by the beam on 0 of these." in err
    assert t.main(["--no-such-option=1", "ark:%s" % (d / "in.ark"), "ark:%s" % (d / "o.ark")]) != 0


def test_zero_acoustic_scale_is_the_reference_s_error(lats, capfd):
    d, _ = lats
    assert tool().main(["--acoustic-scale=0.0", "ark:%s" % (d / "in.ark"), "ark:%s" % (d / "o.ark")]) == 255
    assert "Do not use a zero acoustic scale (cannot be inverted)" in capfd.readouterr().err


@pytest.mark.parametrize("scale,beam", [(1.0, 10.0), (0.25, 3.0), (0.083333, 6.0)])
def test_scale_determinize_unscale_equals_the_library_call(lats, scale, beam):
    d, keyed = lats
    assert tool().main(["--acoustic-scale=%r" % scale, "--beam=%r" % beam, "ark:%s" % (d / "in.ark"), "ark:%s" % (d / "o.ark")]) == 0
    got = read_clats(d / "o.ark")
    assert [k for k, _ in got] == [k for k, _ in keyed]
    for (_, g), (_, L) in zip(got, keyed):
        same(g, in_process(L, scale, beam))
        assert g["n_states"] > 1


def test_the_scale_decides_which_path_survives_and_is_taken_out_again(tmp_path):
    """Two arcs with the same word: at scale 1 the second is cheaper (3 + 1 < 1 + 4), at 0.25 the first (1 + 1 < 3 + 0.25); the
    acoustic cost written is the unscaled one."""
    n = 2
    fg = np.asarray([np.inf, 0.0], F)
    L = dict(num_states=n, start=0, state_frame=np.zeros(n, np.int32), arc_src=np.asarray([0, 0], np.int32), arc_dst=np.asarray([1, 1], np.int32),
             arc_il=np.asarray([1, 2], np.int32), arc_ol=np.asarray([5, 5], np.int32), arc_g=np.asarray([1.0, 3.0], F),
             arc_a=np.asarray([4.0, 1.0], F), state_final=fg, state_final_graph=fg, state_final_acoustic=np.asarray([np.inf, 0.0], F))
    write_table(tmp_path / "in.ark", "lattice", [("u", L)])
    for scale, tid, g, a in ((1.0, 2, 3.0, 1.0), (0.25, 1, 1.0, 4.0)):
        assert tool().main(["--acoustic-scale=%r" % scale, "ark:%s" % (tmp_path / "in.ark"), "ark:%s" % (tmp_path / "o.ark")]) == 0
        (_, c), = read_clats(tmp_path / "o.ark")
        assert len(c["arc_src"]) == 1 and int(c["arc_label"][0]) == 5
        strings = [int(x) for x in c["arc_string"][0]] + [int(x) for s in c["final_string"] for x in s]
        assert strings == [tid]
        assert float(c["arc_g"].sum() + c["final_g"][np.isfinite(c["final_g"])].sum()) == g
        assert float(c["arc_a"].sum() + c["final_a"][np.isfinite(c["final_a"])].sum()) == a


def test_incomplete_determinization_warns_and_is_counted(tmp_path, capfd):
    keyed = [("big", word_lattice(3, n_frames=14, width=4, n_words=6)), ("small", word_lattice(41))]
    write_table(tmp_path / "in.ark", "lattice", keyed)
    assert tool().main(["--max-mem=1", "--beam=50", "ark:%s" % (tmp_path / "in.ark"), "ark:%s" % (tmp_path / "o.ark")]) == 0
    err = capfd.readouterr().err
    incomplete = [k for k, L in keyed if not in_process(L, 1.0, 50.0, max_mem=1)["complete"]]
    assert incomplete                                                             # the limit stops at least one of them early
    for k, _ in keyed:
        line = ("WARNING (lattice-determinize-pruned:main()) For key %s, determinization did not succeed"
                "(partial output will be pruned tighter than the specified beam.)" % k)
        assert (line in err) == (k in incomplete), k
    n_warn = len(incomplete)
    assert ("LOG (lattice-determinize-pruned:main()) Done 2 lattices, determinization finished earlier than specified by the beam on %d of these."
            % n_warn) in err
    got = dict(read_clats(tmp_path / "o.ark"))
    same(got["big"], in_process(keyed[0][1], 1.0, 50.0, max_mem=1))


@pytest.mark.parametrize("text", [False, True])
def test_text_and_binary_tables_of_both_kinds(lats, text):
    """A CompactLattice table is read as SequentialLatticeReader reads it (converted to a Lattice): the same result as for
    the Lattice it expands to."""
    d, keyed = lats
    kio = pkg("kaldi_io")
    write_table(d / "l.ark", "lattice", keyed, text)
    first = [(k, in_process(L, 1.0, 10.0)) for k, L in keyed]
    write_table(d / "c.ark", "compact_lattice", first, text)
    t = tool()
    assert t.main(["ark:%s" % (d / "l.ark"), "ark:%s" % (d / "o1.ark")]) == 0
    for (_, g), (_, w) in zip(read_clats(d / "o1.ark"), first):
        if text:                       # (text tables hold %.7g)
            assert g["n_states"] == w["n_states"] and np.allclose(g["arc_a"], w["arc_a"], rtol=1e-6)
        else:
            same(g, w)
    assert t.main(["--beam=8", "ark:%s" % (d / "c.ark"), "ark,t:%s" % (d / "o2.txt")]) == 0
    got = list(pkg("kaldi_cli").SequentialTableReader("ark:%s" % (d / "o2.txt"), "compact_lattice"))
    assert [k for k, _ in got] == [k for k, _ in keyed]
    for (_, g), (k, c) in zip(got, first):
        want = in_process(kio.compact_lattice_to_lattice(c), 1.0, 8.0)
        assert g["n_states"] == want["n_states"] and np.array_equal(g["arc_label"], want["arc_label"])
        assert np.allclose(g["arc_g"], want["arc_g"], rtol=1e-6) and np.allclose(g["arc_a"], want["arc_a"], rtol=1e-6)


def test_no_lattices_exit_status_and_the_shim(tmp_path):
    write_table(tmp_path / "empty.ark", "lattice", [])
    env = dict(os.environ, PATH=os.path.join(ROOT, "bin") + os.pathsep + os.environ["PATH"], PYTHON=sys.executable)
    p = subprocess.run(["bash", "-c", "lattice-determinize-pruned ark:empty.ark ark:o.ark"], cwd=tmp_path, env=env, capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 1
    assert "LOG (lattice-determinize-pruned:main()) Done 0 lattices, determinization finished earlier than specified by the beam on 0 of these." in p.stderr
    write_table(tmp_path / "in.ark", "lattice", [("a", word_lattice(44))])
    p = subprocess.run(["bash", "-c", "set -o pipefail; cat in.ark | lattice-determinize-pruned --acoustic-scale=0.083333 --beam=6.0 ark:- "
                        "'ark:|gzip -c > lat.gz' && gunzip -c lat.gz > lat.ark"], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    (k, c), = read_clats(tmp_path / "lat.ark")
    same(c, in_process(word_lattice(44), 0.083333, 6.0))
