"""CPU: the oracle path and the depth (lattice-oracle, lattice-depth).  The restatement (latoracle_restatement.py) that
checks the kernel on the GPU is itself checked here against brute force - the minimum Levenshtein distance over every
complete path - and on hand lattices; its walk back is checked to be a real path whose moves reproduce the counts; the
tools' logic runs with the device call replaced by the restatement; the new entry points exist and refuse to run without
a device."""
import io
import os
import re

import numpy as np
import pytest

from conftest import ROOT, pkg

import latoracle_cases
import latoracle_restatement as R

WILD = (9,)


def _api():
    return pkg("api")


def restated(clat, ref, wildcards=(), **masks):
    """The restatement in the layout of api.compact_lattice_oracle."""
    csr = _api().compact_lattice_to_prune_csr(clat)
    r = R.oracle(csr, ref, wildcards, **masks)
    if r["errors"] < 0:
        return dict(r, words=[], path_arcs=[])
    arcs = np.asarray(r["path_arcs"], np.int64)
    labels = np.asarray(csr["arc_label"])[arcs]
    words = [int(w) for w in labels if R.map_word(w, set(wildcards)) != 0]
    return dict(r, words=words, path_arcs=np.asarray(csr["perm"])[arcs], csr=csr)


def check_walk(csr, ref, wildcards, r, arc_keep=None, final_keep=None):
    """The traced path is a start-to-final path over kept arcs, and replaying its moves against the reference gives the
    counts."""
    wild = set(wildcards)
    off, nxt = np.asarray(csr["arc_offsets"], np.int64), np.asarray(csr["arc_nextstate"], np.int64)
    src = np.repeat(np.arange(csr["n_states"]), np.diff(off))
    refw = [int(w) for w in ref if R.map_word(w, wild) != 0]
    assert r["R"] == len(refw)
    s = int(csr["start"])
    for a in r["path_arcs"]:
        assert src[a] == s and (arc_keep is None or arc_keep[a])
        s = int(nxt[a])
    assert s == r["final_state"] and R.is_final_of(csr)[s] and (final_keep is None or final_keep[s])
    assert r["correct"] + r["sub"] + r["del"] == len(refw)
    assert r["sub"] + r["ins"] + r["del"] == r["errors"]
    j, cnt, arcs = 0, dict(correct=0, sub=0, ins=0, eps=0, **{"del": 0}), []
    for kind, a, _ in r["moves"]:
        w = 0 if a is None else R.map_word(csr["arc_label"][a], wild)
        if kind == "del":
            j += 1
        elif kind == "eps":
            assert w == 0
        elif kind == "ins":
            assert w != 0
        elif kind == "correct":
            assert w != 0 and w == refw[j]
            j += 1
        else:
            assert kind == "sub" and w != 0 and w != refw[j]
            j += 1
        cnt[kind] += 1
        if a is not None:
            arcs.append(a)
    assert j == len(refw) and arcs == list(r["path_arcs"])
    assert [cnt[k] for k in ("correct", "sub", "ins", "del")] == [r[k] for k in ("correct", "sub", "ins", "del")]


@pytest.mark.parametrize("seed", range(240))
def test_restatement_against_brute_force(seed):
    """Random acyclic lattices of at most 10 states and 3 arcs per state over 3 words, epsilon and one wildcard, references
    of 0 to 6 words (wildcards among them): ties are everywhere.  Every fourth case drops arcs and finals by a mask, every
    fifth has its start state behind state 0."""
    rng = np.random.default_rng(4100 + seed)
    n = int(rng.integers(1, 11))
    start = int(rng.integers(0, n)) if seed % 5 == 4 else 0
    clat = R.random_word_clat(rng, n, start=start, last_final=bool(rng.random() < 0.9))
    csr = _api().compact_lattice_to_prune_csr(clat)
    assert csr["start"] == start
    ref = [int(x) for x in rng.choice([1, 2, 3, 9], size=int(rng.integers(0, 7)))]
    ak = fk = None
    if seed % 4 == 3:
        ak, fk = rng.random(len(csr["arc_label"])) < 0.8, rng.random(n) < 0.8
    r = R.oracle(csr, ref, WILD, arc_keep=ak, final_keep=fk)
    assert r["errors"] == R.brute_force(csr, ref, WILD, ak, fk)
    if r["errors"] >= 0:
        check_walk(csr, ref, WILD, r, ak, fk)
    else:
        assert len(r["path_arcs"]) == 0 and r["final_state"] == -1


@pytest.mark.parametrize("case", latoracle_cases.all_cases(), ids=lambda c: c[0])
def test_hand_lattices_through_the_restatement(case):
    name, clat, ref, wild, want = case
    got = restated(clat, ref, wild)
    latoracle_cases.check_result(got, want, name)
    if got["errors"] >= 0:
        check_walk(got["csr"], ref, wild, got)
        assert got["errors"] == R.brute_force(got["csr"], ref, wild)
    if "moves" in want:
        assert [m[0] for m in got["moves"]] == want["moves"]


def test_no_kept_final_gives_minus_one():
    name, clat, ref, wild, want = latoracle_cases.skip_arc_picks_the_matching_path()
    assert restated(clat, ref, wild, final_keep=np.zeros(4, bool))["errors"] == -1
    assert restated(clat, ref, wild, arc_keep=np.array([True, False, True, False]))["errors"] == 2


def test_frame_sum_is_the_depth_numerator():
    """Unmasked: every arc's and every state's string; masked: the kept arcs and the kept finals of surviving states - a
    kept final on a state Connect removed is not counted."""
    name, clat, ref, wild, want = latoracle_cases.skip_arc_picks_the_matching_path()
    clat["final_string"][3] = np.array([5, 6], np.int32)
    clat["final_g"][1] = clat["final_a"][1] = np.float32(0.0)
    clat["final_string"][1] = np.array([7, 7, 7], np.int32)
    csr = _api().compact_lattice_to_prune_csr(clat)
    af, ff = R.frames_of(clat, csr)
    assert R.oracle(csr, ref, wild, arc_frames=af, final_frames=ff)["frame_sum"] == 4 + 2 + 3
    keep = dict(arc_keep=np.array([False, True, False, True]), state_keep=np.array([True, False, True, True]), final_keep=np.ones(4, bool))
    assert R.oracle(csr, ref, wild, arc_frames=af, final_frames=ff, **keep)["frame_sum"] == 2 + 2
    d, t = R.compact_lattice_depth(clat)        # times: state 1 at 1 (+3), state 3 at 2 (+2): inconsistent, the longer one
    assert t == 4 and d == np.float32(9) / np.float32(4)


def consistent_clat(rng, n):
    """A chain 0 -> 1 -> ... plus random arcs; an arc s -> d carries d - s frames and a final weight the rest, so every
    state is reachable and the state times are consistent (the reference asserts both)."""
    pairs = [(s, s + 1) for s in range(n - 1)] + [(int(s), int(rng.integers(s + 1, n))) for s in rng.integers(0, max(n - 1, 1), size=n) if s < n - 1]
    arcs = [(s, d, int(rng.integers(0, 4)), 0.25 * int(rng.integers(0, 20)), 0.25 * int(rng.integers(0, 20)), list(range(1, d - s + 1)))
            for s, d in pairs]
    finals = {s: (0.0, 0.5, list(range(n - 1 - s))) for s in range(n) if s == n - 1 or rng.random() < 0.2}
    return R.make_clat(n, arcs, finals)


def test_api_depth_against_the_restatement():
    api = _api()
    rng = np.random.default_rng(7)
    for n in (1, 2, 7, 30):
        clat = consistent_clat(rng, n)
        d, t = api.compact_lattice_depth(clat)
        d2, t2 = R.compact_lattice_depth(clat)
        assert t == t2 and d == d2 and d.dtype == np.float32
    empty = pkg("kaldi_io").read_compact_lattice(io.BytesIO(b"\n"), binary=False)
    assert api.compact_lattice_depth(empty) == (np.float32(1.0), 0)
    name, clat, ref, wild, want = latoracle_cases.no_final()
    assert api.compact_lattice_depth(clat) == (np.float32(1.0), 0) and R.compact_lattice_depth(clat) == (np.float32(1.0), 0)
    bad = latoracle_cases.skip_arc_picks_the_matching_path()[1]
    bad["arc_string"][0] = np.array([1, 2, 3], np.int32)
    with pytest.raises(pkg("capi").KhError, match="CompactLatticeStateTimes"):
        api.compact_lattice_depth(bad)


def test_mask_words_layout():
    """bit p % 64 of word p / 64, as kh_compact_lattice_prune writes its masks."""
    api = _api()
    m = np.zeros((2, 65), bool)
    m[0, 0] = m[0, 63] = m[1, 64] = m[1, 3] = True
    w = api._mask_words(m, 65)
    assert w.dtype == np.uint64 and w.shape == (2, 2)
    assert w.tolist() == [[(1 << 63) | 1, 0], [8, 1]]


# ---------------------------------------------------------------- the entry points
def test_entry_points_declared_and_loud_without_a_device():
    import torch
    capi = pkg("capi")
    lib = capi.load()
    names = ("kh_compact_lattice_oracle", "kh_compact_lattice_oracle_set_workspace_limit", "kh_compact_lattice_oracle_last_timings")
    header = open(os.path.join(ROOT, "include", "kaldi_hip.h")).read()
    for n in names:
        assert n in capi.SIGNATURES and hasattr(lib, n) and n + "(" in header
    api = _api()
    empty = pkg("kaldi_io").read_compact_lattice(io.BytesIO(b"\n"), binary=False)
    res = api.compact_lattice_oracle([empty], [[1, 2]])           # no start state: no device call
    assert res[0][0]["errors"] == -1 and res[0][0]["depth"] == np.float32(1.0) and res[0][0]["num_frames"] == 0
    if torch.cuda.is_available():
        return
    csr = api.compact_lattice_to_prune_csr(latoracle_cases.tie_lower_arc_number()[1])
    with pytest.raises(capi.KhError, match="no HIP device"):
        api.compact_lattice_oracle_raw([csr], [0], [[3]], ())


# ---------------------------------------------------------------- the tools' logic, the device call replaced by the restatement
def restated_oracle(clats, refs, wildcards=(), points=None, beams=None):
    """api.compact_lattice_oracle's contract from the two restatements: PruneLattice restated per beam, the oracle path on
    its masks, CompactLatticeDepth restated on the pruned lattice."""
    import latprune_restatement as P
    api = _api()
    K = 1 if beams is None else len(beams)
    out = []
    for clat, ref in zip(clats, refs):
        row = []
        for p in range(K):
            if int(clat["n_states"]) == 0 or int(clat.get("start", 0)) < 0:
                row.append(dict(errors=-1, depth=np.float32(1.0), num_frames=0))
                continue
            csr = api.compact_lattice_to_prune_csr(clat)
            masks, kept = {}, clat
            if beams is not None:
                scale, pen = points[0]
                pr = P.prune_lattice(csr, scale, pen, beams[p])
                masks = dict(arc_keep=pr["arc_keep"], state_keep=pr["state_keep"], final_keep=pr["final_keep"])
                kept = P.prune_clat(clat, csr, scale, pen, beams[p])
            r = R.oracle(csr, ref, wildcards, **masks)
            arcs = np.asarray(r["path_arcs"], np.int64)
            labels = np.asarray(csr["arc_label"])[arcs] if len(arcs) else np.zeros(0, np.int32)
            r["words"] = np.asarray([w for w in labels if R.map_word(w, set(wildcards)) != 0], np.int32)
            r["depth"], r["num_frames"] = R.compact_lattice_depth(kept) if "arc_string" in clat and int(kept.get("start", 0)) <= 0 else (None, None)
            row.append(r)
        out.append(row)
    return out


def write_archive(tmp_path, clats, refs, name="in"):
    cli = pkg("kaldi_cli")
    w = cli.TableWriter("ark,t:%s" % (tmp_path / (name + ".lats")), "compact_lattice")
    for k, c in clats:
        w.write(k, c)
    w.close()
    (tmp_path / (name + ".ref")).write_text("".join("%s %s\n" % (k, " ".join(str(x) for x in r)) for k, r in refs))
    return "ark:%s" % (tmp_path / (name + ".lats")), "ark:%s" % (tmp_path / (name + ".ref"))


def small_archive(n=5, seed=3):
    rng = np.random.default_rng(seed)
    clats = [("utt%d" % i, consistent_clat(rng, int(rng.integers(2, 9)))) for i in range(n)]
    refs = [(k, [int(x) for x in rng.integers(1, 5, size=int(rng.integers(0, 6)))]) for k, _ in clats]
    return clats, refs


def _tool(name):
    return __import__("tools." + name, fromlist=["main"])


@pytest.fixture
def restated_device(monkeypatch):
    """The tools with the library's two device entry points replaced: the restatement for the oracle call, nothing for the
    device selection."""
    api = _api()
    monkeypatch.setattr(api, "compact_lattice_oracle", restated_oracle)
    monkeypatch.setattr(api, "select_gpu", lambda *a, **k: None)


def test_oracle_tool_overall_line_fields_and_missing_reference(tmp_path, capfd, restated_device):
    """The fields steps/oracle_wer.sh's awk line reads ($7 errors, $9 words, $10 insertions, $12 deletions, $14
    substitutions), the per-utterance lines, the transcriptions and the edit distances, with one key absent from the
    reference and one lattice without a final state."""
    clats, refs = small_archive()
    clats.append(("nofinal", latoracle_cases.no_final()[1]))
    refs.append(("nofinal", [1]))
    rs, ref_rs = write_archive(tmp_path, clats, refs[1:])           # utt0 has no reference
    tool = _tool("lattice_oracle")
    rc = tool.main(["--wildcard-symbols=4:77", rs, ref_rs, "ark,t:%s" % (tmp_path / "tra"), "ark,t:%s" % (tmp_path / "edits")])
    err = capfd.readouterr().err
    assert rc == 0
    want = [restated_oracle([c], [r], (4, 77))[0][0] for (_, c), (_, r) in list(zip(clats, refs))[1:-1]]
    overall = [l for l in err.splitlines() if re.search(r"\bOverall\b", l)]
    assert len(overall) == 1
    f = overall[0].split()              # awk's fields, 1-based: f[i - 1]
    assert f[2] == "Overall" and f[3] == "%WER" and f[5] == "[" and f[7] == "/"
    tot = lambda k: sum(r[k] for r in want)
    n_words = sum(len([w for w in r if w != 4]) for _, r in refs[1:-1])
    assert int(f[6]) == tot("errors") and int(f[8].rstrip(",")) == n_words == tot("correct") + tot("sub") + tot("del")
    assert (int(f[9]), int(f[11]), int(f[13])) == (tot("ins"), tot("del"), tot("sub"))
    assert f[10] == "insertions," and f[12] == "deletions," and f[14:] == ["substitutions", "]"]
    assert float(f[4]) == float("%g" % (100.0 * tot("errors") / n_words))
    assert "Scored 5 lattices, 2 not present in ref." in err
    assert "WARNING (lattice-oracle:main()) No reference present for utterance utt0" in err
    assert "WARNING (lattice-oracle:main()) Best-path failed for key nofinal" in err
    assert "Lattice utt0 read." in err and "For utterance utt1, best cost %g" % want[0]["errors"] in err
    r = want[0]
    assert "%%WER %s [ %d / %d, %d insertions, %d deletions, %d sub ]" % (
        tool.cxx_ratio(100.0 * r["errors"], r["R"]), r["errors"], r["R"], r["ins"], r["del"], r["sub"]) in err
    tra = (tmp_path / "tra").read_text().splitlines()
    assert tra == ["%s %s" % (k, "".join("%d " % w for w in r["words"])) for (k, _), r in zip(clats[1:-1], want)]
    assert (tmp_path / "edits").read_text().splitlines() == ["%s %d " % (k, r["errors"]) for (k, _), r in zip(clats[1:-1], want)]


def test_oracle_tool_refusals_and_beam_substitution(tmp_path, capfd, restated_device):
    clats, refs = small_archive(2)
    rs, ref_rs = write_archive(tmp_path, clats, refs)
    tool = _tool("lattice_oracle")
    out = "ark,t:%s" % (tmp_path / "tra_BEAM")
    assert tool.main([rs, ref_rs]) == 1
    assert "Usage: lattice-oracle [options] <test-lattice-rspecifier>" in capfd.readouterr().err
    assert tool.main(["--write-lattices=ark:/dev/null", rs, ref_rs, out]) == 255
    assert "--write-lattices" in capfd.readouterr().err
    assert tool.main(["--beams=2,4", rs, ref_rs, "ark,t:%s" % (tmp_path / "same")]) == 255
    assert "must differ per point" in capfd.readouterr().err
    assert tool.main(["--beams=2,4", rs, ref_rs, out, "ark,t:%s" % (tmp_path / "edits")]) == 255
    assert tool.main(["--beams=0,4", rs, ref_rs, out]) == 134
    assert tool.main(["--acoustic-scale=0.5", rs, ref_rs, out]) == 255
    assert tool.main(["--wildcard-symbols=a:b", rs, ref_rs, out]) == 255
    assert tool.main(["--wildcard-symbols-list=x", "--wildcard-symbols=3", rs, ref_rs, out]) == 134
    assert tool.main(["--wildcard-symbols-list=x", rs, ref_rs, out]) == 134
    err = capfd.readouterr().err
    assert "--wildcard-symbols-list option deprecated." in err and "requires --word-symbol-table option" in err
    assert not list(tmp_path.glob("tra_*")) and not (tmp_path / "same").exists()
    assert tool.kt.beam_specs("ark:x_BEAM.tra", ["2", "4.5"]) == ["ark:x_2.tra", "ark:x_4.5.tra"]
    # the sweep: one file and one Overall line per beam; a wide beam gives the unpruned answer
    assert tool.main(["--acoustic-scale=0.5", "--beams=0.25,1000", rs, ref_rs, out]) == 0
    err = capfd.readouterr().err
    assert len(re.findall(r"\[BEAM=0.25\] Overall %WER", err)) == 1 and len(re.findall(r"\[BEAM=1000\] Overall %WER", err)) == 1
    assert tool.main([rs, ref_rs, "ark,t:%s" % (tmp_path / "plain")]) == 0
    assert (tmp_path / "tra_1000").read_text() == (tmp_path / "plain").read_text()
    assert (tmp_path / "tra_0.25").exists()


def test_oracle_tool_symbol_table_lines_and_lattice_input(tmp_path, capfd, restated_device):
    """--word-symbol-table's two debug lines, --wildcard-symbols-list, and a table of state-level Lattices."""
    kio, cli = pkg("kaldi_io"), pkg("kaldi_cli")
    name, clat, ref, wild, want = latoracle_cases.wildcard_both_sides()
    w = cli.TableWriter("ark,t:%s" % (tmp_path / "lat"), "lattice")
    lat = kio.compact_lattice_to_lattice(clat)
    w.write("k", dict(lat, state_frame=np.zeros(lat["num_states"], np.int32)))
    w.close()
    (tmp_path / "ref").write_text("k %s\n" % " ".join(str(x) for x in ref))
    (tmp_path / "words.txt").write_text("<eps> 0\none 1\ntwo 2\n<unk> 9\n")
    (tmp_path / "wild").write_text("<unk>\n")
    tool = _tool("lattice_oracle")
    rc = tool.main(["--word-symbol-table=%s" % (tmp_path / "words.txt"), "--wildcard-symbols-list=%s" % (tmp_path / "wild"),
                    "ark:%s" % (tmp_path / "lat"), "ark:%s" % (tmp_path / "ref"), "ark,t:%s" % (tmp_path / "tra")])
    err = capfd.readouterr().err
    assert rc == 0 and "k (oracle) one two \n" in err and "k (reference) one two \n" in err
    assert "Overall %WER 0 [ 0 / 2, 0 insertions, 0 deletions, 0 substitutions ]" in err
    assert (tmp_path / "tra").read_text() == "k 1 2 \n"


def test_depth_tool_overall_line_and_exit_status(tmp_path, capfd, restated_device):
    """$6 and $8 of the Overall line against CompactLatticeDepth restated; the depth table; exit status 1 when nothing
    was done; the sweep's per-beam lines."""
    clats, refs = small_archive(4, seed=11)
    rs, _ = write_archive(tmp_path, clats, refs)
    tool = _tool("lattice_depth")
    assert tool.main([rs, "ark,t:%s" % (tmp_path / "depth")]) == 0
    err = capfd.readouterr().err
    want = [R.compact_lattice_depth(c) for _, c in clats]
    num, den = sum(float(np.float32(d) * np.float32(t)) for d, t in want), float(sum(t for _, t in want))
    f = [l for l in err.splitlines() if re.search(r"\bOverall\b", l)][0].split()
    assert f[2:5] == ["Overall", "density", "is"] and f[6] == "over" and f[8] == "frames."
    assert f[5] == "%g" % (num / den) and f[7] == "%g" % den
    assert "LOG (lattice-depth:main()) Done 4 lattices." in err
    got = [l.split() for l in (tmp_path / "depth").read_text().splitlines()]
    assert [k for k, _ in got] == [k for k, _ in clats] and [np.float32(float(v)) for _, v in got] == [np.float32("%.7g" % d) for d, _ in want]
    (tmp_path / "none.lats").write_text("")
    assert tool.main(["ark:%s" % (tmp_path / "none.lats")]) == 1
    assert "Done 0 lattices." in capfd.readouterr().err
    assert tool.main([rs, rs, rs]) == 1
    assert tool.main(["--beams=1,2", rs, "ark,t:%s" % (tmp_path / "d")]) == 255
    capfd.readouterr()
    assert tool.main(["--beams=0.25,1000", rs, "ark,t:%s" % (tmp_path / "d_BEAM")]) == 0
    err = capfd.readouterr().err
    wide = [l for l in err.splitlines() if "[BEAM=1000] Overall density" in l][0].split()
    assert wide[6] == f[5] and wide[8] == f[7]
    assert (tmp_path / "d_1000").read_text() == (tmp_path / "depth").read_text() and (tmp_path / "d_0.25").exists()


def test_bin_shims_are_executable():
    for n in ("oracle", "depth"):
        p = os.path.join(ROOT, "bin", "lattice-" + n)
        assert os.access(p, os.X_OK) and "tools/lattice_%s.py" % n in open(p).read()
