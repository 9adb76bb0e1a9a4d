"""No GPU: the tree-statistics file format, the event construction and sum-tree-stats against the line-by-line restatement
(tests/tree_stats_restatement.py) and against bytes and events written out by hand.  Nothing reference-compiled pins this
feature (hmm-utils needs OpenFst, which the reference build here does not have), so the restatement itself is held to
hand-built answers first."""
import io
import os
import struct
import sys

import numpy as np
import pytest

import tree_stats_cases as C
import tree_stats_restatement as R
from conftest import ROOT, pkg

sys.path.insert(0, os.path.join(ROOT, "tools"))

TWO = [(((-1, 0), (1, 7)), dict(count=3.0, var_floor=float(np.float32(0.01)), stats=np.array([[1.5, -2.0], [0.25, 1e10]]))),
       (((-1, 1), (0, 0), (1, 7), (2, 12)), dict(count=1.0, var_floor=float(np.float32(0.01)), stats=np.array([[0.1, 3.0], [1 / 3, 9.0]])))]


def hand_bytes(binary):
    """The two-event file, token by token."""
    vf = float(np.float32(0.01))
    if binary:
        i32 = lambda v: b"\x04" + struct.pack("<i", v)
        dbl = lambda v: b"\x08" + struct.pack("<d", v)
        mat = lambda rows: b"DM " + i32(2) + i32(2) + b"".join(struct.pack("<d", v) for r in rows for v in r)
        return (b"BTS \xfc\x02\x00\x00\x00"
                b"EV \xfc\x02\x00\x00\x00" + i32(-1) + i32(0) + i32(1) + i32(7) + b"T" + b"GCL " + dbl(3.0) + dbl(vf)
                + mat([[1.5, -2.0], [0.25, 1e10]])
                + b"EV \xfc\x04\x00\x00\x00" + i32(-1) + i32(1) + i32(0) + i32(0) + i32(1) + i32(7) + i32(2) + i32(12) + b"T"
                + b"GCL " + dbl(1.0) + dbl(vf) + mat([[0.1, 3.0], [1 / 3, 9.0]]))
    return (b"BTS 2 EV 2 -1 0 1 7 \nT GCL 3 0.01  [\n  1.5 -2 \n  0.25 1e+10 ]\n"
            b"EV 4 -1 1 0 0 1 7 2 12 \nT GCL 1 0.01  [\n  0.1 3 \n  0.3333333 9 ]\n\n")


@pytest.mark.parametrize("binary", [True, False])
def test_two_event_file_bytes_and_round_trip(binary):
    kio = pkg("kaldi_io")
    f = io.BytesIO()
    kio.write_tree_stats(f, TWO, binary)
    assert f.getvalue() == hand_bytes(binary) == R.write_tree_stats(TWO, binary)
    got = kio.read_tree_stats(kio.Stream(io.BytesIO(f.getvalue())), binary)
    assert [e for e, _ in got] == [e for e, _ in TWO]
    for (_, g), (_, w) in zip(got, TWO):
        assert g["stats"].dtype == np.float64 and g["stats"].shape == (2, 2)
        if binary:
            assert g["count"] == w["count"] and g["var_floor"] == w["var_floor"] and C.same_bits(g["stats"], w["stats"])
        else:                                                   # seven digits
            assert g["count"] == w["count"] and abs(g["var_floor"] - 0.01) < 1e-9 and np.allclose(g["stats"], w["stats"], rtol=1e-6)
    # written again the text is the same text, the binary the same bytes
    f2 = io.BytesIO()
    kio.write_tree_stats(f2, got, binary)
    assert f2.getvalue() == f.getvalue()


def test_null_pointer_and_empty_file():
    kio = pkg("kaldi_io")
    for binary in (True, False):
        for stats in ([], [(((0, 3),), None)]):
            f = io.BytesIO()
            kio.write_tree_stats(f, stats, binary)
            assert f.getvalue() == R.write_tree_stats(stats, binary)
            assert kio.read_tree_stats(kio.Stream(io.BytesIO(f.getvalue())), binary) == stats
    assert R.write_tree_stats([], True) == b"BTS \xfc\x00\x00\x00\x00" and R.write_tree_stats([], False) == b"BTS 0 \n"


# ---------------------------------------------------------------- event construction
def hand_alignment(reordered):
    """phones 2 (2 + 1 frames), 1 (1 + 2 + 1), 3 (1 + 3)."""
    return C.alignment([2, 1, 3], [[2, 1], [1, 2, 1], [1, 3]], reordered)


def ev(pc, *pairs):
    return tuple(sorted(((-1, pc),) + pairs))


@pytest.mark.parametrize("reordered", [False, True])
def test_hand_built_events(reordered):
    tm, api = C.tables(), pkg("api")
    ptm = C.product_model(pkg("kaldi_io"))
    ali = hand_alignment(reordered)
    assert len(ali) == 11 and R.is_reordered(tm, ali) == reordered
    split = []
    assert R.split_to_phones(tm, ali, split) and [len(s) for s in split] == [3, 4, 4]
    # N = 3, P = 1: the utterance's edges are phone 0
    want = ([ev(0, (0, 0), (1, 2), (2, 1))] * 2 + [ev(1, (0, 0), (1, 2), (2, 1))]
            + [ev(0, (0, 2), (1, 1), (2, 3))] + [ev(1, (0, 2), (1, 1), (2, 3))] * 2 + [ev(2, (0, 2), (1, 1), (2, 3))]
            + [ev(0, (0, 1), (1, 3), (2, 0))] + [ev(1, (0, 1), (1, 3), (2, 0))] * 3)
    assert R.frame_events(tm, ali, 3, 1, [], None) == (True, want)
    assert api.tree_stats_frame_events(ptm, ali, 3, 1, [], None) == (True, want)
    # N = 1, P = 0
    want = [ev(0, (0, 2))] * 2 + [ev(1, (0, 2))] + [ev(0, (0, 1))] + [ev(1, (0, 1))] * 2 + [ev(2, (0, 1))] + [ev(0, (0, 3))] + [ev(1, (0, 3))] * 3
    assert R.frame_events(tm, ali, 1, 0, [], None) == (True, want)
    assert api.tree_stats_frame_events(ptm, ali, 1, 0, [], None) == (True, want)
    # phone 1 context-independent: only key P is kept for its frames
    want = ([ev(0, (0, 0), (1, 2), (2, 1))] * 2 + [ev(1, (0, 0), (1, 2), (2, 1))]
            + [ev(0, (1, 1))] + [ev(1, (1, 1))] * 2 + [ev(2, (1, 1))]
            + [ev(0, (0, 1), (1, 3), (2, 0))] + [ev(1, (0, 1), (1, 3), (2, 0))] * 3)
    assert R.frame_events(tm, ali, 3, 1, [1], None) == (True, want)
    assert api.tree_stats_frame_events(ptm, ali, 3, 1, [1], None) == (True, want)
    # phone map 1 -> 5, 2 -> 5, 3 -> 6; ci-phones are phones after mapping
    pm = [-1, 5, 5, 6]
    want = ([ev(0, (1, 5))] * 2 + [ev(1, (1, 5))] + [ev(0, (1, 5))] + [ev(1, (1, 5))] * 2 + [ev(2, (1, 5))]
            + [ev(0, (0, 5), (1, 6), (2, 0))] + [ev(1, (0, 5), (1, 6), (2, 0))] * 3)
    assert R.frame_events(tm, ali, 3, 1, [5], pm) == (True, want)
    assert api.tree_stats_frame_events(ptm, ali, 3, 1, [5], np.asarray(pm)) == (True, want)


def test_bad_alignments_and_reference_errors():
    tm, api = C.tables(), pkg("api")
    ptm = C.product_model(pkg("kaldi_io"))
    good = hand_alignment(False)
    bad = dict(cut_short=good[:-1], begins_inside_a_phone=good[2:], phone_changes_without_a_final=good[:2] + good[3:],
               reordered_cut_short=hand_alignment(True)[:-3])
    for name, ali in bad.items():
        assert R.frame_events(tm, ali, 3, 1, [], None) == (False, []), name
        assert api.tree_stats_frame_events(ptm, ali, 3, 1, [], None) == (False, []), name
    assert api.tree_stats_frame_events(ptm, [], 3, 1, [], None) == (True, []) == R.frame_events(tm, [], 3, 1, [], None)
    # the reference's errors and assertions, with its words
    with pytest.raises(R.KaldiErr, match="Out-of-range phone 3 bad --phone-map option?"):
        R.frame_events(tm, good, 3, 1, [], [-1, 5, 5])
    with pytest.raises(api.KhError, match=r"Out-of-range phone 3 bad --phone-map option\?"):
        api.tree_stats_frame_events(ptm, good, 3, 1, [], [-1, 5, 5])
    with pytest.raises(R.KaldiAssert, match="IsSortedAndUniq"):
        R.frame_events(tm, good, 3, 1, [2, 1], None)
    with pytest.raises(api.KhError, match=r"IsSortedAndUniq\(ci_phones\)"):
        api.tree_stats_frame_events(ptm, good, 3, 1, [2, 1], None)
    for N, P in ((3, 4), (3, -1), (1, 3)):
        with pytest.raises(R.KaldiAssert, match="cur_pos =="):
            R.frame_events(tm, good, N, P, [], None)
        with pytest.raises(api.KhError, match=r"cur_pos == static_cast<int>\(alignment.size\(\)\)"):
            api.tree_stats_frame_events(ptm, good, N, P, [], None)
    for text in ("1:0", "2:2", "1:x"):
        with pytest.raises(api.KhError, match="Invalid set of ci_phones: " + text):
            api.tree_stats_ci_phones(text)
    assert api.tree_stats_ci_phones("3:1") == [1, 3] and api.tree_stats_ci_phones("") == []
    with pytest.raises(api.KhError, match="transition-id 19"):
        api.tree_stats_frame_events(ptm, [1, 19], 3, 1, [], None)


@pytest.mark.parametrize("reordered", [False, True])
def test_frame_events_equal_the_restatement_on_random_alignments(reordered):
    tm, api = C.tables(), pkg("api")
    ptm = C.product_model(pkg("kaldi_io"))
    tables = api.tree_stats_tables(ptm)
    rng = np.random.default_rng(5 + reordered)
    n_bad = 0
    for trial in range(60):
        _, ali = C.random_alignment(rng, int(rng.integers(1, 9)), reordered)
        if trial % 4 == 3:                                      # damaged: a frame dropped somewhere
            k = int(rng.integers(0, len(ali)))
            ali = ali[:k] + ali[k + 1:]
        elif trial % 4 == 1:                                    # damaged: a forward transition dropped (the even ids)
            k = int(rng.choice([i for i, t in enumerate(ali) if t % 2 == 0]))
            ali = ali[:k] + ali[k + 1:]
        for N, P, ci, pm in ((3, 1, [], None), (3, 1, [1], None), (1, 0, [], None), (2, 0, [2, 4], None), (5, 2, [7], [-1, 7, 7, 3, 9]),
                             (2, 2, [], None), (0, 0, [], None), (-1, -1, [], None), (-1, 0, [], None), (-2, 1, [3], None)):
            try:
                want = R.frame_events(tm, ali, N, P, ci, pm)
            except R.KaldiAssert as e:
                with pytest.raises(api.KhError, match="KALDI_ASSERT"):
                    api.tree_stats_frame_events(ptm, ali, N, P, ci, pm, tables=tables)
                continue
            assert api.tree_stats_frame_events(ptm, ali, N, P, ci, pm, tables=tables) == want
            ok, table, code = api.tree_stats_frame_events(ptm, ali, N, P, ci, pm, tables=tables, codes=True)     # the same, as indices
            assert (ok, [table[k] for k in code]) == want and code.dtype == np.int32 and len(set(table)) <= len(table) <= max(len(ali), 1)
            n_bad += not want[0]
    assert n_bad > 10                                           # the damaged ones were met


def test_read_phone_map():
    kio = pkg("kaldi_io")
    text = "1 1\n2 1\n4\t2 \n"
    assert kio.read_phone_map(text.encode()).tolist() == [-1, 1, 1, -1, 2] == R.read_phone_map(text)
    for bad, words in (("1 1\n1 2\n", r"\(bad line 1\)"), ("0 1\n", r"\(bad line 0\)"), ("1 0\n", r"\(bad line 0\)"), ("1 2 3\n", r"\(bad line 0\)"),
                       ("1 1\n\n2 2\n", r"\(bad line 1\)"), ("", "Read empty phone map from map.txt"), ("1 x\n", "Error reading phone map from map.txt")):
        with pytest.raises(ValueError, match=words):
            kio.read_phone_map(bad.encode(), "map.txt")
        with pytest.raises(R.KaldiErr):
            R.read_phone_map(bad)


# ---------------------------------------------------------------- the restatement's sums, and sum-tree-stats
def test_restatement_sums_by_hand():
    x = np.array([[1.1, 3e17], [0.3, 0.3], [-1.1, -3e17]], np.float32)
    count, stats = R.add_stats(x, [0, 0, 0], 1)
    f = lambda v: float(np.float32(v))
    sq = lambda v: float(np.float32(np.float32(v) * np.float32(v)))
    assert count.tolist() == [3.0]
    assert stats[0, 0].tolist() == [(f(1.1) + f(0.3)) + f(-1.1), (f(3e17) + f(0.3)) + f(-3e17)]
    assert stats[0, 1].tolist() == [(sq(1.1) + sq(0.3)) + sq(-1.1), (sq(3e17) + sq(0.3)) + sq(-3e17)]
    assert stats[0, 0, 1] == 0.0 and sq(1.1) != f(1.1) * f(1.1)           # 0.3 is lost beside 3e17; the float product rounds


def test_order_cases_are_sensitive():
    for name, case in C.order_cases(np.random.default_rng(3)).items():
        assert C.sensitive(case) == (True, True, True), name


def job_files(rng):
    tm = C.tables()
    jobs = []
    for j in range(3):
        job = []
        for _ in range(3):
            _, ali = C.random_alignment(rng, 4, False)
            job.append((C.features(rng, len(ali), 3), ali))
        jobs.append(R.acc_tree_stats(tm, job, ci_phones=[1])[0])
    return jobs


def test_sum_tree_stats_merge_order_and_status(tmp_path, capfd):
    kio = pkg("kaldi_io")
    import sum_tree_stats as tool
    a, b, c = job_files(np.random.default_rng(11))
    events = lambda stats: set(e for e, _ in stats)
    common = sorted(events(a) & events(b))
    assert common and events(a) & events(b) & events(c) and events(a) ^ events(b)
    dict(b)[common[0]]["var_floor"] = 0.5                       # the first occurrence's floor is the one kept
    assert dict(R.sum_tree_stats([a, b])[0])[common[0]]["var_floor"] == float(np.float32(0.01))
    assert dict(R.sum_tree_stats([b, a])[0])[common[0]]["var_floor"] == 0.5
    want_abc, status = R.sum_tree_stats([a, b, c])
    want_cba, _ = R.sum_tree_stats([c, b, a])
    assert status == 0 and [e for e, _ in want_abc] == sorted(events(a) | events(b) | events(c))
    assert R.write_tree_stats(want_abc, True) != R.write_tree_stats(want_cba, True)    # (a + b) + c against (c + b) + a
    for name, stats in (("a", a), ("b", b), ("c", c)):
        with open(tmp_path / name, "wb") as f:
            f.write(b"\0B")
            kio.write_tree_stats(f, stats, True)
    assert tool.main([str(tmp_path / "abc"), str(tmp_path / "a"), str(tmp_path / "b"), str(tmp_path / "c")]) == 0
    assert tool.main(["--binary=false", str(tmp_path / "cba"), str(tmp_path / "c"), str(tmp_path / "b"), str(tmp_path / "a")]) == 0
    assert (tmp_path / "abc").read_bytes() == b"\0B" + R.write_tree_stats(want_abc, True)
    assert (tmp_path / "cba").read_bytes() == R.write_tree_stats(want_cba, False)
    err = capfd.readouterr().err
    assert err.count("LOG (sum-tree-stats:main()) Wrote summed accs ( %d individual stats)" % len(want_abc)) == 2
    # nothing summed: the file is written, the status is 1
    with open(tmp_path / "empty", "wb") as f:
        f.write(b"\0B")
        kio.write_tree_stats(f, [], True)
    assert R.sum_tree_stats([[], []]) == ([], 1)
    assert tool.main([str(tmp_path / "none"), str(tmp_path / "empty"), str(tmp_path / "empty")]) == 1
    assert (tmp_path / "none").read_bytes() == b"\0BBTS \xfc\x00\x00\x00\x00"
    assert "Wrote summed accs ( 0 individual stats)" in capfd.readouterr().err
    assert tool.main([str(tmp_path / "x")]) == 1 and "Usage:  sum-tree-stats [options] tree-accs-out" in capfd.readouterr().err
