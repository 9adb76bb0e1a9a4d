"""GPU: acc-tree-stats end to end on files (tools/acc_tree_stats.py), in process.  The tiny model of tests/tree_stats_cases.py
(followed in final.mdl by bytes nobody may read), D = 7, seven utterances:
  a  four phones, done            b  0 frames with an empty alignment, done        c  five phones, done
  d  its alignment one frame short: a failure "for other reasons"                  e  a bad alignment (it ends before its last
  phone's final transition): warned about, contributes nothing, still counted done f  no alignment: counted
  g  three phones, done
The written file equals the restatement's (tests/tree_stats_restatement.py: acc_tree_stats, then write_tree_stats) BYTE FOR
BYTE under the default options, --ci-phones, --phone-map, --context-width=1 --central-position=0, --var-floor, --binary=false,
reordered alignments, and whatever --batch-frames; two job files through sum-tree-stats equal the restatement's merge.
Fails without tools/acc_tree_stats.py."""
import importlib
import os
import re
import sys

import numpy as np
import pytest

import tree_stats_cases as C
import tree_stats_restatement as R
from conftest import ROOT, pkg

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(ROOT, "tools"))
DIM = 7
PHONE_MAP = "1 1\n2 2\n3 2\n4 3\n"


def tool(name):
    return importlib.import_module(name.replace("-", "_"))


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    cli, kio = pkg("kaldi_cli"), pkg("kaldi_io")
    d = tmp_path_factory.mktemp("acctree")
    (d / "final.mdl").write_bytes(C.model_bytes(kio))
    (d / "map.txt").write_text(PHONE_MAP)
    rng = np.random.default_rng(21)
    utts = {}
    for key, n_phones in (("a", 4), ("b", 0), ("c", 5), ("d", 3), ("e", 4), ("f", 2), ("g", 3)):
        phones = [int(p) for p in rng.integers(1, 5, n_phones)]
        durations = [[int(x) for x in rng.integers(1, 5, 3 if p == 1 else 2)] for p in phones]
        ali = {r: C.alignment(phones, durations, r) for r in (False, True)}
        if key == "e":                                          # the last phone stays in the state before its last: no final transition
            n_last = durations[-1][-1]
            for r in ali:
                before = C.alignment([phones[-1]], [durations[-1][:-1]], r)      # the phone without its last state
                ali[r][-n_last:] = [before[-durations[-1][-2]]] * n_last             # the first transition-id of the state before
                assert not C.tables().is_final(ali[r][-1])
        utts[key] = (C.features(rng, len(ali[False]), DIM), ali)
    fw = {name: cli.TableWriter("ark:" + str(d / name), "matrix") for name in ("feats.ark", "feats.1.ark", "feats.2.ark")}
    aw = {r: cli.TableWriter("ark:" + str(d / ("ali_r.ark" if r else "ali.ark")), "int32_vector") for r in (False, True)}
    for key, (mat, ali) in utts.items():
        fw["feats.ark"].write(key, mat)
        fw["feats.1.ark" if key in "abc" else "feats.2.ark"].write(key, mat)
        for r in (False, True):
            if key != "f":
                aw[r].write(key, ali[r][:-1] if key == "d" else ali[r])
    ow = cli.TableWriter("ark:" + str(d / "other.ark"), "int32_vector")
    ow.write("nobody", [1, 2])
    for w in list(fw.values()) + list(aw.values()) + [ow]:
        w.close()
    return dict(dir=d, utts=utts)


def job(files, keys="abcdefg", reordered=False):
    out = []
    for k in keys:
        mat, ali = files["utts"][k]
        out.append((mat, None if k == "f" else (ali[reordered][:-1] if k == "d" else ali[reordered])))
    return out


def restated(files, binary=True, keys="abcdefg", reordered=False, **kw):
    stats, done, no_ali, other, bad = R.acc_tree_stats(C.tables(), job(files, keys, reordered), **kw)
    return (b"\0B" if binary else b"") + R.write_tree_stats(stats, binary), stats, (done, no_ali, other, bad)


CASES = dict(
    default=([], {}),
    ci_phones=(["--ci-phones=1:3"], dict(ci_phones=[1, 3])),
    phone_map=(["--phone-map=map.txt", "--ci-phones=1"], dict(ci_phones=[1], phone_map=R.read_phone_map(PHONE_MAP))),
    monophone=(["--context-width=1", "--central-position=0"], dict(N=1, P=0)),
    var_floor=(["--var-floor=0.05", "--context-width=2", "--central-position=0"], dict(var_floor=0.05, N=2, P=0)),
    text=(["--binary=false", "--ci-phones=1"], dict(ci_phones=[1])),
    reordered=(["--ci-phones=1"], dict(ci_phones=[1])),
)


@pytest.mark.parametrize("name", sorted(CASES))
def test_file_is_the_restatement_byte_for_byte(files, name, monkeypatch, capfd):
    monkeypatch.chdir(files["dir"])
    opts, kw = CASES[name]
    ali = "ark:ali_r.ark" if name == "reordered" else "ark:ali.ark"
    want, stats, counts = restated(files, binary=name != "text", reordered=name == "reordered", **kw)
    assert counts == (5, 1, 1, 1) and len(stats) > 5
    assert tool("acc-tree-stats").main(opts + ["final.mdl", "ark:feats.ark", ali, name + ".treeacc"]) == 0
    err = capfd.readouterr().err
    assert (files["dir"] / (name + ".treeacc")).read_bytes() == want
    assert err.count("WARNING (acc-tree-stats:AccumulateTreeStats()) AccumulateTreeStats: alignment appears to be bad, not using it") == 1
    n_d = files["utts"]["d"][0].shape[0]
    assert err.count("WARNING (acc-tree-stats:main()) Alignments has wrong size %d vs. %d" % (n_d - 1, n_d)) == 1
    assert "LOG (acc-tree-stats:main()) Accumulated stats for 5 files, 1 failed due to no alignment, 1 failed for other reasons." in err
    assert "LOG (acc-tree-stats:main()) Number of separate stats (context-dependent states) is %d" % len(stats) in err
    # one utterance per library pass: the same bytes
    assert tool("acc-tree-stats").main(opts + ["--verbose=1", "--batch-frames=1", "final.mdl", "ark:feats.ark", ali, name + ".b.treeacc"]) == 0
    err = capfd.readouterr().err
    assert [int(x) for x in re.findall(r"batch of (\d+) rows in 1 utterances", err)] == [files["utts"][k][0].shape[0] for k in "acg"]
    assert (files["dir"] / (name + ".b.treeacc")).read_bytes() == want


def test_nothing_done_usage_and_job_refusal(files, monkeypatch, capfd):
    monkeypatch.chdir(files["dir"])
    t = tool("acc-tree-stats")
    assert t.main(["final.mdl", "ark:feats.ark", "ark:other.ark", "empty.treeacc"]) == 1
    err = capfd.readouterr().err
    assert "Accumulated stats for 0 files, 7 failed due to no alignment, 0 failed for other reasons." in err
    assert "Number of separate stats (context-dependent states) is 0" in err and "WARNING" not in err
    assert (files["dir"] / "empty.treeacc").read_bytes() == b"\0B" + R.write_tree_stats([], True)
    assert t.main(["final.mdl", "ark:feats.ark"]) == 1
    err = capfd.readouterr().err
    assert "Usage:  acc-tree-stats [options] model-in features-rspecifier alignments-rspecifier [tree-accs-out]" in err
    for opt in ("--binary", "--var-floor", "--ci-phones", "--context-width", "--central-position", "--phone-map", "--batch-frames", "--gpu"):
        assert opt in err
    for args in (["final.mdl", "ark:feats.JOB.ark", "ark:ali.ark", "all.treeacc"], ["final.mdl", "ark:feats.JOB.ark", "ark:ali.ark"]):
        assert t.main(["--world=2", "--rank=1"] + args) == 255
        assert "ERROR (acc-tree-stats) --world=2: the statistics file needs JOB in its name" in capfd.readouterr().err
    assert not (files["dir"] / "all.treeacc").exists()
    assert t.main(["--ci-phones=0:1", "final.mdl", "ark:feats.ark", "ark:ali.ark", "x.treeacc"]) == 255
    assert "ERROR (acc-tree-stats) Invalid set of ci_phones: 0:1" in capfd.readouterr().err
    assert t.main(["--phone-map=nowhere.txt", "final.mdl", "ark:feats.ark", "ark:ali.ark", "x.treeacc"]) == 255
    assert "ERROR (acc-tree-stats) Error reading phone map from nowhere.txt" in capfd.readouterr().err


def test_two_jobs_through_sum_tree_stats(files, monkeypatch, capfd):
    monkeypatch.chdir(files["dir"])
    for rank in (0, 1):
        assert tool("acc-tree-stats").main(["--world=2", "--rank=%d" % rank, "--ci-phones=1", "final.mdl", "ark:feats.JOB.ark", "ark:ali.ark",
                                            "JOB.treeacc"]) == 0
    one, s1, c1 = restated(files, keys="abc", ci_phones=[1])
    two, s2, c2 = restated(files, keys="defg", ci_phones=[1])
    assert (c1, c2) == ((3, 0, 0, 0), (2, 1, 1, 1))
    assert (files["dir"] / "1.treeacc").read_bytes() == one and (files["dir"] / "2.treeacc").read_bytes() == two
    assert tool("sum-tree-stats").main(["treeacc", "1.treeacc", "2.treeacc"]) == 0
    merged, status = R.sum_tree_stats([s1, s2])
    assert status == 0 and (files["dir"] / "treeacc").read_bytes() == b"\0B" + R.write_tree_stats(merged, True)
    # the sum of the jobs is not the whole job's file in general (other order of the adds), but it holds the same events and counts
    whole = restated(files, ci_phones=[1])[1]
    assert [e for e, _ in merged] == [e for e, _ in whole] and [g["count"] for _, g in merged] == [g["count"] for _, g in whole]
    capfd.readouterr()
