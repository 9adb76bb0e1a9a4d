"""GPU box: kh_compact_lattice_oracle (csrc/kh_latoracle.hip) against the cell-by-cell restatement
(latoracle_restatement.py).  Everything is an integer and the tie rule is fixed, so every output - errors, the four counts,
the path's arcs, the final state, the frame sum - is compared exactly."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

import latoracle_cases
import latoracle_restatement as R
from test_lattice_oracle_wer import consistent_clat, restated_oracle, small_archive, write_archive

pytestmark = pytest.mark.gpu

WILD = (9,)


def with_frames(api, clat):
    csr = api.compact_lattice_to_prune_csr(clat)
    csr["arc_frames"], csr["final_frames"] = R.frames_of(clat, csr)
    return csr


def assert_point_equals(raw, i, p, r, what):
    """Lattice i, point p of compact_lattice_oracle_raw's answer against the restatement's r."""
    assert int(raw["errors"][i, p]) == r["errors"], what
    assert raw["counts"][i, p].tolist() == [r["correct"], r["sub"], r["ins"], r["del"]], what
    assert raw["paths"][i][p].tolist() == list(r["path_arcs"]), what
    assert int(raw["final_state"][i, p]) == r["final_state"], what
    assert int(raw["path_len"][i, p]) == (len(r["path_arcs"]) if r["errors"] >= 0 else -1), what
    if r["frame_sum"] is not None:
        assert int(raw["frame_sum"][i, p]) == r["frame_sum"], what


def test_hand_lattices(api):
    """Every hand lattice alone through the dict-level call, and all of them as one batch through the raw call."""
    cases = latoracle_cases.all_cases()
    for name, clat, ref, wild, want in cases:
        got = api.compact_lattice_oracle([clat], [ref], wild)[0][0]
        latoracle_cases.check_result(got, want, name)
        exp = restated_oracle([clat], [ref], wild)[0][0]
        assert got["errors"] == exp["errors"], name
        if exp["depth"] is not None:
            assert (got["depth"], got["num_frames"]) == (exp["depth"], exp["num_frames"]), name
    csrs = [with_frames(api, c[1]) for c in cases]
    raw = api.compact_lattice_oracle_raw(csrs, [L["start"] for L in csrs], [c[2] for c in cases], WILD)
    for i, (name, clat, ref, wild, want) in enumerate(cases):
        r = R.oracle(csrs[i], ref, WILD, arc_frames=csrs[i]["arc_frames"], final_frames=csrs[i]["final_frames"])
        assert_point_equals(raw, i, 0, r, name)


@pytest.fixture(scope="module")
def fuzz(api):
    """Random lattices of at most 40 states over 3 words, epsilon and the wildcard, against references of 0, 1, 63, 64, 65
    and 130 words (wildcards among them: the lengths are those after their removal): the chunk boundaries of the lane
    mapping and the carries of the diagonal and of the prefix-min.  Every fifth has its start state behind state 0."""
    clats, refs = [], []
    for seed in range(4):
        for k, n_ref in enumerate((0, 1, 63, 64, 65, 130)):
            rng = np.random.default_rng(5200 + 10 * seed + k)
            n = int(rng.integers(2, 41))
            start = int(rng.integers(0, n // 2 + 1)) if len(clats) % 5 == 4 else 0
            clats.append(R.random_word_clat(rng, n, start=start, last_final=bool(rng.random() < 0.9)))
            ref = [int(x) for x in rng.choice([1, 2, 3], size=n_ref)]
            for pos in sorted(rng.integers(0, n_ref + 1, size=int(rng.integers(0, 4))).tolist(), reverse=True):
                ref.insert(pos, 9)
            refs.append(ref)
    csrs = [with_frames(api, c) for c in clats]
    wants = [R.oracle(L, ref, WILD, arc_frames=L["arc_frames"], final_frames=L["final_frames"]) for L, ref in zip(csrs, refs)]
    return clats, csrs, refs, wants


def test_fuzz_against_the_restatement(api, fuzz):
    clats, csrs, refs, wants = fuzz
    assert sorted(set(w["R"] for w in wants)) == [0, 1, 63, 64, 65, 130]
    raw = api.compact_lattice_oracle_raw(csrs, [L["start"] for L in csrs], refs, WILD)
    for i, w in enumerate(wants):
        assert_point_equals(raw, i, 0, w, i)
    assert api.compact_lattice_oracle_last_timings()["launches"] == 1


def test_bounded_workspace_gives_the_same(api, fuzz):
    """Lattices of very different sizes (a chain of 600 states against 130 words among them) under a workspace limit that
    admits only the largest alone: several launches, the same answers."""
    clats, csrs, refs, wants = fuzz
    big = latoracle_cases.chain([1 + (i % 3) for i in range(599)])
    csrs = csrs[:12] + [with_frames(api, big)]
    refs = refs[:12] + [[1 + (i % 2) for i in range(130)]]
    starts = [L["start"] for L in csrs]
    one = api.compact_lattice_oracle_raw(csrs, starts, refs, WILD)
    assert api.compact_lattice_oracle_last_timings()["launches"] == 1
    for i, w in enumerate(wants[:12]):
        assert_point_equals(one, i, 0, w, i)
    assert_point_equals(one, 12, 0, R.oracle(csrs[12], refs[12], WILD, arc_frames=csrs[12]["arc_frames"],
                                             final_frames=csrs[12]["final_frames"]), "big")
    many = api.compact_lattice_oracle_raw(csrs, starts, refs, WILD, workspace_limit=600 * 131 * 4)
    assert api.compact_lattice_oracle_last_timings()["launches"] > 1
    for k in ("errors", "counts", "path_len", "final_state", "frame_sum"):
        assert np.array_equal(one[k], many[k]), k
    assert all(np.array_equal(a[0], b[0]) for a, b in zip(one["paths"], many["paths"]))


@pytest.mark.parametrize("n_points", [1, 64, 65])
def test_masks_from_the_pruning_call(api, n_points):
    """The masks of compact_lattice_prune_raw at ascending beams (W = 1 and 2 words): every point equals the restatement
    on the same masks, errors do not increase with the beam, and the widest beam is the unmasked call."""
    rng = np.random.default_rng(77)
    clats = [consistent_clat(rng, int(rng.integers(3, 15))) for _ in range(4)] + [latoracle_cases.no_final()[1]]
    refs = [[int(x) for x in rng.integers(1, 4, size=int(rng.integers(0, 6)))] for _ in clats]
    csrs = [with_frames(api, c) for c in clats]
    starts = [L["start"] for L in csrs]
    beams = np.linspace(0.25, 12.0, n_points).astype(np.float32) if n_points > 1 else np.array([3.0], np.float32)
    beams[-1] = 1000.0
    masks = api.compact_lattice_prune_raw(csrs, starts, [api.score_point(acoustic_scale=0.5)] * n_points, beams)
    raw = api.compact_lattice_oracle_raw(csrs, starts, refs, WILD, masks)
    plain = api.compact_lattice_oracle_raw(csrs, starts, refs, WILD)
    # the pruning call's own words went to the device; the bool arrays alone, packed again, say the same
    repacked = api.compact_lattice_oracle_raw(csrs, starts, refs, WILD, {k: masks[k] for k in ("arc_keep", "state_keep", "final_keep")})
    for k in ("errors", "counts", "path_len", "final_state", "frame_sum"):
        assert np.array_equal(raw[k], repacked[k]), k
    so, ao = masks["state_offsets"], masks["arc_offsets"]
    for i, L in enumerate(csrs):
        for p in range(n_points):
            r = R.oracle(L, refs[i], WILD, arc_keep=masks["arc_keep"][ao[i]:ao[i + 1], p], state_keep=masks["state_keep"][so[i]:so[i + 1], p],
                         final_keep=masks["final_keep"][so[i]:so[i + 1], p], arc_frames=L["arc_frames"], final_frames=L["final_frames"])
            assert_point_equals(raw, i, p, r, (i, p))
        e = raw["errors"][i]
        none = e < 0                       # what a wider beam keeps includes what a narrower one keeps: no path is lost again
        assert not np.any(np.diff(none.astype(np.int8)) > 0), (i, e)
        assert np.all(np.diff(e[~none]) <= 0), (i, e)
        for k in ("errors", "counts", "final_state") + (("frame_sum",) if e[-1] >= 0 else ()):     # (nothing survives: no frames)
            assert np.array_equal(raw[k][i, -1], plain[k][i, 0]), (i, k)
        assert np.array_equal(raw["paths"][i][-1], plain["paths"][i][0])
    assert (raw["errors"][-1] == -1).all()
    # the dict-level call chains the two and adds depth and words
    res = api.compact_lattice_oracle(clats, refs, WILD, points=[api.score_point(acoustic_scale=0.5)], beams=beams[-2:])
    exp = restated_oracle(clats, refs, WILD, points=[api.score_point(acoustic_scale=0.5)], beams=beams[-2:])
    for row, erow in zip(res, exp):
        for g, e in zip(row, erow):
            assert g["errors"] == e["errors"] and (g["depth"], g["num_frames"]) == (e["depth"], e["num_frames"])
            if e["errors"] >= 0:
                assert [g[k] for k in ("correct", "sub", "ins", "del")] == [e[k] for k in ("correct", "sub", "ins", "del")]
                assert g["words"].tolist() == e["words"].tolist()


def test_refusals(api):
    """Every KH_EINVAL case names what it refuses; none reaches the device."""
    capi = importlib.import_module("old-kaldi-git_amd.capi")
    lib = capi.load()
    ip, lp = capi.c_int32_p, capi.c_int64_p
    ptr = lambda a, t: a.ctypes.data_as(t)

    def call(nxt=(1, 2), start=0, n_points=1, roff=(0, 1), room=(0, 2), masks=False):
        soff, aoff = np.array([0, 3], np.int32), np.array([0, 1, 2, 2], np.int64)
        lab, ns = np.array([1, 2], np.int32), np.asarray(nxt, np.int32)
        fin, st = np.array([0, 0, 1], np.int32), np.array([start], np.int32)
        ro, rw = np.asarray(roff, np.int64), np.array([1, 2], np.int32)
        K = max(n_points, 1)
        po = np.asarray(room, np.int64)
        out = [np.zeros(4 * K + 8, np.int32) for _ in range(5)]
        fs = np.zeros(K, np.int64)
        m = [np.full((3, 1), 1, np.uint64) for _ in range(3)] if masks else None
        up = capi.c_uint64_p
        return lib.kh_compact_lattice_oracle(1, ptr(soff, ip), ptr(st, ip), ptr(aoff, lp), ptr(lab, ip), ptr(ns, ip), ptr(fin, ip),
                                             ptr(ro, lp), ptr(rw, ip), 0, None, n_points, ptr(m[0], up) if m else None,
                                             ptr(m[1], up) if m else None, ptr(m[2], up) if m else None, None, None,
                                             ptr(out[0], ip), ptr(out[1], ip), ptr(out[2], ip), ptr(out[3], ip), ptr(po, lp), ptr(out[4], ip),
                                             ptr(fs, lp))
    err = lambda: lib.kh_last_error().decode()
    assert call() == 0
    assert call(nxt=(1, 1)) != 0 and "lattice 0: arc 1 (state 1 -> 1 of 3): input lattice must be topologically sorted" in err()
    assert call(nxt=(1, 3)) != 0 and "arc 1 (state 1 -> 3 of 3)" in err()
    assert call(start=3) != 0 and "lattice 0: start state 3 of 3 states" in err()
    assert call(start=-1) != 0 and "start state -1" in err()
    assert call(n_points=0) != 0 and "n_points = 0" in err()
    assert call(n_points=2) != 0 and "n_points = 2 without keep masks" in err()
    assert call(roff=(0, -1)) != 0 and "lattice 0: ref_offsets 0, -1" in err()
    assert call(roff=(0, 1 << 24)) != 0 and "lattice 0: a reference of 16777216 words: at most 16777215 are taken" in err()
    assert call(room=(0, 1)) != 0 and "lattice 0, point 0: path_offsets leaves room for 1 arcs, a path may have 2" in err()
    assert call(masks=True) == 0
    with pytest.raises(capi.KhError, match="topologically sorted"):
        bad = api.compact_lattice_to_prune_csr(latoracle_cases.chain([1, 2]))
        bad["arc_nextstate"] = np.array([1, 1], np.int32)
        api.compact_lattice_oracle_raw([bad], [0], [[1]], ())


def test_tools_end_to_end(api, tmp_path, monkeypatch, capfd):
    """The plain command lines against the restatement's numbers; the --beams sweep's files against the per-beam runs of
    bin/lattice-prune | bin/lattice-oracle, and of bin/lattice-depth on the same pruned archive, as processes, byte for byte."""
    clats, refs = small_archive(6, seed=21)
    clats.append(("nofinal", latoracle_cases.no_final()[1]))
    refs.append(("nofinal", [1]))
    monkeypatch.chdir(tmp_path)
    rs, ref_rs = write_archive(tmp_path, clats, refs[1:])            # utt0 has no reference
    oracle_tool, depth_tool = importlib.import_module("tools.lattice_oracle"), importlib.import_module("tools.lattice_depth")
    assert oracle_tool.main(["--wildcard-symbols=4", rs, ref_rs, "ark,t:plain.tra", "ark,t:plain.edits"]) == 0
    err = capfd.readouterr().err
    want = [restated_oracle([c], [r], (4,))[0][0] for (_, c), (_, r) in list(zip(clats, refs))[1:-1]]
    tot = lambda k: sum(r[k] for r in want)
    assert ("Overall %%WER %s [ %d / %d, %d insertions, %d deletions, %d substitutions ]"
            % (oracle_tool.cxx_ratio(100.0 * tot("errors"), tot("R")), tot("errors"), tot("R"), tot("ins"), tot("del"), tot("sub"))) in err
    assert "Scored 6 lattices, 2 not present in ref." in err
    assert open("plain.tra").read().splitlines() == ["%s %s" % (k, "".join("%d " % w for w in r["words"])) for (k, _), r in zip(clats[1:-1], want)]
    assert open("plain.edits").read().splitlines() == ["%s %d " % (k, r["errors"]) for (k, _), r in zip(clats[1:-1], want)]
    beams = ("0.5", "3")
    assert oracle_tool.main(["--wildcard-symbols=4", "--acoustic-scale=0.5", "--beams=" + ",".join(beams), rs, ref_rs,
                             "ark,t:sweep_BEAM.tra", "ark,t:sweep_BEAM.edits"]) == 0
    sweep_err = capfd.readouterr().err
    assert depth_tool.main(["--acoustic-scale=0.5", "--beams=" + ",".join(beams), rs, "ark,t:sweep_BEAM.depth"]) == 0
    depth_err = capfd.readouterr().err
    env = dict(os.environ, PATH=os.path.join(ROOT, "bin") + os.pathsep + os.environ["PATH"], PYTHON=sys.executable)
    for b in beams:
        cmd = ("lattice-prune --acoustic-scale=0.5 --beam=%s %s ark:- | tee pruned_%s.lats | "
               "lattice-oracle --wildcard-symbols=4 ark:- %s ark,t:pipe_%s.tra ark,t:pipe_%s.edits && "
               "lattice-depth ark:- ark,t:pipe_%s.depth < pruned_%s.lats" % (b, rs, b, ref_rs, b, b, b, b))
        r = subprocess.run(["sh", "-c", cmd], env=env, stderr=subprocess.PIPE, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        for ext in ("tra", "edits", "depth"):
            got, exp = open("sweep_%s.%s" % (b, ext), "rb").read(), open("pipe_%s.%s" % (b, ext), "rb").read()
            assert len(exp) > 0 and got == exp, (b, ext)
        piped = [l.split(") ", 1)[1] for l in r.stderr.decode().splitlines() if "Overall %WER" in l or "Overall density" in l]
        mine = [l.split(") ", 1)[1].replace("[BEAM=%s] " % b, "") for l in (sweep_err + depth_err).splitlines()
                if "[BEAM=%s] Overall" % b in l]
        assert len(piped) == 2 and piped == mine, (piped, mine)
