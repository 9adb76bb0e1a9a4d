"""GPU box: kh_rescore_compact_lattice (csrc/kh_latrescore.hip) against the line-by-line restatement
(tests/rescore_restatement.py), which is fed the device's own log-likelihood matrix copied to the host - so every arc and
final cost is held to exact equality - and, end to end through the GMM scorer, against the CPU oracle's scores within the
bound rescore_cases.py derives."""
import numpy as np
import pytest

import gmm_cases as G
import latalign_cases as A
import rescore_cases as C
import rescore_restatement as R

pytestmark = pytest.mark.gpu
F = np.float32


def device_loglikes(rows, cols=C.N_PDFS, seed=0):
    import torch
    ll = (np.random.default_rng(seed).standard_normal((rows, cols)) * 3 - 4).astype(F)
    return torch.from_numpy(ll).cuda(), ll


def layout(clats, extra):
    """Row offsets that give lattice i utt_len + extra[i] rows."""
    n = [max(C.utt_len_of(c) + e, 0) if int(c["n_states"]) > 0 else 2 for c, e in zip(clats, extra)]
    return np.concatenate([[0], np.cumsum(n)]).astype(np.int32)


def check_against_restatement(api, clats, rows, ll_dev, ll_host, t2p):
    got = api.compact_lattice_rescore(clats, ll_dev, rows, t2p)
    for i, (c, r) in enumerate(zip(clats, got)):
        status, want = R.rescore(c, ll_host[rows[i]:rows[i + 1]], t2p)
        if status == "cyclic":
            assert r["status"] == api.RESCORE_CYCLIC and r["clat"] is None, i
            continue
        assert r["status"] == status, (i, r["status"], status)
        if status != R.OK:
            assert r["clat"] is None, i
            continue
        R.same_clat(r["clat"], want, i)
        assert r["utt_len"] == R.compact_lattice_state_times(want)[0], i
    return got


def item_counts(clats):
    lens = [len(x) for c in clats for x in list(c["arc_string"]) + list(c["final_string"])]
    return sum(1 for n in lens if 1 <= n <= C.SHORT_LEN), sum(1 for n in lens if n > C.SHORT_LEN)


def test_every_string_length_both_mappings_and_final_strings(api):
    """Lengths 0, 1, 2, 8 | 9, 63, 64, 65, 130 on arcs (the cut-over between the thread and the wave mapping lies between 8
    and 9), a final weight with a short and with a 70-id string, Zero finals, an arc that ends at the last frame (final_len
    0), two transition-ids sharing a pdf, and row ranges that start anywhere and are longer than utt_len."""
    clats = [C.lengths_clat(5, 3), C.lengths_clat(8, 0), C.long_final_clat()]
    assert max(len(x) for x in clats[0]["arc_string"]) == 130 and len(clats[1]["final_string"][-1]) == 0
    t2p = C.tid2pdf()
    assert t2p[5] == t2p[6]
    rows = layout(clats, [0, 2, 1])
    ll_dev, ll_host = device_loglikes(int(rows[-1]) + 3)
    got = check_against_restatement(api, clats, rows, ll_dev, ll_host, t2p)
    assert all(r["status"] == api.RESCORE_OK for r in got)
    t = api.compact_lattice_rescore_last_timings()
    assert (t["thread_items"], t["wave_items"]) == item_counts(clats) and t["wave_items"] >= 10 and t["thread_items"] >= 10
    assert t["launches"] == 2
    # the empty strings kept their bits, the others moved
    c, out = clats[0], got[0]["clat"]
    for j in range(len(c["arc_src"])):
        assert (out["arc_a"][j] == c["arc_a"][j]) == (len(c["arc_string"][j]) == 0), j
    assert np.all(np.isinf(out["final_a"][:-1])) and np.isfinite(out["final_a"][-1])


def test_a_batch_with_every_status_leaves_the_bad_ones_untouched(api):
    t2p = C.tid2pdf()
    clats = [C.plain_clat(7), C.empty_clat(), C.inconsistent_clat(), C.plain_clat(8, 5, 2), C.plain_clat(9), C.bad_tid_clat(0),
             C.bad_tid_clat(C.NUM_TIDS + 1), C.unreachable_clat(), C.plain_clat(10, 3, 9)]
    rows = np.concatenate([[0], np.cumsum([12, 2, 9, 10 + 3, 12 - 1, 9, 9, 9, 27])]).astype(np.int32)
    ll_dev, ll_host = device_loglikes(int(rows[-1]))
    got = check_against_restatement(api, clats, rows, ll_dev, ll_host, t2p)
    S = api
    assert [r["status"] for r in got] == [S.RESCORE_OK, S.RESCORE_EMPTY, S.RESCORE_INCONSISTENT_TIMES, S.RESCORE_OK, S.RESCORE_FEATURES_TOO_SHORT,
                                          S.RESCORE_BAD_TID, S.RESCORE_BAD_TID, S.RESCORE_INCONSISTENT_TIMES, S.RESCORE_OK]
    assert got[4]["utt_len"] == 12 and got[3]["utt_len"] == 10
    # the raw call: the arrays of the lattices that were not rescored come back bit for bit, the others changed
    csrs = [api.compact_lattice_align_csr(c) for c in clats]
    status, utt_len, arcs, finals = api.compact_lattice_rescore_raw(csrs, ll_dev, rows, t2p)
    for i, L in enumerate(csrs):
        same = arcs[i].tobytes() == np.asarray(L["arc_acoustic"], F).tobytes() and finals[i].tobytes() == np.asarray(L["final_acoustic"], F).tobytes()
        assert same == (status[i] != api.RESCORE_OK), i
    # FEATURES_TOO_SHORT exactly at rows == utt_len - 1; OK at utt_len and beyond
    c = C.plain_clat(9)
    for n_rows, want in ((11, S.RESCORE_FEATURES_TOO_SHORT), (12, S.RESCORE_OK), (15, S.RESCORE_OK)):
        r, = api.compact_lattice_rescore([c], ll_dev, [5, 5 + n_rows], t2p)
        assert r["status"] == want, n_rows
    a = api.compact_lattice_rescore([c], ll_dev, [5, 17], t2p)[0]["clat"]["arc_a"]
    b = api.compact_lattice_rescore([c], ll_dev, [5, 20], t2p)[0]["clat"]["arc_a"]
    assert a.tobytes() == b.tobytes()
    assert C.bad_tid_clat(C.NUM_TIDS)["arc_string"][1][1] == C.NUM_TIDS
    assert api.compact_lattice_rescore([C.bad_tid_clat(C.NUM_TIDS)], ll_dev, [0, 9], t2p)[0]["status"] == S.RESCORE_OK


def test_negative_zero_with_an_empty_string_keeps_its_sign(api):
    c = C.negative_zero_clat()
    ll_dev, ll_host = device_loglikes(6)
    r, = check_against_restatement(api, [c], np.asarray([1, 5], np.int32), ll_dev, ll_host, C.tid2pdf())
    out = r["clat"]
    assert out["arc_a"][0] == 0 and np.signbit(out["arc_a"][0]) and out["final_a"][2] == 0 and np.signbit(out["final_a"][2])
    assert out["arc_a"][1] != 0


def test_unsorted_input_comes_back_in_the_top_sorted_numbering(api):
    import latmbr_cases as M
    clats = [C.unsorted_clat(), M.unsorted()]
    rows = layout(clats, [0, 1])
    ll_dev, ll_host = device_loglikes(int(rows[-1]))
    got = check_against_restatement(api, clats, rows, ll_dev, ll_host, C.tid2pdf())
    out = got[0]["clat"]
    assert out["start"] == 0 and out["arc_src"].tolist() == [0, 0, 1, 2] and out["arc_dst"].tolist() == [2, 1, 3, 3]
    assert out["arc_label"].tolist() == [1, 2, 4, 3]
    cyc = A.clat(3, [(0, 1, 1, 0.0, 0.0, [1]), (1, 2, 2, 0.0, 0.0, [2]), (2, 1, 3, 0.0, 0.0, [3])], {2: (0.0, 0.0, [])})
    ll_dev, _ = device_loglikes(15)
    r = api.compact_lattice_rescore([cyc, C.plain_clat(7)], ll_dev, [0, 3, 15], C.tid2pdf())
    assert r[0]["status"] == api.RESCORE_CYCLIC and r[1]["status"] == api.RESCORE_OK


def test_generated_batch(api):
    clats = C.generated_batch()
    assert len(clats) == 50
    rows = layout(clats, [i % 3 for i in range(len(clats))])
    ll_dev, ll_host = device_loglikes(int(rows[-1]), seed=3)
    got = check_against_restatement(api, clats, rows, ll_dev, ll_host, C.tid2pdf())
    assert all(r["status"] == api.RESCORE_OK for r in got)
    t = api.compact_lattice_rescore_last_timings()
    assert (t["thread_items"], t["wave_items"]) == item_counts(clats) and t["wave_items"] > 0 and t["thread_items"] > 0
    print("timings", t)


def test_arguments_are_checked(api):
    import torch
    capi = api.capi
    c = C.plain_clat(7)
    ll_dev, _ = device_loglikes(20)
    t2p = C.tid2pdf()
    bad = t2p.copy()
    bad[17] = C.N_PDFS                         # a pdf the matrix does not have
    with pytest.raises(capi.KhError, match="tid2pdf"):
        api.compact_lattice_rescore([c], ll_dev, [0, 12], bad)
    with pytest.raises(capi.KhError):          # rows past the matrix
        api.compact_lattice_rescore([c], ll_dev, [10, 22], t2p)
    L = api.compact_lattice_align_csr(c)
    L["arc_nextstate"] = L["arc_nextstate"][::-1].copy()
    with pytest.raises(capi.KhError, match="topologically sorted"):
        api.compact_lattice_rescore_raw([L], ll_dev, [0, 12], t2p)
    with pytest.raises(capi.KhError):
        api.compact_lattice_rescore([c], ll_dev.double(), [0, 12], t2p)
    with pytest.raises(capi.KhError):
        api.compact_lattice_rescore([c], torch.zeros(20, C.N_PDFS), [0, 12], t2p)


@pytest.fixture(scope="module")
def gmm_case(api, oracle):
    """One GMM (16 pdfs of 1 .. 128 Gaussians, 13 dimensions), frames for five lattices, the device model and the oracle's
    scores, computed once."""
    import torch
    off, g, mi, iv, dim, rng = G.build("edge_small_d13", oracle)
    n_pdfs = len(off) - 1
    clats = [C.lengths_clat(5, 3), C.long_final_clat(), C.plain_clat(7), A.generate(11007, 6), C.negative_zero_clat()]
    rows = layout(clats, [0, 3, 1, 0, 2])
    feats = G.frames(rng, int(rows[-1]), dim)
    am = api.AmDiagGmm(g, mi, iv, off)
    scores = oracle.am_gmm_loglikes(feats, g, mi, iv, off, prune=-1.0)
    return dict(am=am, feats=torch.from_numpy(feats).cuda(), rows=rows, clats=clats, t2p=C.tid2pdf(n_pdfs), scores=scores, sizes=np.diff(off))


def test_end_to_end_against_the_oracles_scores_within_the_derived_bound(api, gmm_case):
    g = gmm_case
    got = api.gmm_rescore_compact_lattices(g["am"], g["feats"], g["rows"], g["clats"], g["t2p"])
    worst, n_items = 0.0, 0
    for i, (c, r) in enumerate(zip(g["clats"], got)):
        assert r["status"] == api.RESCORE_OK, i
        out = r["clat"]
        utt_len, times = R.compact_lattice_state_times(c)        # (these lattices are top-sorted: the numbering is the input's)
        ll = g["scores"][g["rows"][i]:g["rows"][i + 1]]
        todo = [(c["arc_a"][j], out["arc_a"][j], times[int(c["arc_src"][j])], c["arc_string"][j]) for j in range(len(c["arc_src"]))]
        todo += [(c["final_a"][s], out["final_a"][s], times[s], c["final_string"][s]) for s in range(int(c["n_states"])) if np.isfinite(c["final_g"][s])]
        for old, new, t0, string in todo:
            pdfs = [int(g["t2p"][int(x)]) for x in string]
            ref, bound = C.item_bound(old, [ll[t0 + k, p] for k, p in enumerate(pdfs)], [g["sizes"][p] for p in pdfs])
            if len(string) == 0:
                assert new.tobytes() == F(old).tobytes()
                continue
            err = abs(float(new) - ref)
            worst = max(worst, err / bound)
            n_items += 1
            assert err <= bound, (i, len(string), err, bound)
    print("items", n_items, "worst error / bound", worst)
    assert n_items == 36                                       # every arc and final weight with a string was looked at


def test_batching_frames_groups_consecutive_lattices(api, gmm_case):
    """--batch-frames: consecutive lattices are scored and rescored in groups of at most that many frames (one lattice
    always runs).  A group's answer is the unbatched call on the group alone, bit for bit (the same frames go through the
    scorer in the same launch shape)."""
    g = gmm_case
    rows, n = g["rows"].astype(np.int64), len(g["clats"])
    for batch_frames in (1, 100, 10 ** 6):
        groups, i = [], 0
        while i < n:
            j = i + 1
            while j < n and rows[j + 1] - rows[i] <= batch_frames:
                j += 1
            groups.append((i, j))
            i = j
        assert (len(groups) == n if batch_frames == 1 else len(groups) == 1 if batch_frames > 100 else 1 < len(groups) < n), groups
        got = api.gmm_rescore_compact_lattices(g["am"], g["feats"], rows, g["clats"], g["t2p"], batch_frames=batch_frames)
        for i, j in groups:
            want = api.gmm_rescore_compact_lattices(g["am"], g["feats"][rows[i]:rows[j]], rows[i:j + 1] - rows[i], g["clats"][i:j], g["t2p"])
            for a, b in zip(got[i:j], want):
                assert a["status"] == b["status"] == api.RESCORE_OK
                R.same_clat(a["clat"], b["clat"], batch_frames)
