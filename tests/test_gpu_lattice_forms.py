"""GPU: every form of the lattice kernels of csrc/kh_lattice.hip - the two preparations (dependency levels / dataflow), the
two sweeps (by level / dataflow: window direct or tagged, staging 384 or 192, every arc of a block staged or not), the
level-only alpha-beta and MPE kernels, the counters in LDS or in device memory, the refusals - on lattices wide enough to
reach them (lattice_cases.py; test_lattice_cases.py holds their preconditions), against the CPU oracle and, form against
form, bit for bit.  After each call api.lattice_last_plan() says which form ran: a test that misses its branch fails.

Tolerances are test_gpu_lattice.py's: up to 5 000 states tot_like 1e-9 relative, arc_post 1e-6, acoustic_like_sum 1e-6
relative, state times equal; above (its config-5 figures) tot_like 1e-8, arc_post 1e-5, alpha / beta rtol 1e-11 atol 1e-8,
sMBR score 1e-7.  Form against form: arc_post, tot_like and state_times are EQUAL (the library is built with
-ffp-contract=off and every form folds a state's arcs in ascending arc order); acoustic_like_sum is a per-lane sum, equal only
between forms that deal the arcs to the lanes alike (direct / tagged at the same staging size), else held to 1e-6.

Measured on an MI355X against the oracle (every case prints its figures): tot_like within 1.3e-16 relative, arc_post equal
as float32, acoustic_like_sum within 2.8e-14 relative, alpha / beta of `dense` within 8.9e-16, sMBR / MPFE scores within
1.2e-16 relative - the lattices are 4-5 frames deep, so a state's value is a handful of LogAdds from the start."""
import functools

import numpy as np
import pytest

import lattice_cases as LC
from oracle import binding as B
from test_gpu_lattice import _trans
from test_lattice_oracle import random_lattice

pytestmark = pytest.mark.gpu

SWITCHES = ("KH_LATTICE_WIN", "KH_LATTICE_LEVELS", "KH_LATTICE_DATAFLOW", "KH_LATTICE_ONE_STREAM")
FORMS = {
    "default": {},
    "win512": {"KH_LATTICE_WIN": "512"},
    "levels": {"KH_LATTICE_LEVELS": "1"},
    "levels_dataflow": {"KH_LATTICE_LEVELS": "1", "KH_LATTICE_DATAFLOW": "1"},
    "levels_dataflow_win512": {"KH_LATTICE_LEVELS": "1", "KH_LATTICE_DATAFLOW": "1", "KH_LATTICE_WIN": "512"},
}


@pytest.fixture(autouse=True)
def clean_switches(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


def set_form(monkeypatch, form):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in FORMS[form].items():
        monkeypatch.setenv(k, v)


@functools.lru_cache(maxsize=None)
def case(name):
    """(lattice, the oracle's forward-backward of it): made once, shared, not modified."""
    L = LC.make(name)
    return L, B.lattice_forward_backward(L)


def cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def rel(a, b):
    return abs(a - b) / max(1.0, abs(b))


def check_oracle(L, got, want):
    big = L["n_states"] > 5000
    e_tot, e_post, e_ac = rel(got["tot_like"], want["tot_like"]), float(np.abs(got["arc_post"] - want["arc_post"]).max()), \
        rel(got["acoustic_like_sum"], want["acoustic_like_sum"])
    print("states %d: tot_like rel %.3g, arc_post abs %.3g, acoustic_like_sum rel %.3g" % (L["n_states"], e_tot, e_post, e_ac))
    assert e_tot < (1e-8 if big else 1e-9)
    assert e_post < (1e-5 if big else 1e-6)
    assert np.array_equal(got["state_times"], want["state_times"])
    assert e_ac < 1e-6


def same_bits(a, b, ac):
    """Two device forms: equal posteriors, totals and times; ac: the per-lane sums are dealt alike, so they are equal too."""
    assert np.array_equal(a["arc_post"].view(np.int32), b["arc_post"].view(np.int32))
    assert a["tot_like"] == b["tot_like"]
    assert np.array_equal(a["state_times"], b["state_times"])
    if ac:
        assert a["acoustic_like_sum"] == b["acoustic_like_sum"]
    else:
        assert rel(a["acoustic_like_sum"], b["acoustic_like_sum"]) < 1e-6


def plan_is(api, **want):
    plan = api.lattice_last_plan()
    assert {k: plan[k] for k in want} == want, plan
    return plan


# what far256 alone (one workgroup per CU) must report, by form
FAR256_PLAN = {
    "default": dict(prep_dataflow=1, prep_per_cu=1, prep_win=4096, prep_lds_states=1601, n_prep_off_lds=0, sweep_dataflow=1, sweep_per_cu=1,
                    sweep_stage=384, sweep_win=2048, n_tagged=0),
    "win512": dict(prep_dataflow=1, n_prep_off_lds=0, sweep_dataflow=1, sweep_stage=384, sweep_win=512, n_tagged=1),
    "levels": dict(prep_dataflow=0, prep_lds_states=5120, n_prep_off_lds=0, sweep_dataflow=0, n_tagged=0),
    "levels_dataflow": dict(prep_dataflow=0, n_prep_off_lds=0, sweep_dataflow=1, sweep_stage=384, sweep_win=2048, n_tagged=0),
    "levels_dataflow_win512": dict(prep_dataflow=0, n_prep_off_lds=0, sweep_dataflow=1, sweep_stage=384, sweep_win=512, n_tagged=1),
}
_far256_default = {}


def far256_default(api):
    """far256 at the default switches (direct window, every operand from LDS), checked against the oracle, once."""
    if not _far256_default:
        L, want = case("far256")
        got = api.lattice_forward_backward([L])[0]
        plan_is(api, **FAR256_PLAN["default"])
        check_oracle(L, got, want)
        _far256_default["r"] = got
    return _far256_default["r"]


# ---------------------------------------------------------------- a. far256: four forms (and the tagged sweep on a level batch)
@pytest.mark.parametrize("form", list(FORMS))
def test_far256_forms(api, monkeypatch, form):
    """55 % of far256's arcs span more than 256 states: under KH_LATTICE_WIN=512 (256 tagged slots) their operand has left
    the window and is read from memory (WinRead<false>'s `evicted` branch); block 0 has more outgoing arcs than the staging
    area (the unstaged loop forms, backward).  Every form gives the default form's bits and the oracle's numbers."""
    L, want = case("far256")
    base = far256_default(api)
    set_form(monkeypatch, form)
    got = api.lattice_forward_backward([L])[0]
    plan_is(api, cus=cus(), **FAR256_PLAN[form])
    check_oracle(L, got, want)
    same_bits(got, base, ac=form in ("default", "win512"))


@pytest.mark.parametrize("form", list(FORMS))
def test_far256_forms_resident_batch(api, monkeypatch, form):
    """The same through api.LatticeBatch (created and swept under the form's switches)."""
    L, want = case("far256")
    base = far256_default(api)
    set_form(monkeypatch, form)
    batch = api.LatticeBatch([L])
    r = batch.forward_backward(want_times=True)
    plan_is(api, **FAR256_PLAN[form])
    got = dict(arc_post=r["arc_post"], tot_like=float(r["tot_like"][0]), acoustic_like_sum=float(r["acoustic_like_sum"][0]),
               state_times=r["state_times"])
    check_oracle(L, got, want)
    same_bits(got, base, ac=form in ("default", "win512"))
    if form == "default":
        d = batch.forward_backward_device()
        plan_is(api, **FAR256_PLAN[form])
        assert np.array_equal(d["arc_post"].cpu().numpy().view(np.int32), base["arc_post"].view(np.int32))
        assert d["tot_like"][0] == base["tot_like"] and d["acoustic_like_sum"][0] == base["acoustic_like_sum"]


# ---------------------------------------------------------------- b. far1024 behind fillers: four workgroups per CU
@functools.lru_cache(maxsize=None)
def filler():
    return random_lattice(np.random.default_rng(1024), n_frames=3, width=4)


def test_far1024_behind_fillers(api):
    """3 * CUs + 1 lattices: four workgroups per CU.  far1024 then has its preparation counters in device memory (4 401 >
    2 816 states), its state times through a 1024-slot window that 45 % of its arcs overrun (`tag > src` in PrepKernelDF), and
    its sweeps in the tagged form with the 192 staging (ForwardBackwardDFKernel<false, 192>, blocks over 192 arcs both ways).
    Alone it is direct with counters in LDS: the same bits.  The fillers equal one another."""
    L, want = case("far1024")
    n_fill = 3 * cus()
    alone = api.lattice_forward_backward([L])[0]
    plan_is(api, prep_dataflow=1, prep_per_cu=1, prep_lds_states=4401, n_prep_off_lds=0, sweep_dataflow=1, sweep_stage=384, sweep_win=8192,
            n_tagged=0)
    check_oracle(L, alone, want)
    out = api.lattice_forward_backward([filler()] * n_fill + [L])
    plan_is(api, prep_dataflow=1, prep_per_cu=4, prep_win=1024, prep_lds_states=2816, n_prep_off_lds=1, sweep_dataflow=1, sweep_per_cu=4,
            sweep_stage=192, sweep_win=2048, n_tagged=1)
    check_oracle(L, out[-1], want)
    same_bits(out[-1], alone, ac=False)      # (192 against 384 staged arcs: the lanes' sums are dealt differently)
    check_oracle(filler(), out[0], B.lattice_forward_backward(filler()))
    for r in out[1:-1]:
        same_bits(r, out[0], ac=True)


# ---------------------------------------------------------------- c. 1 200 lattices, tagged + 192 staging + staging overflow
def test_many_lattices_tagged_with_small_staging(api, monkeypatch):
    """The batch of test_gpu_lattice.test_window_forms_and_staging_overflow (four lattices 300 times over; the width-24 one has
    blocks of more arcs than either staging area) on the device once, swept at the default window (direct: it holds the largest lattice)
    and under KH_LATTICE_WIN=512 (tagged, staging 192): equal bits, and the oracle's numbers."""
    rng = np.random.default_rng(41)
    lats = [random_lattice(rng, n_frames=150, width=7), random_lattice(rng, n_frames=40, width=24, eps_frac=0.05),
            random_lattice(rng, n_frames=3, width=2), random_lattice(rng, n_frames=260, width=5)]
    reps = 300
    assert 4 * reps > 3 * cus(), "four workgroups per CU need more than 3 * CUs lattices"
    n_big = sum(L["n_states"] > 512 for L in lats)
    assert n_big >= 1 and max(L["n_states"] for L in lats) <= 2048
    assert LC.facts(lats[1], 256)["in_blocks_over_192"] >= 1 and LC.facts(lats[1], 256)["out_blocks_over_192"] >= 1
    batch = api.LatticeBatch(lats * reps)
    direct = batch.forward_backward(want_times=True)
    plan_is(api, prep_dataflow=1, prep_per_cu=4, sweep_dataflow=1, sweep_per_cu=4, sweep_stage=192, n_tagged=0)
    monkeypatch.setenv("KH_LATTICE_WIN", "512")
    tagged = batch.forward_backward(want_times=True)
    plan_is(api, sweep_dataflow=1, sweep_stage=192, sweep_win=512, n_tagged=n_big * reps)
    for k in ("arc_post", "tot_like", "acoustic_like_sum", "state_times"):
        assert np.array_equal(direct[k], tagged[k]), k
    a0 = 0
    for i, L in enumerate(lats):
        na = len(L["arc_ilabel"])
        got = dict(arc_post=tagged["arc_post"][a0:a0 + na], tot_like=float(tagged["tot_like"][i]),
                   acoustic_like_sum=float(tagged["acoustic_like_sum"][i]),
                   state_times=tagged["state_times"][batch.soff[i]:batch.soff[i + 1]])
        check_oracle(L, got, B.lattice_forward_backward(L))
        a0 += na
    total = a0
    for rep in (1, reps - 1):      # the copies equal the first four
        assert np.array_equal(tagged["arc_post"][rep * total:(rep + 1) * total], tagged["arc_post"][:total])
        assert np.array_equal(tagged["tot_like"][4 * rep:4 * rep + 4], tagged["tot_like"][:4])


# ---------------------------------------------------------------- d. far8192: the default sizes' largest forms
def test_far8192_alone(api, monkeypatch):
    """28 001 states in one workgroup: more than the 27 392 whose counters fit the LDS beside a 4096-slot state-time window,
    and more than the 16 384-slot value window (8 192 tagged slots, overrun by 26 % of the arcs).  Against the oracle, and
    against the level-based kernels (whose preparation counts in device memory too) bit for bit."""
    L, want = case("far8192")
    got = api.lattice_forward_backward([L])[0]
    plan_is(api, prep_dataflow=1, prep_per_cu=1, prep_win=4096, prep_lds_states=27392, n_prep_off_lds=1, sweep_dataflow=1, sweep_per_cu=1,
            sweep_stage=384, sweep_win=16384, n_tagged=1)
    check_oracle(L, got, want)
    monkeypatch.setenv("KH_LATTICE_LEVELS", "1")
    lev = api.lattice_forward_backward([L])[0]
    plan_is(api, prep_dataflow=0, n_prep_off_lds=1, sweep_dataflow=0)
    same_bits(lev, got, ac=False)


# ---------------------------------------------------------------- e. dense: the level kernels at width
@pytest.mark.parametrize("viterbi", [False, True])
def test_dense_alphas_betas(api, viterbi):
    """Levels of up to 853 states (the k += kThreads loops), 61 blocks of more than 384 incoming entries (SortIncomingLists'
    insertion sort in memory), 5 201 states (PrepKernel's counters in device memory)."""
    L, _ = case("dense")
    got = api.lattice_alphas_betas([L], viterbi)[0]
    plan_is(api, prep_dataflow=0, prep_lds_states=5120, n_prep_off_lds=1, sweep_dataflow=-1)
    want = B.lattice_alphas_betas(L, viterbi)
    print("alpha abs %.3g, beta abs %.3g" % (np.abs(got["alpha"] - want["alpha"]).max(), np.abs(got["beta"] - want["beta"]).max()))
    assert np.allclose(got["alpha"], want["alpha"], rtol=1e-11, atol=1e-8) and np.allclose(got["beta"], want["beta"], rtol=1e-11, atol=1e-8)
    assert abs(got["tot"] - want["tot"]) < 1e-8 * max(1.0, abs(want["tot"]))
    if viterbi:  # max / plus only: exact
        assert np.array_equal(got["alpha"], want["alpha"]) and np.array_equal(got["beta"], want["beta"])


@pytest.mark.parametrize("criterion,one_class", [("smbr", False), ("smbr", True), ("mpfe", False), ("mpfe", True)])
def test_dense_mpe(api, criterion, one_class):
    L, _ = case("dense")
    T = LC.SHAPES["dense"][0]
    rng = np.random.default_rng(77)
    t2ph, t2pdf = _trans(rng)
    ali = rng.integers(1, 50, T).astype(np.int32)
    got = api.lattice_forward_backward_mpe([L], t2ph, t2pdf, [2, 5], [ali], criterion, one_class)[0]
    plan_is(api, prep_dataflow=0, n_prep_off_lds=1, sweep_dataflow=-1)
    want = B.lattice_forward_backward_mpe(L, t2ph, t2pdf, [2, 5], ali, criterion, one_class)
    print("score rel %.3g, arc_post abs %.3g" % (rel(got["tot_forward_score"], want["tot_forward_score"]),
                                                np.abs(got["arc_post"] - want["arc_post"]).max()))
    assert rel(got["tot_forward_score"], want["tot_forward_score"]) < 1e-7
    assert np.abs(got["arc_post"] - want["arc_post"]).max() < 1e-5
    assert np.abs(want["arc_post"]).max() > 1e-4      # (the comparison is of something)


def test_dense_forward_backward_by_level(api, monkeypatch):
    """ForwardBackwardKernel (KH_LATTICE_LEVELS) on wide levels, against the oracle and the dataflow form's bits."""
    L, want = case("dense")
    df = api.lattice_forward_backward([L])[0]
    plan_is(api, prep_dataflow=1, n_prep_off_lds=0, sweep_dataflow=1, sweep_win=8192, n_tagged=0)
    check_oracle(L, df, want)
    monkeypatch.setenv("KH_LATTICE_LEVELS", "1")
    lev = api.lattice_forward_backward([L])[0]
    plan_is(api, prep_dataflow=0, n_prep_off_lds=1, sweep_dataflow=0)
    check_oracle(L, lev, want)
    same_bits(lev, df, ac=False)


def test_dense_beside_far256(api, monkeypatch):
    """One batch, two lattices: dense counts in device memory, far256 in LDS (the level preparation chooses per lattice).
    Each equals its result alone."""
    D, wd = case("dense")
    F, wf = case("far256")
    f_default = far256_default(api)
    ab_alone = [api.lattice_alphas_betas([X])[0] for X in (D, F)]
    ab = api.lattice_alphas_betas([D, F])
    plan_is(api, prep_dataflow=0, n_prep_off_lds=1)
    for a, b in zip(ab, ab_alone):
        assert np.array_equal(a["alpha"], b["alpha"]) and np.array_equal(a["beta"], b["beta"]) and a["tot"] == b["tot"]
    monkeypatch.setenv("KH_LATTICE_LEVELS", "1")
    for order in ((D, F), (F, D)):
        out = api.lattice_forward_backward(list(order))
        plan_is(api, prep_dataflow=0, n_prep_off_lds=1, sweep_dataflow=0)
        for X, r in zip(order, out):
            check_oracle(X, r, wd if X is D else wf)
        same_bits(out[0 if order[0] is F else 1], f_default, ac=False)


# ---------------------------------------------------------------- f. refusals
def inconsistent_lattice():
    """0 -> 1 -> 2 with transition-ids and 0 -> 2 with one: state 2 at time 1 and at time 2."""
    return dict(n_states=3, arc_offsets=np.array([0, 2, 3, 3], np.int64), arc_ilabel=np.array([1, 1, 2], np.int32),
                arc_nextstate=np.array([1, 2, 2], np.int32), arc_graph=np.zeros(3, np.float32), arc_acoustic=np.zeros(3, np.float32),
                state_final=np.array([np.inf, np.inf, 0], np.float32))


def unsorted_lattice():
    return dict(n_states=2, arc_offsets=np.array([0, 1, 2], np.int64), arc_ilabel=np.array([1, 2], np.int32),
                arc_nextstate=np.array([1, 0], np.int32), arc_graph=np.zeros(2, np.float32),
                arc_acoustic=np.zeros(2, np.float32), state_final=np.array([np.inf, 0], np.float32))


@pytest.mark.parametrize("bad,message", [(inconsistent_lattice, "inconsistent state times at state 2"), (unsorted_lattice, "topologically sorted")],
                         ids=["inconsistent", "unsorted"])
@pytest.mark.parametrize("prep", ["dataflow", "levels"])
def test_refusals(api, bad, message, prep):
    """The bad lattice is the middle one of three: both preparations name it, and the next call is untouched."""
    rng = np.random.default_rng(61)
    good = [random_lattice(rng, n_frames=9, width=5) for _ in range(2)]
    call = api.lattice_forward_backward if prep == "dataflow" else api.lattice_alphas_betas
    clean = call(good)
    plan_is(api, prep_dataflow=1 if prep == "dataflow" else 0)
    with pytest.raises(api.KhError, match=message) as e:
        call([good[0], bad(), good[1]])
    assert "lattice 1:" in str(e.value)
    plan_is(api, prep_dataflow=1 if prep == "dataflow" else 0, sweep_dataflow=-1)      # (no sweep ran)
    again = call(good)
    for a, b in zip(again, clean):
        for k in a:
            if k != "post":
                assert np.array_equal(a[k], b[k]), k


def test_inconsistency_found_through_the_evicted_window(api):
    """far1024 with one more arc from frame 2 into the last state (frame 4), behind the fillers: the predecessor that
    disagrees lies more than the 1024 slots of the state-time window back."""
    L, _ = case("far1024")
    T, W = LC.SHAPES["far1024"][:2]
    s, d = 1 + W + 7, L["n_states"] - 1
    assert d - s > 1024
    bad = LC.add_arc(L, s, d, 5, 1.0, 1.0)
    n_fill = 3 * cus()
    with pytest.raises(api.KhError, match="inconsistent state times at state %d " % d) as e:
        api.lattice_forward_backward([filler()] * n_fill + [bad])
    assert "lattice %d:" % n_fill in str(e.value)
    plan_is(api, prep_dataflow=1, prep_per_cu=4, prep_win=1024, n_prep_off_lds=1, sweep_dataflow=-1)
    with pytest.raises(api.KhError, match="inconsistent state times at state %d " % d):      # ... and the level preparation
        api.lattice_alphas_betas([filler(), bad, filler()])
    ok = api.lattice_forward_backward([filler(), L])
    same_bits(ok[0], api.lattice_forward_backward([filler()])[0], ac=True)


# ---------------------------------------------------------------- g. kh_lattice_state_times
def one_state_lattice():
    e = lambda dt: np.zeros(0, dt)
    return dict(n_states=1, arc_offsets=np.zeros(2, np.int64), arc_ilabel=e(np.int32), arc_nextstate=e(np.int32), arc_graph=e(np.float32),
                arc_acoustic=e(np.float32), state_final=np.zeros(1, np.float32))


def with_extra_root(L):
    """L with one more state just before its last state f: no incoming arc, one arc (a transition-id) into f, which keeps
    its place as the last state.  The new arc is the last arc."""
    n = L["n_states"]
    assert L["arc_offsets"][n] == L["arc_offsets"][n - 1] and np.isfinite(L["state_final"][n - 1])      # f: final, no arcs out
    nxt = L["arc_nextstate"].copy()
    nxt[nxt == n - 1] = n
    app = lambda k, v: np.concatenate([L[k], np.array([v], L[k].dtype)])
    A = int(L["arc_offsets"][n])
    return dict(n_states=n + 1, arc_offsets=np.concatenate([L["arc_offsets"][:n], [A + 1, A + 1]]).astype(np.int64),
                arc_ilabel=app("arc_ilabel", 7), arc_nextstate=np.concatenate([nxt, np.array([n], np.int32)]),
                arc_graph=app("arc_graph", 0.5), arc_acoustic=app("arc_acoustic", 0.25),
                state_final=np.concatenate([L["state_final"][:n - 1], np.array([np.inf, L["state_final"][n - 1]], np.float32)]))


@pytest.mark.parametrize("prep", ["dataflow", "levels"])
def test_state_times_batch(api, monkeypatch, prep):
    """kh_lattice_state_times (the only caller of the preparation without cost arrays) against the oracle's LatticeStateTimes."""
    if prep == "levels":
        monkeypatch.setenv("KH_LATTICE_LEVELS", "1")
    rng = np.random.default_rng(62)
    small = [random_lattice(rng, n_frames=int(T), width=5) for T in (1, 8, 33)]
    lats = [case("far256")[0], small[0], one_state_lattice(), case("dense")[0], small[1], small[2]]
    want = [case("far256")[1]["state_times"], None, np.zeros(1, np.int32), case("dense")[1]["state_times"], None, None]
    got = api.lattice_state_times_batch(lats)
    plan_is(api, prep_dataflow=1 if prep == "dataflow" else 0, n_prep_off_lds=1 if prep == "levels" else 0, sweep_dataflow=-1)
    for L, w, g in zip(lats, want, got):
        w = B.lattice_forward_backward(L)["state_times"] if w is None else w
        assert np.array_equal(g["state_times"], w) and g["max_time"] == int(w.max())
        if L["n_states"] < 300:
            assert np.array_equal(api.lattice_state_times(L), w)      # (the Python loop agrees)


@pytest.mark.parametrize("prep", ["dataflow", "levels"])
def test_extra_root_state(api, monkeypatch, prep):
    """A state without incoming arcs that is not state 0: no path from the start reaches it.  include/kaldi_hip.h's contract:
    its time is -1, the other times are unchanged (the reference's loop would hand time -1 + 1 on to its successor and
    assert: DESIGN.md); its arc's posterior is exactly 0, everything else keeps its bits."""
    if prep == "levels":
        monkeypatch.setenv("KH_LATTICE_LEVELS", "1")
    base = random_lattice(np.random.default_rng(63), n_frames=12, width=6)
    n = base["n_states"]
    X = with_extra_root(base)
    want_t = B.lattice_forward_backward(base)["state_times"]      # (the oracle is never given X: it aborts as the reference does)
    t = api.lattice_state_times_batch([base, X, base])
    assert np.array_equal(t[0]["state_times"], want_t) and np.array_equal(t[2]["state_times"], want_t)
    assert np.array_equal(t[1]["state_times"], np.concatenate([want_t[:n - 1], [-1], want_t[n - 1:]]))
    assert t[1]["max_time"] == t[0]["max_time"] == int(want_t.max())
    r0, r1 = api.lattice_forward_backward([base, X])
    plan_is(api, prep_dataflow=1 if prep == "dataflow" else 0, sweep_dataflow=1 if prep == "dataflow" else 0)
    check_oracle(base, r0, B.lattice_forward_backward(base))
    assert r1["arc_post"][-1] == 0.0
    assert np.array_equal(r1["arc_post"][:-1].view(np.int32), r0["arc_post"].view(np.int32)) and r1["tot_like"] == r0["tot_like"]
    assert np.array_equal(r1["state_times"], t[1]["state_times"])
    assert rel(r1["acoustic_like_sum"], r0["acoustic_like_sum"]) < 1e-6
