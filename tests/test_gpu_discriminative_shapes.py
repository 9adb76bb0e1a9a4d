"""The lattice computations of the discriminative pass (kh_discriminative_lattice_computations: pseudo log-likelihoods ->
forward-backward -> device radix sort of the arcs' (row, pdf) keys -> SegmentKernel -> EmitKernel) against the oracle's
restatement of NnetDiscriminativeUpdater::LatticeComputations, at shapes where the sort takes several passes per key half and
several tiles: test_gpu_discriminative.py's decoded lattices give 6 + 8 key bits and a few thousand arcs.

No network: api.discriminative_lattice_computations only asks its `nnet` for compute(feats, foff, pad_input=False,
wait=False), so a stand-in hands over a prepared device matrix (rows of a float32 softmax) and the row offsets.  The
lattices come from a vectorised generator of time-synchronous, top-sorted CSR lattices (below); the checks and their
tolerances are test_gpu_discriminative.py's."""
import functools
import importlib

import numpy as np
import pytest

from oracle import binding as B

TIDS_PER_PDF = 3
SIL = [1, 2]


# ---------------------------------------------------------------- lattices
def not_multiple_of_5(a):
    """a = 0, 1, 2, ... -> 1, 2, 3, 4, 6, 7, ...: the pdfs of ordinary arcs.  The multiples of 5 are kept for the arcs whose
    posterior is exactly zero and for numerator labels that the denominator lattice does not hold."""
    return a + a // 4 + 1


def synthetic_lattice(rng, T, P, wa, wb, arcs, eps, n_active):
    """A top-sorted lattice of T frames.  Time t holds a layer A of `wa` states and a layer B of `wb` states, in that order;
    epsilon arcs lead from A to B at the same time, arcs with a transition-id from either layer at time t to layer A at
    time t + 1 (arcs[0]..arcs[1] of them per frame, eps[0]..eps[1] epsilons per time).  Every state is reached from the
    start and reaches a final state.  The arcs of frame t take their pdfs from n_active pdfs drawn for that frame (the
    first ones more often), with one of TIDS_PER_PDF transition-ids each, so that a (frame, pdf) is met by several arcs
    with several transition-ids, repeated.  Frame 0 is a single arc (posterior exactly 1).  In every third frame one arc
    has a pdf of its own and a graph cost of 400: its posterior is exactly 0 in float32.
    Returns the CSR lattice, the state times, a numerator alignment (about 2 labels in 3 are transition-ids of the
    frame's arcs, the others map to a pdf the frame does not hold; label 0 is the single arc's) and the (frame, pdf) of
    the zero-posterior arcs."""
    WA = np.full(T + 1, wa, np.int64)
    WB = np.full(T + 1, wb, np.int64)
    WA[:2] = 1
    WB[0] = WB[T] = 0
    ns_t = WA + WB
    offA = np.cumsum(ns_t) - ns_t
    offB = offA + WA
    n_states = int(ns_t.sum())
    state_time = np.repeat(np.arange(T + 1), ns_t)
    big = 1 << 30
    # arcs with a transition-id
    m = rng.integers(arcs[0], arcs[1] + 1, T)
    m[0] = 1
    assert (m[1:] > np.maximum(ns_t[1:T], WA[2:])).all()
    fr = np.repeat(np.arange(T), m)
    first = np.cumsum(m) - m
    i = np.arange(len(fr)) - first[fr]
    src = offA[fr] + np.where(i < ns_t[fr], i, rng.integers(0, big, len(fr)) % ns_t[fr])            # every state has a successor
    dst = offA[fr + 1] + np.where(i < WA[fr + 1], i, rng.integers(0, big, len(fr)) % WA[fr + 1])    # ... and layer A a predecessor
    n_ord = P - (P + 4) // 5
    n_zero = (P + 4) // 5
    active = not_multiple_of_5(rng.integers(0, n_ord, (T, n_active)))
    pdf = active[fr, rng.integers(0, n_active, (2, len(fr))).min(0)]
    graph = rng.uniform(0.0, 3.0, len(fr))
    zero_idx = rng.integers(0, n_zero, T)
    is_zero = (i == m[fr] - 1) & (fr % 3 == 1)          # (the frame's last arc: its ends are drawn, not assigned)
    pdf[is_zero] = 5 * zero_idx[fr[is_zero]]
    graph[is_zero] = 400.0
    tid = 1 + pdf * TIDS_PER_PDF + rng.integers(0, TIDS_PER_PDF, len(fr))
    # epsilon arcs
    e = rng.integers(eps[0], eps[1] + 1, T + 1)
    e[WB == 0] = 0
    assert (e >= WB).all()
    te = np.repeat(np.arange(T + 1), e)
    j = np.arange(len(te)) - (np.cumsum(e) - e)[te]
    e_src = offA[te] + rng.integers(0, big, len(te)) % WA[te]
    e_dst = offB[te] + np.where(j < WB[te], j, rng.integers(0, big, len(te)) % np.maximum(WB[te], 1))   # layer B has a predecessor
    a_src = np.concatenate([src, e_src])
    a_dst = np.concatenate([dst, e_dst])
    a_il = np.concatenate([tid, np.zeros(len(te), np.int64)])
    a_g = np.concatenate([graph, rng.uniform(0.0, 1.0, len(te))])
    perm = np.lexsort((np.arange(len(a_src)), a_src))
    off = np.zeros(n_states + 1, np.int64)
    off[1:] = np.cumsum(np.bincount(a_src, minlength=n_states))
    fin = np.full(n_states, np.inf, np.float32)
    fin[state_time == T] = rng.uniform(0.0, 1.0, int(ns_t[T]))
    assert (a_src < a_dst).all() and (state_time[a_dst] == state_time[a_src] + (a_il != 0)).all()
    # acoustic costs: those of the arcs with a transition-id are to be overwritten by the pseudo log-likelihoods; the
    # epsilon arcs keep theirs (nnet-compute-discriminative.cc:272-276), and the oracle's interface, which takes no
    # acoustic costs, has them at 0 - as the decoder's raw lattices do
    a_ac = np.where(a_il != 0, rng.uniform(0.0, 2.0, len(a_il)), 0.0)
    csr = dict(n_states=n_states, arc_offsets=off, arc_ilabel=a_il[perm].astype(np.int32), arc_nextstate=a_dst[perm].astype(np.int32),
               arc_graph=a_g[perm].astype(np.float32), arc_acoustic=a_ac[perm].astype(np.float32), state_final=fin)
    # numerator
    pick = first + rng.integers(0, big, T) % np.maximum(m - 1, 1)        # (never the zero-posterior arc)
    ali = tid[pick]
    absent = (rng.random(T) < 0.35) & (np.arange(T) > 0)
    absent_pdf = 5 * ((zero_idx + 1 + rng.integers(0, n_zero - 1, T)) % n_zero)       # (nor the zero-posterior arc's pdf)
    ali = np.where(absent, 1 + absent_pdf * TIDS_PER_PDF + rng.integers(0, TIDS_PER_PDF, T), ali).astype(np.int32)
    zf = np.unique(fr[is_zero])
    return csr, state_time, ali, (zf, 5 * zero_idx[zf])


SHAPES = {
    # P = 300: lo_bits = 9; 340 rows: hi_bits = 9 - two passes per half, the second with a one-bit mask, four in all;
    # 10-20 k arcs: several tiles, the last one partial
    "mid": dict(P=300, lens=(100, 127, 113), weights=(1.0, 0.5, 2.0), wa=6, wb=3, arcs=(30, 50), eps=(3, 6), n_active=5, seed=71),
    # P = 256: lo_bits = 8, P = 257: lo_bits = 9; 256 rows exactly: the rows take 8 bits, the key of an arc without a
    # transition-id (row = 256) the ninth
    "edge_p256": dict(P=256, lens=(90, 70, 96), weights=(1.0, 0.5, 2.0), wa=5, wb=2, arcs=(24, 36), eps=(2, 5), n_active=5, seed=72),
    "edge_p257": dict(P=257, lens=(90, 70, 96), weights=(1.0, 0.5, 2.0), wa=5, wb=2, arcs=(24, 36), eps=(2, 5), n_active=5, seed=73),
    # P = 5000: lo_bits = 13; 2000 rows: hi_bits = 11; just over 256 tiles of arcs: the scan of the sort goes round twice
    "large": dict(P=5000, lens=(230, 290, 210, 260, 270, 240, 280, 220), weights=(1.0, 0.5, 2.0, 0.25, 1.5, 0.75, 1.25, 3.0),
                  wa=24, wb=8, arcs=(450, 510), eps=(40, 60), n_active=40, seed=74),
}


@functools.lru_cache(maxsize=None)
def make_shape(name):
    """The inputs of one shape (made once, shared by its cases, not modified): lattices, alignments, maps, priors, the
    softmax rows and the cells of them that are set to exactly 0."""
    s = SHAPES[name]
    rng = np.random.default_rng(s["seed"])
    P = s["P"]
    ntid = P * TIDS_PER_PDF
    tid2pdf = np.concatenate([[0], np.arange(ntid) // TIDS_PER_PDF]).astype(np.int32)
    tid2phone = np.concatenate([[0], 1 + (np.arange(ntid) // 6) % 11]).astype(np.int32)
    row_off = np.concatenate([[0], np.cumsum(s["lens"])]).astype(np.int64)
    egs, times, zero_cells, one_cells = [], [], [], []
    for u, T in enumerate(s["lens"]):
        csr, state_time, ali, (zf, zp) = synthetic_lattice(rng, T, P, s["wa"], s["wb"], s["arcs"], s["eps"], s["n_active"])
        egs.append(dict(den_lat=csr, num_ali=ali, weight=s["weights"][u]))
        times.append(state_time)
        zero_cells.append(np.stack([row_off[u] + zf, zp], 1))
        one_cells.append([row_off[u], tid2pdf[ali[0]]])
    logits = rng.standard_normal((int(row_off[-1]), P)).astype(np.float32)
    ex = np.exp(logits - logits.max(1, keepdims=True))
    post = (ex / ex.sum(1, keepdims=True, dtype=np.float32)).astype(np.float32)
    priors = rng.uniform(0.5, 1.5, P)
    priors = (priors / priors.sum()).astype(np.float32)
    return dict(name=name, P=P, egs=egs, times=times, tid2pdf=tid2pdf, tid2phone=tid2phone, row_off=row_off, post=post, priors=priors,
                zero_cells=np.concatenate(zero_cells), one_cells=np.array(one_cells))


def posteriors_of(shape, criterion):
    """The softmax rows with a few cells at exactly 0, where the 1e-20 floor of the pseudo log-likelihoods is taken and no
    derivative comes out: the cells of the zero-posterior arcs (their entry is dropped, as MergePairVectorSumming drops a
    zero) and, for MMI, the cell of each example's frame 0, where numerator and denominator cancel exactly (1 - 1)."""
    post = shape["post"].copy()
    cells = shape["zero_cells"] if criterion != "mmi" else np.concatenate([shape["zero_cells"], shape["one_cells"]])
    post[cells[:, 0], cells[:, 1]] = 0.0
    return post


def preconditions(shape):
    """What the inputs of a shape hold, counted on the host from the lattices and the alignments."""
    P, ntid1 = shape["P"], len(shape["tid2pdf"])
    rows, tids, n_arcs, n_eps, present = [], [], 0, 0, []
    for u, e in enumerate(shape["egs"]):
        L = e["den_lat"]
        src = np.repeat(np.arange(L["n_states"]), np.diff(L["arc_offsets"]))
        il = L["arc_ilabel"].astype(np.int64)
        row = shape["row_off"][u] + shape["times"][u][src]
        rows.append(row[il != 0])
        tids.append(il[il != 0])
        n_arcs += len(il)
        n_eps += int((il == 0).sum())
    rows, tids = np.concatenate(rows), np.concatenate(tids)
    pdfs = shape["tid2pdf"][tids].astype(np.int64)
    seg, seg_arcs = np.unique(rows * P + pdfs, return_counts=True)
    rt, rt_arcs = np.unique(rows * ntid1 + tids, return_counts=True)
    rt_seg = (rt // ntid1) * P + shape["tid2pdf"][rt % ntid1]
    _, seg_tids = np.unique(rt_seg, return_counts=True)
    ali = np.concatenate([e["num_ali"] for e in shape["egs"]]).astype(np.int64)
    present = np.isin(np.arange(len(ali)) * P + shape["tid2pdf"][ali], seg)
    return dict(total_arcs=n_arcs, total_rows=len(ali), eps_fraction=n_eps / n_arcs, segments=len(seg),
                segments_of_two_arcs=int((seg_arcs >= 2).sum()), segments_of_two_tids=int((seg_tids >= 2).sum()),
                segments_with_a_repeated_tid=len(np.unique(rt_seg[rt_arcs >= 2])),
                rows_with_numerator_present=int(present.sum()), rows_with_numerator_absent=int((~present).sum()))


@pytest.mark.parametrize("name", list(SHAPES))
def test_shapes_hold_what_the_gpu_cases_rely_on(name):
    """No GPU: the generated lattices exercise what the cases below claim."""
    shape = make_shape(name)
    c = preconditions(shape)
    print(name, c)
    assert c["total_rows"] == {"mid": 340, "edge_p256": 256, "edge_p257": 256, "large": 2000}[name]
    assert c["segments_of_two_arcs"] >= 1000
    assert c["segments_of_two_tids"] >= 100
    assert c["segments_with_a_repeated_tid"] >= 100
    assert c["rows_with_numerator_present"] >= 20 and c["rows_with_numerator_absent"] >= 20   # drop_frames drops and keeps rows
    assert c["eps_fraction"] >= 0.05
    if name == "mid":
        assert 10000 <= c["total_arcs"] <= 20000 and c["total_arcs"] % 4096 != 0
    if name == "large":
        assert 256 * 4096 < c["total_arcs"] < 1.1e6
    assert len(shape["zero_cells"]) >= 20


# ---------------------------------------------------------------- the device against the oracle
class PreparedOutput:
    """Stands in for api.Nnet: the forward pass has been done."""

    def __init__(self, out, row_off):
        self.out, self.row_off = out, row_off

    def compute(self, feats, foff, pad_input=True, wait=True):
        assert not pad_input and not wait
        return self.out, self.row_off


def run_case(api, name, criterion, drop, sliced=False):
    import torch
    shape = make_shape(name)
    post = posteriors_of(shape, criterion)
    rows, P = post.shape
    if sliced:      # a column slice of a wider allocation: the row stride is not the number of columns
        wide = torch.full((rows, P + 11), 0.5, dtype=torch.float32, device="cuda")
        out = wide[:, 4:4 + P]
        out.copy_(torch.from_numpy(post))
        assert out.stride(0) == P + 11
    else:
        out = torch.from_numpy(post).cuda()
    egs = [dict(e, feats=torch.zeros((len(e["num_ali"]), 1))) for e in shape["egs"]]
    got = api.discriminative_lattice_computations(PreparedOutput(out, shape["row_off"].astype(np.int32)), shape["priors"], shape["tid2pdf"],
                                                  egs, criterion=criterion, acoustic_scale=0.1, drop_frames=drop,
                                                  tid2phone=shape["tid2phone"], silence_phones=SIL)
    torch.cuda.synchronize()
    assert np.array_equal(got["output"].cpu().numpy(), post)
    deriv = got["deriv"].cpu().numpy()
    stats = np.zeros(5)
    want = np.zeros_like(post)
    for u, e in enumerate(shape["egs"]):
        r0, r1 = shape["row_off"][u], shape["row_off"][u + 1]
        _, d = B.discriminative_lattice_computations(post[r0:r1], shape["priors"], e["den_lat"], shape["tid2pdf"], shape["tid2phone"], SIL,
                                                     e["num_ali"], criterion, 0.1, drop, False, e["weight"], stats)
        want[r0:r1] = d
    gs = got["stats"]
    got_stats = np.array([gs["tot_t"], gs["tot_t_weighted"], gs["tot_num_count"], gs["tot_num_objf"], gs["tot_den_objf"]])
    scale = np.abs(want).max()
    print(name, criterion, drop, "stats", got_stats, stats, "max|deriv - want|", np.abs(deriv - want).max(), "scale", scale,
          "non-zero", (want != 0).sum(), (deriv != 0).sum())
    assert np.isfinite(want).all() and np.isfinite(deriv).all()
    assert np.allclose(got_stats, stats, rtol=1e-5, atol=1e-4), (got_stats, stats)
    assert (want != 0).sum() > 50
    assert np.abs(deriv - want).max() < 2e-4 * scale, (np.abs(deriv - want).max(), scale)
    # the same (row, pdf) entries are non-zero, up to cancellations at float rounding
    both = (np.abs(want) > 1e-3 * scale) | (np.abs(deriv) > 1e-3 * scale)
    assert np.array_equal((want != 0) & both, (deriv != 0) & both)
    if criterion == "mmi":   # where the posteriors are 0 nothing came out (dropped zero entries; 1 - 1 at frame 0)
        cells = np.concatenate([shape["zero_cells"], shape["one_cells"]])
        assert not deriv[cells[:, 0], cells[:, 1]].any() and not want[cells[:, 0], cells[:, 1]].any()
    return got


MID_CASES = [("mmi", False), ("mmi", True), ("smbr", False)]
_mid_default = {}


def mid_default(api, criterion, drop):
    """The `mid` shape's checked result at the default switches (once per case; call before a switch is set)."""
    if (criterion, drop) not in _mid_default:
        got = run_case(api, "mid", criterion, drop)
        _mid_default[criterion, drop] = (got, api.lattice_last_plan())
    return _mid_default[criterion, drop]


@pytest.mark.gpu
@pytest.mark.parametrize("criterion,drop", MID_CASES)
def test_mid_shape(api, criterion, drop):
    got, plan = mid_default(api, criterion, drop)
    # MMI: dataflow preparation and sweep; sMBR: the level preparation, AlphaBetaKernel + MpeKernel (no forward-backward sweep)
    want = (1, 1) if criterion == "mmi" else (0, -1)
    assert (plan["prep_dataflow"], plan["sweep_dataflow"]) == want, plan


@pytest.mark.gpu
@pytest.mark.parametrize("switch", ["KH_LATTICE_LEVELS", "KH_LATTICE_ONE_STREAM"])
@pytest.mark.parametrize("criterion,drop", MID_CASES)
def test_mid_shape_under_a_switch(api, monkeypatch, switch, criterion, drop):
    """KH_LATTICE_LEVELS=1: MMI's forward-backward runs ForwardBackwardKernel on a level-prepared batch; KH_LATTICE_ONE_STREAM=1:
    the steps beside the forward pass run on the library's stream.  Either way the checks of run_case hold and the derivative
    and the statistics EQUAL the default run's: the sweeps fold the same operands in the same order, and the radix sort behind
    them is stable."""
    import torch
    base, _ = mid_default(api, criterion, drop)
    monkeypatch.setenv(switch, "1")
    got = run_case(api, "mid", criterion, drop)
    plan = api.lattice_last_plan()
    if switch == "KH_LATTICE_LEVELS":
        assert (plan["prep_dataflow"], plan["sweep_dataflow"]) == ((0, 0) if criterion == "mmi" else (0, -1)), plan
    else:
        assert (plan["prep_dataflow"], plan["sweep_dataflow"]) == ((1, 1) if criterion == "mmi" else (0, -1)), plan
    assert torch.equal(got["deriv"], base["deriv"])
    assert got["stats"] == base["stats"], (got["stats"], base["stats"])
    assert got["objf"] == base["objf"] and got["weight"] == base["weight"]


@pytest.mark.gpu
def test_begin_without_a_second_stream_is_refused(api, monkeypatch):
    """KH_LATTICE_ONE_STREAM=1 leaves nothing for an overlapped call to run on: begin=True raises, and the next plain call
    is untouched."""
    import torch
    shape = make_shape("mid")
    out = torch.from_numpy(posteriors_of(shape, "mmi")).cuda()
    egs = [dict(e, feats=torch.zeros((len(e["num_ali"]), 1))) for e in shape["egs"]]
    call = lambda **kw: api.discriminative_lattice_computations(
        PreparedOutput(out, shape["row_off"].astype(np.int32)), shape["priors"], shape["tid2pdf"], egs, criterion="mmi", acoustic_scale=0.1,
        drop_frames=False, tid2phone=shape["tid2phone"], silence_phones=SIL, **kw)
    base, _ = mid_default(api, "mmi", False)
    monkeypatch.setenv("KH_LATTICE_ONE_STREAM", "1")
    with pytest.raises(api.KhError, match="no second stream"):
        call(begin=True)
    monkeypatch.delenv("KH_LATTICE_ONE_STREAM")
    got = call()
    torch.cuda.synchronize()
    assert torch.equal(got["deriv"], base["deriv"]) and got["stats"] == base["stats"]


@pytest.mark.gpu
def test_mid_shape_output_as_a_column_slice(api):
    run_case(api, "mid", "mmi", True, sliced=True)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["edge_p256", "edge_p257"])
def test_power_of_two_edges(api, name):
    run_case(api, name, "mmi", False)


@pytest.mark.gpu
def test_large_shape(api):
    """1 056 432 arcs in 258 tiles, 76 764 (row, pdf) segments.  Measured on an MI355X: max|deriv - want| = 3.9e-3 at a
    scale of 5.3e5 (7e-9 of it, an ulp of the largest entries; the bound is 2e-4), the same 76 814 non-zero entries, the
    statistics equal to 2e-9 relative."""
    run_case(api, "large", "mmi", False)
