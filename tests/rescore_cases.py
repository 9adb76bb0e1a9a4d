"""Helpers of the acoustic-rescoring tests (test_rescore_restatement.py, test_gpu_lattice_rescore.py,
test_gpu_rescore_tools.py): a transition-id -> pdf table that shares pdfs, hand lattices that put every string length and
every status in front of kh_rescore_compact_lattice, and the end-to-end error bound.

THE END-TO-END BOUND (item_bound).  An item's new cost is v = old, then v = fl32((-s_k) + v) for its len scores s_k in
string order.  The test compares the device's v, built from the device's GMM scores d_k, with R = old + sum(-o_k) in
float64, built from the CPU oracle's scores o_k.  tests/gmm_cases.py derives, against the float64 LogSumExp ref_k of the
same float32 per-Gaussian scores,
    |d_k - ref_k| <= c(n_k) + 1/2 ulp32(d_k)          (terms a .. g, then the final rounding h)
    |o_k - ref_k| <= 2^-21 + 2^-23 + 1/2 ulp32(o_k)   (terms a, d and h), and 2^-21 + 2^-23 < c(n) for every n,
n_k = the number of Gaussians of the pdf.  So per score |d_k - o_k| <= 2 c(n_k) + ulp32(|o_k| + 2 c(n_k)): the c part and
the two final roundings, the ulp taken at |o_k| + 2 c so that a score pushed over a binade edge is covered.  Each of the
len float additions of the device's chain rounds its partial sum by at most half an ulp; R's float64 additions add
len 2^-53 relative, which is nothing next to that.  With M = the largest |partial sum| of the float64 chain plus the c
and ulp terms above, times 1 + len 2^-23 for the roundings themselves (so that it bounds the device's partial sums too):

    |v - R| <= sum_k [2 c(n_k) + ulp32(|o_k| + 2 c(n_k))] + len * 1/2 ulp32(M).

Nothing in it is measured from the kernel."""
import numpy as np

import gmm_cases as G
import latalign_cases as A

F = np.float32
NUM_TIDS = 240
N_PDFS = 37


def tid2pdf(n_pdfs=N_PDFS):
    """num_tids + 1 entries: transition-ids 2 j + 1 and 2 j + 2 (a self-loop and the transition forward) share pdf j mod
    n_pdfs, as they do in a TransitionModel."""
    t = np.zeros(NUM_TIDS + 1, np.int32)
    t[1:] = (np.arange(NUM_TIDS) // 2) % n_pdfs
    return t


def tids(rng, n):
    return [int(x) for x in rng.integers(1, NUM_TIDS + 1, n)]


SHORT_LEN = 8                                   # kShortLen, csrc/kh_latrescore.hip: longer strings go to the wave kernel
LENGTHS = (0, 1, 2, SHORT_LEN, SHORT_LEN + 1, 63, 64, 65, 130)


def lengths_clat(seed=5, final_len=3):
    """A chain with two parallel arcs per step - strings of every length of LENGTHS, the second arc's with other ids - whose
    last state is final with a string of final_len ids (0: the last arc ends at the last frame); every other final weight
    is Zero.  One pair of transition-ids sharing a pdf sits on the length-2 arcs."""
    rng = np.random.default_rng(seed)
    arcs = []
    for i, n in enumerate(LENGTHS):
        for k in range(2):
            s = tids(rng, n)
            if n == 2:
                s = [5, 6] if k == 0 else [6, 5]          # pdf 2 twice
            arcs.append((i, i + 1, 1 + k, float(F(rng.uniform(0, 3))), float(F(rng.uniform(-2, 5))), s))
    last = len(LENGTHS)
    return A.clat(last + 1, arcs, {last: (0.25, 1.5, tids(rng, final_len))})


def long_final_clat(seed=6):
    """Final weights with strings on two states, one of them longer than a wave (70 ids): utt_len agrees on both."""
    rng = np.random.default_rng(seed)
    arcs = [(0, 1, 3, 0.5, 0.25, tids(rng, 4)), (1, 2, 4, 1.0, 0.5, tids(rng, 66)), (0, 2, 5, 1.5, 0.75, tids(rng, 70))]
    return A.clat(3, arcs, {1: (0.5, 2.0, tids(rng, 70)), 2: (0.125, -1.0, tids(rng, 4))})


def negative_zero_clat():
    """Empty strings on an arc and on a final weight whose old acoustic costs are -0.0, next to an arc that is rescored."""
    c = A.clat(3, [(0, 1, 7, 0.5, -0.0, []), (1, 2, 8, 0.25, -0.0, [3, 4, 9])], {2: (1.0, -0.0, [])})
    assert np.signbit(c["arc_a"][0]) and np.signbit(c["final_a"][2])
    return c


def empty_clat():
    return A.empty()


def inconsistent_clat():
    """Two paths of different length into state 2 (the assertion at :87)."""
    return A.clat(3, [(0, 1, 1, 0.0, 0.0, [1, 2]), (0, 2, 2, 0.0, 0.0, [1, 2, 3, 4]), (1, 2, 3, 0.0, 0.0, [5])], {2: (0.0, 0.0, [])})


def unreachable_clat():
    """State 1 has no incoming arc: its time stays -1 (:1187).  Its arc is 3 ids long, so that -1 + 3 agrees with the time of
    state 2 and the assertion at :87 does not fire first."""
    return A.clat(3, [(0, 2, 1, 0.5, 0.5, [1, 2]), (1, 2, 2, 0.5, 0.5, [3, 4, 5])], {2: (0.0, 0.0, [])})


def bad_tid_clat(tid):
    return A.clat(3, [(0, 1, 1, 0.5, 0.5, [1, 2]), (1, 2, 2, 0.5, 0.5, [3, tid, 4])], {2: (0.0, 0.0, [])})


def plain_clat(seed=7, n=4, length=3):
    rng = np.random.default_rng(seed)
    arcs = [(i, i + 1, i + 1, float(F(rng.uniform(0, 2))), float(F(rng.uniform(0, 2))), tids(rng, length)) for i in range(n)]
    return A.clat(n + 1, arcs, {n: (0.5, 0.25, [])})


def utt_len_of(clat):
    import rescore_restatement as R
    c = clat
    if not (R.is_top_sorted(c) and int(c.get("start", 0)) == 0):
        c = R.renumber(c, R.top_sort(int(c["n_states"]), int(c["start"]), c["arc_src"], c["arc_dst"]))
    return R.compact_lattice_state_times(c)[0]


def unsorted_clat():
    """A lattice numbered against its arcs: start state 2, an arc 3 -> 1, strings with a consistent time per state."""
    arcs = [(2, 3, 1, 0.5, 0.5, [1, 2]), (2, 0, 2, 1.0, 0.25, [3, 4, 5]), (3, 1, 3, 0.25, 0.5, [6, 7, 8, 9]), (0, 1, 4, 0.5, 1.5, [10, 11, 12])]
    return A.clat(4, arcs, {1: (0.0, 0.0, [])}, start=2)


def generated_batch():
    """About 50 lattices: the generator sets of the MBR and the word-alignment tests."""
    import latmbr_cases as M
    return M.generator_clats() + A.batch(11, 30)


def item_bound(old, scores, sizes):
    """The bound of the module docstring for one item: old cost, the oracle's scores o_k (float32) and n_k in string order.
    Returns (R, bound) in float64."""
    o = np.asarray(scores, np.float32).astype(np.float64)
    c2 = 2.0 * G.lse_c(np.asarray(sizes, np.int64))
    per_score = c2 + np.spacing((np.abs(o) + c2).astype(np.float32)).astype(np.float64)
    partial = float(old) + np.cumsum(-o)
    R = float(partial[-1]) if len(o) else float(old)
    acc = float(per_score.sum())
    M = (max([abs(float(old))] + [abs(float(p)) for p in partial]) + acc) * (1.0 + len(o) * 2.0 ** -23)   # (+ the roundings themselves)
    return R, acc + len(o) * 0.5 * float(np.spacing(np.float32(M)))
