"""CPU: tests/lda_restatement.py against exactly rounded sums, within the bound tests/lda_cases.py derives; the rational and
the fsum forms of the exact sums agree; Read(Write(acc)) returns acc up to the float casts of the file."""
from fractions import Fraction

import numpy as np
import pytest

import lda_cases as C
import lda_restatement as L
import mllt_restatement as M


@pytest.mark.parametrize("dim,n", [(1, 5), (3, 300), (5, 2 * C.CHUNK + 1), (17, 257), (40, 120)])
def test_restatement_within_the_bound(dim, n):
    c = C.kernel_case(dim, n, 100 * dim + n)
    x, w, cls = C.items_of(c["feats"], c["ent"])
    assert len(w) == n and C.EMPTY_CLASS not in set(cls.tolist())
    acc = C.restate(c["feats"], c["ent"], c["num_classes"])
    print("D", dim, "n", n, "restatement worst error / bound", C.check_bound(acc, x, w, cls, 7, "restatement"))
    assert not acc["first"][C.EMPTY_CLASS].any() and acc["zero"][C.EMPTY_CLASS] == 0.0
    # the counts: every order of these weights is exact, so the restatement's count IS the exact sum
    assert C.zero_is_exact(w)
    for k in range(c["num_classes"]):
        assert Fraction(float(acc["zero"][k])) == sum((Fraction(float(v)) for v in w[cls == k]), Fraction(0))


def test_rational_and_fsum_sums_agree():
    c = C.kernel_case(4, 90, 5)
    x, w, cls = C.items_of(c["feats"], c["ent"])
    sp = C.second_picks(4, 0)
    assert len(sp) == 10
    for (s, m), (rs, rm) in zip(C.exact_second(x, w, sp), C.exact_second(x, w, sp, rational=True)):
        assert s == float(rs) and m == float(rm)                         # float(Fraction) rounds once, as fsum does
    fp = C.first_picks(4, c["num_classes"], 0)
    assert len(fp) == 5 * 5
    for (s, m, n), (rs, rm, rn) in zip(C.exact_first(x, w, cls, fp), C.exact_first(x, w, cls, fp, rational=True)):
        assert s == float(rs) and m == float(rm) and n == rn


def test_dspr_is_the_packed_lower_update():
    rng = np.random.default_rng(2)
    x = rng.standard_normal(6)
    ap = np.zeros(21)
    L.dspr(ap, 0.75, x)
    r, c = np.tril_indices(6)
    assert np.array_equal(ap, x[c] * (0.75 * x[r]))


def test_acc_lda_loop_counts_and_init():
    """Init at the first utterance that has posteriors, even one whose posterior has the wrong length; both mismatches fail."""
    tid2pdf = np.array([-1, 0, 0, 1, 2], np.int32)
    f = lambda t, d: np.ones((t, d), np.float32)
    post = lambda t: [[(1 + i % 4, 1.0)] for i in range(t)]
    utts = [(f(3, 2), None), (f(4, 2), post(3)), (f(2, 3), post(2)), (f(5, 2), post(5)), (f(0, 2), [])]
    acc, done, fail = L.acc_lda(3, tid2pdf, utts, 0.0)
    assert (done, fail) == (2, 3) and acc["dim"] == 2 and acc["num_classes"] == 3
    assert acc["zero"].tolist() == [3.0, 1.0, 1.0] and acc["second"].tolist() == [5.0, 5.0, 5.0]
    acc, done, fail = L.acc_lda(3, tid2pdf, [(f(3, 2), None)], 0.0)
    assert (done, fail, acc["dim"], acc["num_classes"]) == (0, 1, 0, 0)
    # pruning at 4.0: every survivor is +-4; the draws are counted
    M.srand(3)
    before = M.DRAWS[0]
    trace = []
    acc, _, _ = L.acc_lda(3, tid2pdf, [(f(40, 2), [[(1 + i % 4, 0.5 if i % 3 else -0.5)] for i in range(40)])], 4.0, trace=trace)
    assert M.DRAWS[0] - before == 40 and set(np.abs(np.asarray(trace)[:, 1]).tolist()) <= {0.0, 4.0}
    assert acc["zero"].sum() == float(np.asarray(trace)[:, 1].astype(np.float64).sum())


@pytest.mark.parametrize("dim,nc", [(1, 1), (4, 3), (13, 5)])
def test_read_of_write(dim, nc):
    """Write casts the counts and rows to float and the mangled matrix to float; Read demangles from those floats.  So
    zero and first come back within 2^-24 relative, and second within
        2^-24 |mangled| + 5 2^-24 sum_c |first_c[a] first_c[b] / zero_c|
    (the float cast of the mangled value; first_c[a], first_c[b] and zero_c each within 2^-24, their product and quotient
    to first order 3 2^-24, the rest covers the second-order terms and the double roundings)."""
    rng = np.random.default_rng(dim)
    acc = L.init(L.empty(), nc, dim)
    n = 50
    for i in range(n):
        L.accumulate(acc, rng.standard_normal(dim).astype(np.float32) * 3 + 1, int(rng.integers(0, nc)) if i else nc - 1, 0.5 + rng.random())
    if nc > 1:
        acc["zero"][0], acc["first"][0] = 0.0, 0.0                       # a class without a count is not demangled
    back = L.read_of_write(acc)
    u = 2.0 ** -24
    assert (np.abs(back["zero"] - acc["zero"]) <= u * np.abs(acc["zero"])).all()
    assert (np.abs(back["first"] - acc["first"]) <= u * np.abs(acc["first"])).all()
    r, c = np.tril_indices(dim)
    spread = sum(np.abs(acc["first"][k][r] * acc["first"][k][c] / acc["zero"][k]) for k in range(nc) if acc["zero"][k] != 0)
    assert (np.abs(back["second"] - acc["second"]) <= u * np.abs(L.mangled(acc)) + 5 * u * spread).all()
    once = {k: np.array(back[k]) for k in ("zero", "first", "second")}
    again = L.read_of_write(acc, back)                                   # add = true: the same values once more, exactly doubled
    assert again is back and all(np.array_equal(again[k], 2 * once[k]) for k in once)
    with pytest.raises(ValueError, match="dimension or classes count mismatch, %d, %d,  vs. %d, %d" % (nc + 1, dim, nc, dim)):
        L.read_of_write(acc, L.init(L.empty(), nc + 1, dim))
