"""tools/latmbr_cpu_baseline.cc - the one-thread host program tools/lattice_mbr_rate.py times next to the device call -
against the line-by-line restatement (latmbr_restatement.py) on the generator set: the program is a second implementation
in another language with the same libm underneath, and every output is compared bit for bit.  No device."""
import numpy as np
import pytest

from conftest import pkg

import latmbr_cases as Cs
import latmbr_restatement as R


@pytest.fixture(scope="module")
def rate(tmp_path_factory):
    import tools.lattice_mbr_rate as rate
    d = str(tmp_path_factory.mktemp("latmbr_cpu"))
    return rate, rate.cpu_baseline(d), d


def test_generator_set_bit_for_bit(rate):
    rate, exe, d = rate
    clats, csrs, hyps, wants = Cs.generator_set()
    got, _ = rate.run_cpu(exe, rate.pack(csrs, [Cs.IDENTITY], [[h] for h in hyps], True), d)
    for i, w in enumerate(wants):
        R.assert_same(dict(got[i][0], bayes_risk=np.float32(got[i][0]["bayes_risk"])), w, i)
        assert got[i][0]["bayes_risk"] == w["bayes_risk_double"], i
    assert sorted(set(w["iterations"] for w in wants))[:3] == [1, 2, 3]


def test_points_given_hypotheses_and_map(rate):
    """Three score points at once, and do_mbr = 0 with hypotheses that are not paths of the lattice."""
    rate, exe, d = rate
    api = pkg("api")
    clats, csrs, hyps, wants = Cs.generator_set()
    points = [api.score_point(inv_acoustic_scale=7.0, word_ins_penalty=0.5), api.score_point(lm_scale=0.5, word_ins_penalty=-1.0), Cs.IDENTITY]
    pick = [2, 5, 14, 17]
    sub = [csrs[i] for i in pick]
    hy = [[R.best_path_words(L, *pt) for pt in points] for L in sub]
    got, _ = rate.run_cpu(exe, rate.pack(sub, points, hy, True), d)
    for k, L in enumerate(sub):
        for p, pt in enumerate(points):
            R.assert_same(dict(got[k][p], bayes_risk=np.float32(got[k][p]["bayes_risk"])), R.mbr(L, pt[0], pt[1], hy[k][p], True), (k, p))
    given = [[[3, 1, 4, 1, 5]], [[]], [[9, 9]], [[2] * 40]]
    got, _ = rate.run_cpu(exe, rate.pack(sub, [Cs.IDENTITY], given, False), d)
    for k, L in enumerate(sub):
        w = R.mbr(L, Cs.IDENTITY[0], Cs.IDENTITY[1], given[k][0], False)
        R.assert_same(dict(got[k][0], bayes_risk=np.float32(got[k][0]["bayes_risk"])), w, k)
        assert w["iterations"] == 1 and w["words"].tolist() == given[k][0]


def test_refuses_what_it_does_not_take(rate):
    rate, exe, d = rate
    api = pkg("api")
    ok = api.compact_lattice_mbr_prepare(Cs.two_paths())
    nxt = ok["arc_nextstate"].copy()
    nxt[1] = 1
    with pytest.raises(ValueError, match="arc 1 is not forward"):
        rate.run_cpu(exe, rate.pack([dict(ok, arc_nextstate=nxt)], [Cs.IDENTITY], [[[1]]]), d)
    g = ok["arc_graph"].copy()
    g[0] = np.inf
    with pytest.raises(ValueError, match="state 1: alpha = -inf"):
        rate.run_cpu(exe, rate.pack([dict(ok, arc_graph=g)], [Cs.IDENTITY], [[[1]]]), d)
    data, n, K = rate.pack([ok], [Cs.IDENTITY], [[[1]]])
    with pytest.raises(ValueError, match="does not match its header"):
        rate.run_cpu(exe, (data[:-4], n, K), d)
