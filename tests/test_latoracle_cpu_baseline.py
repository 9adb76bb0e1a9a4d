"""tools/latoracle_cpu_baseline.cc - the host implementation tools/lattice_oracle_rate.py times next to the device call -
against the cell-by-cell restatement (latoracle_restatement.py): it is written in push form with back-pointers, and its
strict updates in arrival order are the project's tie rule, so every output is compared exactly.  No device."""
import numpy as np
import pytest

from conftest import pkg

import latoracle_cases
import latoracle_restatement as R

WILD = (9,)


@pytest.fixture(scope="module")
def rate(tmp_path_factory):
    import tools.lattice_oracle_rate as rate
    return rate, rate.cpu_baseline(str(tmp_path_factory.mktemp("latoracle_cpu")))


def packed(rate, csrs, refs):
    return rate.pack(csrs, [L["start"] for L in csrs], refs, WILD, [R.is_final_of(L) for L in csrs])


def assert_point_equals(got, i, p, r, what):
    assert int(got["errors"][i, p]) == r["errors"], what
    assert got["counts"][i, p].tolist() == [r["correct"], r["sub"], r["ins"], r["del"]], what
    assert got["paths"][i][p].tolist() == list(r["path_arcs"]), what
    assert int(got["final_state"][i, p]) == r["final_state"], what
    assert int(got["path_len"][i, p]) == (len(r["path_arcs"]) if r["errors"] >= 0 else -1), what


def test_hand_lattices_as_one_batch(rate):
    rate, fn = rate
    api = pkg("api")
    cases = latoracle_cases.all_cases()
    csrs = [api.compact_lattice_to_prune_csr(c[1]) for c in cases]
    got = rate.run_cpu(fn, packed(rate, csrs, [c[2] for c in cases]))
    for i, (name, clat, ref, wild, want) in enumerate(cases):
        assert_point_equals(got, i, 0, R.oracle(csrs[i], ref, WILD), name)
        assert int(got["errors"][i, 0]) == want["errors"], name


def test_random_lattices_and_masks_of_two_words(rate):
    """Random lattices full of ties (3 words, epsilon, the wildcard; some with the start state behind state 0) against
    references of 0 to 70 words, unmasked and under 65 random mask points (two words per arc and state)."""
    rate, fn = rate
    api = pkg("api")
    clats, refs = [], []
    for k, n_ref in enumerate((0, 1, 2, 5, 9, 70) * 4):
        rng = np.random.default_rng(8100 + k)
        n = int(rng.integers(2, 25))
        clats.append(R.random_word_clat(rng, n, start=int(rng.integers(0, n // 2 + 1)) if k % 5 == 4 else 0, last_final=bool(rng.random() < 0.9)))
        refs.append([int(x) for x in rng.choice([1, 2, 3, 9], size=n_ref, p=[0.3, 0.3, 0.3, 0.1])])
    csrs = [api.compact_lattice_to_prune_csr(c) for c in clats]
    B = packed(rate, csrs, refs)
    got = rate.run_cpu(fn, B)
    for i, (L, ref) in enumerate(zip(csrs, refs)):
        assert_point_equals(got, i, 0, R.oracle(L, ref, WILD), i)
    K = 65
    rng = np.random.default_rng(8200)
    ak = rng.random((len(B["label"]), K)) < np.linspace(0.5, 1.0, K)
    fk = rng.random((int(B["soff"][-1]), K)) < np.linspace(0.6, 1.0, K)
    got = rate.run_cpu(fn, B, K, api._mask_words(ak, K), api._mask_words(fk, K))
    a0 = 0
    for i, (L, ref) in enumerate(zip(csrs, refs)):
        s0, na = int(B["soff"][i]), len(L["arc_label"])
        for p in (0, 1, 31, 63, 64):
            r = R.oracle(L, ref, WILD, arc_keep=ak[a0:a0 + na, p], final_keep=fk[s0:s0 + L["n_states"], p])
            assert_point_equals(got, i, p, r, (i, p))
        a0 += na
    assert (got["errors"] == -1).any() and (got["errors"] >= 0).any()


def test_refuses_what_it_does_not_take(rate):
    rate, fn = rate
    api = pkg("api")
    csr = api.compact_lattice_to_prune_csr(latoracle_cases.chain([1, 2]))
    with pytest.raises(ValueError):
        rate.run_cpu(fn, packed(rate, [dict(csr, arc_nextstate=np.array([1, 1], np.int32))], [[1]]))
    with pytest.raises(ValueError):
        rate.run_cpu(fn, packed(rate, [dict(csr, start=3)], [[1]]))
