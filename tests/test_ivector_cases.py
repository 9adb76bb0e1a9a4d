"""CPU: the case table of tests/ivector_cases.py is what it says.  For every case the oracle runs, the inputs are separated
(no near-tie of the num_gselect-th posterior, no posterior near min_post: both margins >= 20 x the float error of the
scores), and each entry of the case's "reaches" holds for the constants of csrc/kh_ivector.hip as the source states them
today - so the table cannot drift from the kernel unnoticed."""
import numpy as np
import pytest

import ivector_cases as C
from oracle import ivector_oracle as IO


@pytest.fixture(scope="module")
def K():
    return C.kernel_constants()


def test_kernel_constants_are_the_ones_the_table_was_written_for(K):
    assert (K["kGemmK"], K["kGemmN"], K["kGemmM"], K["kLinItem"], K["kSortChunk"], K["kMaxPerLane"], K["kWChunk"]) == (16, 128, 64, 512, 4096, 32, 16)
    assert K["kMaxGselect"] == 16 and K["kLdsLimit"] == 65536 and K["kJacobiPairs"] * 2 == 256 and K["kEigSlots"] == 16


@pytest.mark.parametrize("name", list(C.CASES))
def test_oracle_runs_and_inputs_are_separated(name):
    c = C.CASES[name]
    runs = C.oracle_runs(name)
    assert [r["label"] for r in runs] == (["plain", "adapt_round0", "adapt_round1"] if c["adapt"] else ["plain"])
    for r in runs:
        m = r["model"]
        for u, (rows, st), tr in zip(r["utts"], r["want"], r["traces"]):
            assert rows.shape == (len(u), c["S"]) and np.isfinite(rows).all() and np.isfinite(st["quad"]).all()
            delta, sel, prune = C.separation(tr, m)
            print("%s %s T=%d: delta %.2e selection margin %.2e min_post margin %.2e" % (name, r["label"], len(u), delta, sel, prune))
            assert sel >= C.MARGIN_FACTOR * delta, (r["label"], sel, delta)
            assert prune >= C.MARGIN_FACTOR * delta, (r["label"], prune, delta)
            # the float64 recomputation selects and prunes as the float32 oracle does
            assert [[g for g, _ in e] for e in tr["post32"]] == [[g for g, _ in e] for e in tr["post64"]]
            # the trace restates IO.extract: its counts rebuild the oracle's quadratic term
            if r["states_in"][0] is None and m["max_count"] == 0.0:
                U, _ = IO.derived(m)
                rr, cc = IO.packed_index(c["S"])
                Q = np.zeros((c["S"], c["S"]))
                Q[rr, cc] = C.counts(tr["post32"], c["I"]) @ U
                np.testing.assert_allclose(np.eye(c["S"]) + Q + np.tril(Q, -1).T, st["quad"], rtol=1e-9, atol=1e-9)


def test_count_tolerance_is_four_times_the_measured_float_difference():
    worst = 0.0
    for name in C.CASES:
        for r in C.oracle_runs(name):
            for tr in r["traces"]:
                c32, c64 = C.counts(tr["post32"], C.CASES[name]["I"]), C.counts(tr["post64"], C.CASES[name]["I"])
                assert np.array_equal(c32 != 0, c64 != 0)
                nz = c64 != 0
                worst = max(worst, float((np.abs(c32 - c64)[nz] / c64[nz]).max()))
    print("largest relative difference of the counts, float32 vs float64 posteriors: %.3e" % worst)
    assert C.COUNT_RTOL / 4 * 0.5 <= worst <= C.COUNT_RTOL / 4 * 1.05       # the bound is 4 x what is measured here, neither less nor much more


@pytest.mark.parametrize("name", list(C.CASES))
def test_case_reaches_what_it_claims(name, K):
    f = C.facts(name, K)
    for key, want in C.CASES[name]["reaches"].items():
        assert f[key] == want, (name, key, f[key], want)


def test_every_branch_of_the_issue_has_a_case(K):
    """Each gap the table was written to close is reached by at least one case (with the constants of today's source)."""
    F = {n: C.facts(n, K) for n in C.CASES}
    some = lambda pred: [n for n in C.CASES if pred(F[n], C.CASES[n])]
    assert some(lambda f, c: f["k_tail"] and f["wide"] and f["b_edge_mixed"])            # IvGemmF64Kernel: K-tail + mixed B row under `wide`
    assert some(lambda f, c: f["wide"] and f["a_quad_partial"])                          # an A quad straddling K under `wide`
    assert some(lambda f, c: f["k_tail"] and not f["wide"] and c["I"] % 2 == 1)          # scalar: odd K
    assert some(lambda f, c: f["k_tail"] and not f["wide"] and c["I"] % 2 == 0)          # scalar: odd N only
    assert some(lambda f, c: not f["k_tail"] and not f["wide"])
    assert {F[n]["spmv_tail"] for n in C.CASES} == {0, 1, 2, 3} and some(lambda f, c: f["spmv_trips"] == 0)
    assert some(lambda f, c: c["S"] == 64) and some(lambda f, c: c["S"] == 65)
    assert some(lambda f, c: f["per_lane"] > 1 and f["ragged_lanes"]) and some(lambda f, c: f["per_lane_is_max"])
    assert some(lambda f, c: f["s_w_full"] and f["period_chunks"] > 1 and not c["overrides"].get("greedy_most_recent"))
    assert some(lambda f, c: f["gselect_padding"]) and some(lambda f, c: c["I"] == 1)
    assert some(lambda f, c: f["sort_blocks"] >= 2 and f["items_min"] >= 2)
    assert some(lambda f, c: [512, 1] in f.get("chunk_item_sizes", []) and [512, 512] in f.get("chunk_item_sizes", []))
    assert some(lambda f, c: f["base_is_max"] and f["stride_over_base"])
    assert some(lambda f, c: f["solve_fits"] and not f["solve_fits_plus_one"])
    assert some(lambda f, c: f["acc_fits"] and not f["acc_fits_plus_one"] and c["streams"])
    # the streams-only over-limit shape: create() accepts it, the streams kernel does not fit
    o = C.STREAMS_OVER
    need = C.lds_need(K, o["feat"], o["S"], o["num_gselect"])
    assert max(need["lin"], need["solve"]) <= K["kLdsLimit"] < need["stream"]
    assert need["stream"] - K["kStreamStaticLds"] == 67640
    # the state chain covers the cases the adaptation-state branches were asked on; the streams theirs
    assert [n for n in C.CASES if C.CASES[n]["adapt"]] == ["odd_dims", "odd_k", "two_waves"]
    assert {"odd_dims", "multi_block"} <= {n for n in C.CASES if C.CASES[n]["streams"]}
    for n in ("odd_dims", "odd_k", "two_waves"):          # max_count = 3 rescales the prior in every one of them ...
        r0 = C.oracle_runs(n)[1]
        assert max(st["num_frames"] for _, st in r0["want"]) > 3.0
    r0 = C.oracle_runs("odd_dims")[1]                     # ... and LimitFrames scales the statistics between the rounds
    assert max(st["num_frames"] for _, st in r0["want"]) > C.MAX_REMEMBERED * r0["model"]["posterior_scale"]


@pytest.mark.parametrize("name", list(C.FALLBACK))
def test_oracle_falls_back_to_the_exact_solve_at_odd_dimensions(name):
    f = C.FALLBACK[name]
    assert f["S"] % 2 == 1 and len(f["lengths"]) <= 8
    want, n_exact = C.fallback_oracle(name)
    print("%s: %d exact solves" % (name, n_exact))
    assert n_exact >= f["min_exact"]
    assert all(np.isfinite(w).all() for w in want)
