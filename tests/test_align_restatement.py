"""CPU: the two modes of tests/align_restatement.py against each other.  "reference" is FasterDecoder as it is written (list
order, running cutoff, first-arrival ties); "library" is the rule kh_align_compiled implements (the frame's final cutoff,
lowest arc position).  On every committed case they must give the same status, alignment and words, and no equal-cost
comparison may occur in either - otherwise the GPU tests, which hold the device to library mode, would not say anything
about the reference.  The size of the deliberate difference is measured and printed, not asserted (DESIGN.md has the
counts)."""
import pytest

import align_cases as C
import align_restatement as R

CASES = C.hand_cases() + C.generated_cases()


def both(c, beam=None, retry_beam=None, min_active=None):
    kw = dict(beam=c["beam"] if beam is None else beam, retry_beam=c["retry_beam"] if retry_beam is None else retry_beam,
              min_active=c["min_active"] if min_active is None else min_active)
    return (R.align(c["graph"], c["loglikes"], c["tid2pdf"], mode="library", **kw),
            R.align(c["graph"], c["loglikes"], c["tid2pdf"], mode="reference", **kw))


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_modes_agree_without_ties(c):
    lib, ref = both(c)
    assert not lib["had_tie"] and not ref["had_tie"]
    assert lib["status"] == ref["status"] and lib["retried"] == ref["retried"]
    assert lib["alignment"] == ref["alignment"] and lib["words"] == ref["words"]
    if lib["status"] == R.DONE and not ref["order_sensitive"]:
        # with no token above the frame's final cutoff the two searches hold the same tokens: everything is equal
        assert lib["cost"] == ref["cost"] and lib["path"] == ref["path"] and lib["weight"] == ref["weight"]


def test_every_cutoff_branch_and_a_retry_are_among_the_cases():
    seen = dict(cut_inf=0, cut_select=0, cut_beam=0)
    retried = 0
    for c in CASES:
        lib = R.align(c["graph"], c["loglikes"], c["tid2pdf"], c["beam"], c["retry_beam"], "library", c["min_active"])
        for k in seen:
            seen[k] += lib.get(k, 0)
        retried += lib["retried"]
    assert all(v > 0 for v in seen.values()), seen
    assert retried > 0


def test_the_tie_rule():
    """Equal costs go to the lowest arc position, equal final totals to the lowest state (library mode only: the
    reference's choice depends on its list order)."""
    c = C.tie_case()
    r = R.align(c["graph"], c["loglikes"], c["tid2pdf"], c["beam"], mode="library")
    assert r["had_tie"] and r["status"] == R.DONE
    # frame 3 into state 2: over 0 -> 1 -> 1 -> 2 and over 0 -> 2 -> 2 -> 2 both cost 4.5; arc (1, 2) lies before (2, 2)
    assert r["alignment"] == [1, 1, 1] and r["words"] == [51, 53, 55]
    # the eps arcs into the final states 3 and 4 give the same total 5.75: state 3
    assert r["best_state"] == 3 and r["cost"] == 5.75


def test_float_rounded_selection():
    """min_active's cutoff is taken among float-rounded costs: the token at 3 + 2^-23 (float 3) propagates, the one at the
    cutoff 3 + 2^-22 does not."""
    c = C.float_rounding_case()
    lib, ref = both(c)
    assert lib["cut_select"] == 1 and lib["status"] == R.DONE and lib["alignment"] == ref["alignment"]
    wide, _ = both(c, beam=50.0)
    assert wide["cut_select"] == 0


def test_negative_eps_cycle_ends_at_the_bound():
    c = C.negative_eps_cycle_case()
    assert R.decode_library(c["graph"], c["loglikes"], c["tid2pdf"], c["beam"])["status"] == R.BOUND


def test_refusals():
    c = CASES[0]
    for beam, retry in ((0.0, 0.0), (-1.0, 0.0), (10.0, 10.0), (10.0, 5.0)):
        with pytest.raises(ValueError):
            R.align(c["graph"], c["loglikes"], c["tid2pdf"], beam, retry)


def test_measure_the_deliberate_difference():
    """Over 200 generated utterances at min_active 20: how many had, in reference mode, a token at or above its frame's final
    cutoff, and how many of those aligned differently in library mode.  Printed (pytest -s); DESIGN.md records the counts."""
    for beam in (10.0, 200.0):
        sensitive = changed = ties = 0
        for seed in range(2000, 2200):
            c = C.generate(seed, n_words=2 + seed % 4, n_phones=8, max_prons=3, pad_to=40 + seed % 50)
            lib, ref = both(c, beam=beam, retry_beam=0.0, min_active=20)
            ties += lib["had_tie"] or ref["had_tie"]
            if ref["order_sensitive"]:
                sensitive += 1
                changed += (lib["status"], lib["alignment"], lib["words"]) != (ref["status"], ref["alignment"], ref["words"])
        print("beam %g: %d of 200 utterances order-sensitive, %d of them aligned differently, %d with a tie" % (beam, sensitive, changed, ties))
