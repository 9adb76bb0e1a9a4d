"""tools/align_cpu_baseline.cc - the one-thread host program tools/align_rate.py times next to the device call - compiles and
equals library mode of tests/align_restatement.py bit for bit on the hand cases and 50 generated ones: status, the double
total cost, the best final state, every path arc's labels and two floats (alignment and words are the path's labels).  A
second implementation of the library's rule in another language, arcs walked forward instead of by destination.  No device."""
import numpy as np
import pytest

import align_cases as C
import align_restatement as R


@pytest.fixture(scope="module")
def rate(tmp_path_factory):
    import tools.align_rate as rate
    d = str(tmp_path_factory.mktemp("align_cpu"))
    return rate, rate.cpu_baseline(d), d


def compare(rate, cases, beam, min_active, room=400):
    rate, exe, d = rate
    got, _ = rate.run_cpu(exe, cases, beam, min_active, d, room=room)
    assert len(got) == len(cases)
    for c, g in zip(cases, got):
        w = R.decode_library(c["graph"], c["loglikes"], c["tid2pdf"], beam, min_active)
        assert g["status"] == w["status"], c["name"]
        if w["status"] == R.DONE:
            assert g["cost"] == w["cost"] and g["best_state"] == w["best_state"], c["name"]
            assert g["path"] == [tuple(x) for x in w["path"]], c["name"]
            assert [a[0] for a in g["path"] if a[0]] == w["alignment"] and [a[1] for a in g["path"] if a[1]] == w["words"]


def test_hand_cases(rate):
    cases = [c for c in C.hand_cases() if c["name"] != "float_rounding"]
    compare(rate, cases, 200.0, 20)
    compare(rate, [C.float_rounding_case()], 1e-7, 2)
    compare(rate, [C.tie_case()], 200.0, 20)
    compare(rate, [C.negative_eps_cycle_case()], 200.0, 20)


@pytest.mark.parametrize("beam,min_active", [(200.0, 20), (8.0, 20), (4.0, 2), (2.0, 0)])
def test_generated(rate, beam, min_active):
    compare(rate, [C.generate(s, n_words=2 + s % 3, pad_to=(65 if s % 2 else 0)) for s in range(3000, 3050)], beam, min_active)


def test_needs_more_room(rate):
    r, exe, d = rate
    c = [c for c in C.hand_cases() if c["name"] == "eps_chains_T37"]
    got, _ = r.run_cpu(exe, c, 200.0, 20, d, room=2)
    w = R.decode_library(c[0]["graph"], c[0]["loglikes"], c[0]["tid2pdf"], 200.0)
    assert got[0]["status"] == R.NEEDS_ROOM and got[0]["path_len"] == len(w["path"]) and got[0]["cost"] == w["cost"]
