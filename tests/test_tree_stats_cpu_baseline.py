"""tools/tree_stats_cpu_baseline.cc - the one-thread host program tools/tree_stats_rate.py times next to the device route -
compiles, also under -fsanitize=address,undefined (a stand-alone program: no report, the same outputs), and equals
tests/tree_stats_restatement.py bit for bit on small cases, the order-sensitive ones included, with its events in std::map
order.  The generated set of the rate tool has the shape its documentation states.  No device."""
import subprocess

import numpy as np
import pytest

import tree_stats_cases as C
import tree_stats_restatement as R

SAN = ["-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


@pytest.fixture(scope="module")
def rate(tmp_path_factory):
    import tools.tree_stats_rate as rate
    d = tmp_path_factory.mktemp("tree_cpu")
    san = d / "san"
    san.mkdir()
    return rate, rate.cpu_baseline(str(d)), rate.cpu_baseline(str(san), SAN), str(d)


def events_for(E):
    return [((-1, e % 3), (0, e // 3), (1, 7 - e)) if e % 2 else ((-1, e % 3), (1, e)) for e in range(E)]


@pytest.mark.parametrize("name", ["edges", "alone", "among_others"])
def test_baseline_equals_the_restatement(rate, name):
    rate, exe, exe_san, d = rate
    rng = np.random.default_rng(17)
    feats, fe, E = C.kernel_case(rng, 9, C.edge_runs(8), unused=6) if name == "edges" else C.order_cases(rng)[name]
    events = events_for(E)
    got, ms = rate.run_cpu(exe, feats, fe, events, d)
    count, stats = R.add_stats(feats, fe, E)
    met = [e for e in range(E) if (fe == e).any()]
    assert [ev for ev, _, _ in got] == sorted(events[e] for e in met) and ms >= 0
    for ev, c, s in got:
        e = events.index(ev)
        assert c == count[e] and C.same_bits(s, stats[e]), ev
    san, _ = rate.run_cpu(exe_san, feats, fe, events, d)         # the sanitized build: the same bytes out
    assert len(san) == len(got) and all(a[0] == b[0] and a[1] == b[1] and C.same_bits(a[2], b[2]) for a, b in zip(got, san))


def test_baseline_refuses_bad_input(rate, tmp_path):
    rate, exe, exe_san, d = rate
    bad = tmp_path / "bad.bin"
    bad.write_bytes(b"\0" * 12)
    p = subprocess.run([exe_san, str(bad), str(tmp_path / "o")], capture_output=True, text=True)
    assert p.returncode == 2 and "short input" in p.stderr
    with pytest.raises(ValueError, match="inconsistent offsets"):
        rate.run_cpu(exe_san, np.zeros((2, 3), np.float32), np.array([0, 1], np.int32), [((0, 1),)], d)      # event 1 of 1


def test_generated_set_is_recipe_like(rate):
    rate = rate[0]
    feats, fe, events = rate.make_set(20000, 4, 4000)
    runs = np.bincount(fe, minlength=len(events))
    assert feats.shape == (20000, 4) and feats.dtype == np.float32 and len(set(events)) == len(events) == 4005
    assert 0.18 < runs[:5].sum() / 20000 < 0.22 and (runs > 0).sum() > 2000 and runs[5:].max() < runs[:5].min()
    assert all(len(e) == 2 for e in events[:5]) and all(len(e) == 4 and e == tuple(sorted(e)) for e in events[5:])
