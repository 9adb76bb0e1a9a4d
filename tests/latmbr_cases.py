"""Test helper: the lattices of the minimum-Bayes-risk tests - hand lattices and a small seeded generator - in the
CompactLattice dict layout, with transition-id strings whose lengths give every state one time (CompactLatticeStateTimes
asserts that).  The restatement's answers on the generator set are computed once per process (generator_set)."""
import functools

import numpy as np

from latbest_restatement import make_clat

f32 = np.float32
IDENTITY = (np.array([1.0, 0.0, 0.0, 1.0]), f32(0.0))


def _string(n):
    return list(range(1, n + 1))


def chain(words, frames=None, weights=None):
    """One path: state i -> i + 1 with words[i]; the last state final with weight One."""
    n = len(words)
    frames = [2 + (i % 3) for i in range(n)] if frames is None else frames
    weights = [(0.5 * (i % 4), 0.25 * (i % 3)) for i in range(n)] if weights is None else weights
    arcs = [(i, i + 1, int(words[i]), weights[i][0], weights[i][1], _string(frames[i])) for i in range(n)]
    return make_clat(n + 1, arcs, {n: (0.0, 0.0, [])})


def two_paths(g1=1.0, g2=2.25):
    """1 2 4 and 1 3 4: the paths differ in the second word."""
    arcs = [(0, 1, 1, 0.5, 0.25, _string(3)), (1, 2, 2, g1, 0.5, _string(4)), (1, 2, 3, g2, 0.125, _string(4)),
            (2, 3, 4, 0.75, 1.0, _string(2))]
    return make_clat(4, arcs, {3: (0.0, 0.0, [])})


def confusion_network(seed, n_bins=6, max_alt=4):
    """Parallel arcs between consecutive states, distinct words within a bin (word 0 among them in some)."""
    rng = np.random.default_rng(seed)
    arcs = []
    for b in range(n_bins):
        k = int(rng.integers(1, max_alt + 1))
        words = rng.choice(np.arange(0 if b % 2 else 1, 9), size=k, replace=False)
        for w in words:
            arcs.append((b, b + 1, int(w), float(rng.uniform(0, 3)), float(rng.uniform(0, 3)), _string(3)))
    return make_clat(n_bins + 1, arcs, {n_bins: (0.0, 0.0, [])})


def fan_in(n_in=70):
    """A state with n_in incoming arcs: more than one wave's worth of an incoming list."""
    arcs = [(0, 1, 1 + (i % 7), 0.125 * (i % 9), 0.0625 * (i % 5), _string(2)) for i in range(n_in)]
    arcs += [(1, 2, 3, 0.5, 0.5, _string(3)), (1, 2, 0, 1.5, 0.25, _string(3))]
    return make_clat(3, arcs, {2: (0.0, 0.0, [])})


def shortcut_words(n_words=40):
    return [1] + [2 + (i % 5) for i in range(n_words - 1)]


def shortcut(n_words=40):
    """A chain of n_words words and one arc from the first state to the last that carries the chain's first word, which no
    other arc carries: against
    the chain's words that arc matches at q = 2 and is strictly ahead from there on (a3 < a1: no tie that :175 would give to
    case 1), so its row is one run of b_arc == 3 over q = 3..Q, across the boundary between lanes 63 and 64."""
    c = chain(shortcut_words(n_words), frames=[2] * n_words)
    arcs = [(int(s), int(d), int(w), float(g), float(a), list(x)) for s, d, w, g, a, x in
            zip(c["arc_src"], c["arc_dst"], c["arc_label"], c["arc_g"], c["arc_a"], c["arc_string"])]
    arcs.append((0, n_words, 1, 3.0, 1.0, _string(2 * n_words)))
    arcs.sort(key=lambda x: x[0])
    return make_clat(n_words + 1, arcs, {n_words: (0.0, 0.0, [])})


def all_eps(n=3):
    """Every arc carries label 0: the best path has no words, Q = 1."""
    arcs = [(i, i + 1, 0, 0.5, 0.5, _string(2)) for i in range(n)] + [(0, 1, 0, 1.0, 0.25, _string(2))]
    arcs.sort(key=lambda x: x[0])
    return make_clat(n + 1, arcs, {n: (0.0, 0.0, [])})


def several_finals():
    """Three final states with weights and strings: CreateSuperFinal adds state 4 and three epsilon arcs."""
    arcs = [(0, 1, 1, 0.5, 0.5, _string(2)), (0, 2, 2, 1.0, 0.25, _string(3)), (1, 3, 3, 0.25, 0.5, _string(4)),
            (2, 3, 4, 0.5, 1.5, _string(3))]
    return make_clat(4, arcs, {1: (0.5, 0.25, _string(5)), 2: (1.0, 0.0, _string(4)), 3: (0.125, 0.5, _string(1))})


def unsorted():
    """several_finals' shape in a numbering that is not sorted: start state 2, an arc 3 -> 1."""
    arcs = [(2, 3, 1, 0.5, 0.5, _string(2)), (2, 0, 2, 1.0, 0.25, _string(3)), (3, 1, 3, 0.25, 0.5, _string(4)),
            (0, 1, 4, 0.5, 1.5, _string(3))]
    return make_clat(4, arcs, {1: (0.0, 0.0, [])}, start=2)


def random_mbr_clat(seed, n_states, max_out=4, p_next=0.7, n_words=5, p_eps=0.1, spread=3.0, finals=1):
    """A random top-sorted CompactLattice of n_states <= 40 states with at most max_out arcs out of a state: every state is
    reachable and reaches the last one, weights are uniform in [0, spread), string lengths follow per-state times."""
    rng = np.random.default_rng(seed)
    t = np.concatenate([[0], np.cumsum(rng.integers(1, 5, size=n_states - 1))])
    arcs = []
    for s in range(n_states - 1):
        dsts = {s + 1}                                           # (so every state is reachable and reaches the last)
        for _ in range(int(rng.integers(0, max_out))):
            dsts.add(int(min(n_states - 1, s + 1 + (0 if rng.random() < p_next else int(rng.integers(1, 4))))))
        used = 0
        for d in sorted(dsts):
            for _ in range(1 if used + 1 >= max_out or rng.random() < 0.6 else 2):
                if used >= max_out:
                    break
                w = 0 if rng.random() < p_eps else int(rng.integers(1, n_words + 1))
                arcs.append((s, d, w, float(f32(rng.uniform(0, spread))), float(f32(rng.uniform(0, spread))), _string(int(t[d] - t[s]))))
                used += 1
    fin = {n_states - 1: (0.0, 0.0, [])}
    if finals > 1:
        end = int(t[-1]) + 2
        fin = {n_states - 1: (float(f32(rng.uniform(0, 1))), 0.5, _string(end - int(t[-1])))}
        for s in rng.choice(np.arange(1, n_states - 1), size=finals - 1, replace=False):
            fin[int(s)] = (float(f32(rng.uniform(0, 2))), 0.25, _string(end - int(t[int(s)])))
    return make_clat(n_states, arcs, fin)


# The generator set: (seed, n_states, p_next, finals, spread of the weights).  Chosen by running the restatement alone over
# seeds 7000..7019 and 7100..7129 and keeping a set on which it meets every condition tests/test_lattice_mbr.py states (gamma
# rows sum to 1, L does not increase, times ordered), with eight lattices of >= 2 iterations (two of them 3), runs of
# b_arc == 3 of length >= 2 in all of them, and three whose initial hypothesis has 32, 35 and 31 (33 and more after the
# first update) words, so that Q > 64.
GENERATOR_SET = [(7000 + i, n, p, fin, 3.0) for i, (n, p, fin) in enumerate(
    [(5, 0.7, 1), (8, 0.7, 1), (12, 0.6, 2), (15, 0.7, 1), (20, 0.5, 1), (25, 0.7, 3), (30, 0.8, 1), (36, 0.95, 1), (38, 0.95, 1),
     (40, 0.97, 1), (40, 0.9, 2), (3, 0.7, 1), (10, 0.4, 1), (18, 0.6, 1)])] + [
    (7107, 20, 0.7, 1, 1.0), (7103, 38, 0.97, 1, 1.0), (7109, 38, 0.97, 1, 1.0), (7128, 12, 0.6, 1, 1.0), (7104, 30, 0.8, 1, 1.0),
    (7121, 38, 0.97, 1, 1.0)]


def generator_clats():
    return [random_mbr_clat(seed, n, p_next=p, finals=fin, spread=spread) for seed, n, p, fin, spread in GENERATOR_SET]


@functools.lru_cache(maxsize=None)
def generator_set():
    """(clats, prepared CSR dicts, initial hypotheses, the restatement's answers with do_mbr=True at the identity point),
    computed once per process.  Needs the package for compact_lattice_mbr_prepare (no device)."""
    from conftest import pkg
    import latmbr_restatement as R
    api = pkg("api")
    clats = generator_clats()
    csrs = [api.compact_lattice_mbr_prepare(c) for c in clats]
    hyps = [R.best_path_words(L, *IDENTITY) for L in csrs]
    wants = [R.mbr(L, IDENTITY[0], IDENTITY[1], h, True) for L, h in zip(csrs, hyps)]
    return clats, csrs, hyps, wants


def restated_mbr(clats, points=None, one_bests=None, do_mbr=True, workspace_limit=None):
    """api.compact_lattice_mbr's answer from the restatement alone (no device): what the tools' tests put in its place."""
    from conftest import pkg
    import latmbr_restatement as R
    api = pkg("api")
    points = [IDENTITY] if points is None else list(points)
    out = []
    for i, c in enumerate(clats):
        L = api.compact_lattice_mbr_prepare(c)
        row = []
        for scale, pen in points:
            hyp = R.best_path_words(L, scale, pen) if one_bests is None else [int(w) for w in one_bests[i]]
            r = R.mbr(L, scale, pen, hyp, do_mbr)
            row.append({k: r[k] for k in ("words", "bayes_risk", "iterations", "sausage_stats", "sausage_times", "one_best_times",
                                          "one_best_confidences")})
        out.append(row)
    return out


def small_archive():
    """Five utterances: generator lattices (one with several final states), the two-path lattice and a chain."""
    return [("utt_a", random_mbr_clat(7001, 8)), ("utt_b", random_mbr_clat(7128, 12, p_next=0.6, spread=1.0)),
            ("utt_c", random_mbr_clat(7002, 12, p_next=0.6, finals=2)), ("utt_d", two_paths()), ("utt_e", chain([3, 1, 4, 1, 5]))]


def write_lats(path, keyed):
    from conftest import pkg
    cli = pkg("kaldi_cli")
    w = cli.TableWriter("ark:" + str(path), "compact_lattice")
    for key, clat in keyed:
        w.write(key, clat)
    w.close()
    return "ark:" + str(path)
