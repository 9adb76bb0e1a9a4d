"""Test helper: the oracle path of latbin/lattice-oracle.cc for ONE top-sorted CompactLattice, ONE reference and ONE keep
mask, in plain Python, one cell at a time: the recurrence and the walk back exactly as csrc/kh_latoracle.hip states them,
and CompactLatticeDepth (lat/lattice-functions.cc:574-602) with CompactLatticeStateTimes (:69-106) line by line.  OpenFst
is absent, so the program itself cannot be compiled; this is the checker of the kernel, and tests/test_lattice_oracle.py
checks it in turn against brute force (the minimum Levenshtein distance over every complete path).

The lattice is the CSR dict api.compact_lattice_to_prune_csr returns (top-sorted, `start` in that numbering)."""
import numpy as np

from latbest_restatement import make_clat  # noqa: F401

SENT = 0x3fffffff


def map_word(w, wildcards):
    """MapWildCards lattice-oracle.cc:58-75: label 0 and the wildcards are epsilon."""
    return 0 if (int(w) == 0 or int(w) in wildcards) else int(w)


def is_final_of(L):
    """Final(s) != Weight::Zero()"""
    fg, fa = np.asarray(L["final_graph"], np.float32), np.asarray(L["final_acoustic"], np.float32)
    return ~((fg == np.inf) & (fa == np.inf))


def oracle(L, ref, wildcards=(), arc_keep=None, final_keep=None, state_keep=None, arc_frames=None, final_frames=None,
           is_final=None):
    """Returns dict(errors, correct, sub, ins, del, path_arcs = CSR arc numbers of the path, final_state, moves = the path
    from the start as (kind, arc or None, j after the move), frame_sum, R, D).  errors = -1: no path; the rest is then
    empty."""
    wildcards = set(int(w) for w in wildcards)
    n, start = int(L["n_states"]), int(L["start"])
    off, nxt = np.asarray(L["arc_offsets"], np.int64), np.asarray(L["arc_nextstate"], np.int64)
    label = [map_word(w, wildcards) for w in L["arc_label"]]
    n_arcs = len(label)
    r = [0] + [int(w) for w in ref if map_word(w, wildcards) != 0]           # r[1..R]
    R = len(r) - 1
    arc_keep = np.ones(n_arcs, bool) if arc_keep is None else np.asarray(arc_keep, bool)
    masked = final_keep is not None
    final_keep = np.ones(n, bool) if final_keep is None else np.asarray(final_keep, bool)
    state_keep = np.ones(n, bool) if state_keep is None else np.asarray(state_keep, bool)
    is_final = is_final_of(L) if is_final is None else np.asarray(is_final, bool)
    incoming = [[] for _ in range(n)]                                        # ascending arc number
    for s in range(n):
        for a in range(off[s], off[s + 1]):
            assert s < nxt[a] < n
            incoming[nxt[a]].append((a, s))
    D = [[SENT] * (R + 1) for _ in range(n)]
    for e in range(start, n):
        for j in range(R + 1):
            if e == start:
                D[e][j] = j
                continue
            v = SENT
            for a, s in incoming[e]:
                if not arc_keep[a]:
                    continue
                w = label[a]
                if w == 0:
                    v = min(v, D[s][j])
                else:
                    if j >= 1:
                        v = min(v, D[s][j - 1] + (1 if w != r[j] else 0))   # diagonal
                    v = min(v, D[s][j] + 1)                                  # insertion
            if j >= 1:
                v = min(v, D[e][j - 1] + 1)                                  # deletion
            D[e][j] = min(v, SENT)
    frame_sum = None
    if arc_frames is not None:
        frame_sum = int(sum(int(arc_frames[a]) for a in range(n_arcs) if arc_keep[a]))
        frame_sum += int(sum(int(final_frames[s]) for s in range(n) if (not masked) or (state_keep[s] and final_keep[s])))
    best, end = SENT, -1
    for f in range(n):
        if is_final[f] and final_keep[f] and D[f][R] < best:                 # the lowest-numbered state that attains it
            best, end = D[f][R], f
    if best >= SENT:
        return dict(errors=-1, correct=0, sub=0, ins=0, path_arcs=np.zeros(0, np.int64), final_state=-1, moves=[],
                    frame_sum=frame_sum, R=R, D=D, **{"del": 0})
    cnt = dict(correct=0, sub=0, ins=0)
    n_del = 0
    e, j = end, R
    arcs, moves = [], []
    while e != start:
        val = D[e][j]
        took = None
        for a, s in incoming[e]:
            if not arc_keep[a]:
                continue
            w = label[a]
            if w == 0:
                if D[s][j] == val:
                    took = ("eps", a, s, j)
            else:
                if j >= 1 and D[s][j - 1] + (1 if w != r[j] else 0) == val:
                    took = ("correct" if w == r[j] else "sub", a, s, j - 1)
                elif D[s][j] + 1 == val:
                    took = ("ins", a, s, j)
            if took:
                break
        if took:
            kind, a, s, j2 = took
            if kind != "eps":
                cnt[kind] += 1
            arcs.append(a)
            moves.append((kind, a, j))
            e, j = s, j2
        else:
            assert j >= 1 and D[e][j - 1] + 1 == val
            n_del += 1
            moves.append(("del", None, j))
            j -= 1
    while j > 0:                                                             # D[start][j > 0] is a deletion
        n_del += 1
        moves.append(("del", None, j))
        j -= 1
    arcs.reverse()
    moves.reverse()
    return dict(errors=int(best), correct=cnt["correct"], sub=cnt["sub"], ins=cnt["ins"], path_arcs=np.asarray(arcs, np.int64) - int(off[0]),
                final_state=end, moves=moves, frame_sum=frame_sum, R=R, D=D, **{"del": n_del})


def levenshtein(hyp, ref):
    prev = list(range(len(ref) + 1))
    for i, h in enumerate(hyp, 1):
        cur = [i] + [0] * len(ref)
        for j, w in enumerate(ref, 1):
            cur[j] = min(prev[j - 1] + (h != w), prev[j] + 1, cur[j - 1] + 1)
        prev = cur
    return prev[len(ref)]


def brute_force(L, ref, wildcards=(), arc_keep=None, final_keep=None):
    """The minimum Levenshtein distance over every complete path from the start state over kept arcs; -1 for none."""
    wildcards = set(int(w) for w in wildcards)
    n, start = int(L["n_states"]), int(L["start"])
    off, nxt = np.asarray(L["arc_offsets"], np.int64), np.asarray(L["arc_nextstate"], np.int64)
    refw = [int(w) for w in ref if map_word(w, wildcards) != 0]
    fin = is_final_of(L)
    best = [-1]

    def walk(s, words):
        if fin[s] and (final_keep is None or final_keep[s]):
            d = levenshtein(words, refw)
            if best[0] < 0 or d < best[0]:
                best[0] = d
        for a in range(off[s], off[s + 1]):
            if arc_keep is not None and not arc_keep[a]:
                continue
            w = map_word(L["arc_label"][a], wildcards)
            walk(int(nxt[a]), words + [w] if w else words)
    walk(start, [])
    return best[0]


def random_word_clat(rng, n_states, vocab=(0, 1, 2, 3, 9), max_out=3, p_final=0.2, max_string=3, start=0, last_final=True):
    """A random top-sorted CompactLattice over a tiny vocabulary (0 = epsilon; the tests make 9 the wildcard), so that
    equal-cost alignments are the rule.  Weights are multiples of 0.25."""
    arcs = []
    w = lambda: np.float32(0.25 * int(rng.integers(0, 24)))
    string = lambda: rng.integers(1, 50, size=int(rng.integers(0, max_string + 1)))
    for s in range(n_states - 1):
        for _ in range(int(rng.integers(1, max_out + 1))):
            d = int(min(n_states - 1, s + int(rng.geometric(0.5))))
            arcs.append((s, d, int(vocab[int(rng.integers(0, len(vocab)))]), w(), w(), string()))
    finals = {n_states - 1: (w(), w(), string())} if last_final else {}
    for s in range(n_states - 1):
        if rng.random() < p_final:
            finals[s] = (w(), w(), string())
    return make_clat(n_states, arcs, finals, start=start)


def frames_of(clat, csr):
    """arc_frames, final_frames in CSR order: the lengths of the transition-id strings."""
    af = np.asarray([len(clat["arc_string"][j]) for j in csr["perm"]], np.int32)
    ff = np.asarray([len(clat["final_string"][s]) for s in csr["state_of"]], np.int32)
    return af, ff


# ---------------------------------------------------------------- CompactLatticeDepth
def compact_lattice_state_times(clat):
    """lat/lattice-functions.cc:69-106 on a top-sorted dict lattice with start state 0."""
    num_states = int(clat["n_states"])                                       # :73
    src, dst = np.asarray(clat["arc_src"], np.int64), np.asarray(clat["arc_dst"], np.int64)
    assert np.all(dst > src) and int(clat["start"]) == 0                     # :70-72
    times = [-1] * num_states                                                # :75
    times[0] = 0                                                             # :76
    utt_len = -1                                                             # :77
    by_src = np.argsort(src, kind="stable")
    off = np.concatenate([[0], np.cumsum(np.bincount(src, minlength=num_states))])
    for state in range(num_states):                                          # :78
        cur_time = times[state]                                              # :79
        for a in by_src[off[state]:off[state + 1]]:                          # :80
            arc_len = len(clat["arc_string"][a])                             # :83
            if times[dst[a]] == -1:                                          # :84
                times[dst[a]] = cur_time + arc_len                           # :85
            else:
                assert times[dst[a]] == cur_time + arc_len                   # :87
        if not (clat["final_g"][state] == np.inf and clat["final_a"][state] == np.inf):   # :89
            this_utt_len = times[state] + len(clat["final_string"][state])   # :90
            if utt_len == -1:                                                # :91
                utt_len = this_utt_len
            elif this_utt_len != utt_len:                                    # :93
                utt_len = max(utt_len, this_utt_len)                         # :96
    if utt_len == -1:                                                        # :101
        return 0, times                                                      # :103
    return utt_len, times                                                    # :105


def compact_lattice_depth(clat):
    """lat/lattice-functions.cc:574-602 -> (depth [float32], num_frames).  The project's convention where the reference
    divides by zero (a lattice without a final state, t = 0): depth 1.0, as for the empty lattice (:581-584)."""
    if int(clat["n_states"]) == 0 or int(clat.get("start", 0)) < 0:          # :581
        return np.float32(1.0), 0                                            # :582-583
    num_arc_frames = 0                                                       # :585
    t, _ = compact_lattice_state_times(clat)                                 # :589
    for a in range(len(clat["arc_src"])):                                    # :593-594
        num_arc_frames += len(clat["arc_string"][a])                         # :597
    for s in range(int(clat["n_states"])):
        num_arc_frames += len(clat["final_string"][s])                       # :599
    if t == 0:
        return np.float32(1.0), 0
    return np.float32(num_arc_frames) / np.float32(t), t                     # :601
