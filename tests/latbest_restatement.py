"""Test helper: lattice-scale | lattice-add-penalty | lattice-best-path restated line by line for ONE CompactLattice and
ONE score point, numpy float32 / float64 scalars, one Python statement per reference statement (each cites its line).
OpenFst is absent, so lat/ cannot be compiled; this is the checker of csrc/kh_latbest.hip, and the tests check it in turn
against brute force and the compiled alpha/beta oracle, which share no code with it.

The lattice is the CSR dict api.compact_lattice_to_csr returns (top-sorted: n_states, arc_offsets, arc_label,
arc_nextstate, arc_graph, arc_acoustic, final_graph, final_acoustic)."""
import numpy as np

f32, f64 = np.float32, np.float64
INF32 = f32(np.inf)
K_NO_STATE = -1


def scale_tuple_weight(g, a, scale):
    """fstext/lattice-weight.h:233-241; scale = 2x2 doubles."""
    if g == INF32:                                                           # :237
        return INF32, INF32                                                  # :238 Zero()
    with np.errstate(all="ignore"):
        return (f32(f64(scale[0][0]) * f64(g) + f64(scale[0][1]) * f64(a)),  # :239
                f32(f64(scale[1][0]) * f64(g) + f64(scale[1][1]) * f64(a)))  # :240


def convert_to_cost(g, a):
    """fstext/lattice-weight.h:799-801: static_cast<double>(w.Value1()) + static_cast<double>(w.Value2())."""
    with np.errstate(all="ignore"):
        return f64(g) + f64(a)


def apply_point(L, scale, penalty):
    """ScaleLattice (lattice-scale.cc:86) then AddWordInsPenToCompactLattice (lat/lattice-functions.cc:1128-1149): the arc
    and final weights the search sees."""
    scale = np.asarray(scale, f64).reshape(2, 2)
    n_arcs = len(L["arc_label"])
    g, a = np.empty(n_arcs, f32), np.empty(n_arcs, f32)
    for j in range(n_arcs):
        g[j], a[j] = scale_tuple_weight(f32(L["arc_graph"][j]), f32(L["arc_acoustic"][j]), scale)
        if L["arc_label"][j] != 0:                                           # :1140
            with np.errstate(all="ignore"):
                g[j] = f32(g[j]) + f32(penalty)                              # :1143
    n = int(L["n_states"])
    fg, fa = np.empty(n, f32), np.empty(n, f32)
    for s in range(n):
        fg[s], fa[s] = scale_tuple_weight(f32(L["final_graph"][s]), f32(L["final_acoustic"][s]), scale)
    return g, a, fg, fa


def compact_lattice_shortest_path(L, scale, penalty):
    """lat/lattice-functions.cc:1043-1126 on the weights of apply_point.  Returns None (:1091-1093, the empty best path) or
    dict(arcs = CSR arc numbers of the path, states, final_state, graph_cost, acoustic_cost (GetLinearSymbolSequence's
    float sums, lattice-best-path.cc:98), cost = best_cost_and_pred[superfinal].first)."""
    g, a, fg, fa = apply_point(L, scale, penalty)
    n = int(L["n_states"])
    off, nxt = np.asarray(L["arc_offsets"], np.int64), np.asarray(L["arc_nextstate"], np.int64)
    best_cost = [f64(np.inf)] * (n + 1)                                      # :1060,:1063
    best_pred = [K_NO_STATE] * (n + 1)                                       # :1064
    superfinal = n                                                           # :1061
    best_cost[0] = f64(0.0)                                                  # :1066
    with np.errstate(all="ignore"):
        for s in range(n):                                                   # :1067
            my_cost = best_cost[s]                                           # :1068
            for j in range(off[s], off[s + 1]):                              # :1069
                arc_cost = convert_to_cost(g[j], a[j])                       # :1073
                next_cost = my_cost + arc_cost                               # :1074
                if next_cost < best_cost[nxt[j]]:                            # :1075
                    best_cost[nxt[j]] = next_cost                            # :1076
                    best_pred[nxt[j]] = s                                    # :1077
            final_cost = convert_to_cost(fg[s], fa[s])                       # :1080
            tot_final = my_cost + final_cost                                 # :1081
            if tot_final < best_cost[superfinal]:                            # :1082
                best_cost[superfinal] = tot_final                            # :1083
                best_pred[superfinal] = s                                    # :1084
    states = []                                                              # :1087
    cur_state = superfinal                                                   # :1088
    while cur_state != 0:                                                    # :1089
        prev_state = best_pred[cur_state]                                    # :1090
        if prev_state == K_NO_STATE:                                         # :1091
            return None                                                      # :1093
        states.append(prev_state)                                            # :1095
        assert cur_state != prev_state                                       # :1096
        cur_state = prev_state                                               # :1097
    states.reverse()                                                         # :1099
    arcs = []
    tot_g, tot_a = f32(0.0), f32(0.0)                                        # LatticeWeight::One()
    with np.errstate(all="ignore"):
        for i in range(len(states)):                                         # :1102
            if i + 1 < len(states):                                          # :1104
                have_arc, cur_arc = False, -1                                # :1105-1106
                for j in range(off[states[i]], off[states[i] + 1]):          # :1107
                    if nxt[j] == states[i + 1]:                              # :1111
                        if not have_arc or convert_to_cost(g[j], a[j]) < convert_to_cost(g[cur_arc], a[cur_arc]):   # :1112-1113
                            cur_arc = j                                      # :1114
                            have_arc = True                                  # :1115
                assert have_arc                                              # :1119
                arcs.append(cur_arc - int(off[0]))                           # :1120
                tot_g, tot_a = f32(tot_g + g[cur_arc]), f32(tot_a + a[cur_arc])   # Times, fstext/lattice-weight.h
            else:
                tot_g, tot_a = f32(tot_g + fg[states[i]]), f32(tot_a + fa[states[i]])   # :1123 SetFinal, Times of the final weight last
    return dict(arcs=np.asarray(arcs, np.int64), states=states, final_state=states[-1], graph_cost=tot_g, acoustic_cost=tot_a,
                cost=best_cost[superfinal])


def best_path_of_clat(clat, csr, scale, penalty):
    """... and what lattice-best-path.cc:89-98 makes of it, in the layout of api.compact_lattice_best_paths."""
    r = compact_lattice_shortest_path(csr, scale, penalty)
    if r is None:
        return None
    arcs = np.asarray(csr["perm"])[r["arcs"]] if len(r["arcs"]) else np.zeros(0, np.int64)
    fs = int(csr["state_of"][r["final_state"]])
    labels = np.asarray(clat["arc_label"], np.int32)[arcs]
    strings = [np.asarray(clat["arc_string"][j], np.int32) for j in arcs] + [np.asarray(clat["final_string"][fs], np.int32)]
    return dict(words=labels[labels != 0], alignment=np.concatenate(strings + [np.zeros(0, np.int32)]).astype(np.int32),
                graph_cost=r["graph_cost"], acoustic_cost=r["acoustic_cost"], arcs=arcs.astype(np.int64), final_state=fs)


def make_clat(n_states, arcs, finals, start=0):
    """arcs: (src, dst, label, g, a, string); finals: {state: (g, a, string)} -> the CompactLattice dict layout."""
    fg, fa = np.full(n_states, np.inf, f32), np.full(n_states, np.inf, f32)
    fs = [np.zeros(0, np.int32) for _ in range(n_states)]
    for s, (g, a, string) in finals.items():
        fg[s], fa[s], fs[s] = g, a, np.asarray(string, np.int32)
    return dict(n_states=n_states, start=start, arc_src=np.asarray([x[0] for x in arcs], np.int32),
                arc_dst=np.asarray([x[1] for x in arcs], np.int32), arc_label=np.asarray([x[2] for x in arcs], np.int32),
                arc_g=np.asarray([x[3] for x in arcs], f32), arc_a=np.asarray([x[4] for x in arcs], f32),
                arc_string=[np.asarray(x[5], np.int32) for x in arcs], final_g=fg, final_a=fa, final_string=fs, complete=True)


def random_clat(rng, n_states, max_out=4, quantum=0.25, p_eps=0.2, p_parallel=0.3, max_string=3, p_final=0.1):
    """A random top-sorted CompactLattice: every state but the last has an arc to a higher-numbered state, the last state is
    final (so a final state is reachable from every state), weights are multiples of `quantum` (ties are the rule),
    parallel arcs, label-0 arcs, empty and long strings."""
    arcs = []
    w = lambda: f32(quantum * int(rng.integers(0, 24)))
    string = lambda: rng.integers(1, 50, size=int(rng.integers(0, max_string + 1)) if rng.random() > 0.1 else int(rng.integers(10, 40)))
    for s in range(n_states - 1):
        for _ in range(int(rng.integers(1, max_out + 1))):
            d = int(min(n_states - 1, s + 1 + int(rng.geometric(0.35)) - 1))
            label = 0 if rng.random() < p_eps else int(rng.integers(1, 30))
            arcs.append((s, d, label, w(), w(), string()))
            if rng.random() < p_parallel:
                arcs.append((s, d, 0 if rng.random() < p_eps else int(rng.integers(1, 30)), w(), w(), string()))
    finals = {n_states - 1: (w(), w(), string())}
    for s in range(n_states - 1):
        if rng.random() < p_final:
            finals[s] = (w(), w(), string())
    return make_clat(n_states, arcs, finals)


def score_points_36(api):
    """local/score.sh's grid: LMWT 9..20 x word insertion penalty 0.0 / 0.5 / 1.0."""
    return [api.score_point(inv_acoustic_scale=float(l), word_ins_penalty=w) for w in (0.0, 0.5, 1.0) for l in range(9, 21)]
