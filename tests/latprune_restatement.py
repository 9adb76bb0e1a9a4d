"""Test helper: lattice-scale | lattice-add-penalty | lattice-prune restated line by line for ONE CompactLattice and ONE
score point: PruneLattice (lat/lattice-functions.cc:186-265) plus the masks fst::Connect (:263) leaves, numpy float32 /
float64 scalars, one Python statement per reference statement (each cites its line).  OpenFst is absent, so lat/ cannot be
compiled; this is the checker of csrc/kh_latprune.hip, and tests/test_lattice_prune.py checks it in turn against brute
force, the compiled alpha/beta oracle and hand lattices.

The lattice is the CSR dict api.compact_lattice_to_prune_csr returns (top-sorted, `start` in that numbering)."""
import numpy as np

from latbest_restatement import apply_point, convert_to_cost, make_clat, random_clat, scale_tuple_weight  # noqa: F401

f32, f64 = np.float32, np.float64
INF32 = f32(np.inf)
INF = f64(np.inf)


def prune_lattice(L, scale, penalty, beam):
    """:186-265 on the weights of apply_point.  Returns dict(forward, backward = the two cost vectors, best_final_cost,
    cutoff, cost_keep = arcs that keep their nextstate at :256, final_keep, arc_keep, state_keep = what Connect leaves)."""
    g, a, fg, fa = apply_point(L, scale, penalty)
    beam = f32(beam)                                                         # BaseFloat beam
    assert beam > 0.0                                                        # :192
    num_states = int(L["n_states"])                                          # :202
    start = int(L["start"])                                                  # :201
    off, nxt = np.asarray(L["arc_offsets"], np.int64), np.asarray(L["arc_nextstate"], np.int64)
    n_arcs = len(nxt)
    forward_cost = [INF] * num_states                                        # :204-205
    forward_cost[start] = f64(0.0)                                           # :206
    best_final_cost = INF                                                    # :208
    with np.errstate(all="ignore"):
        for state in range(num_states):                                      # :211
            this_forward_cost = forward_cost[state]                          # :212
            for j in range(off[state], off[state + 1]):                      # :213
                nextstate = int(nxt[j])                                      # :217
                assert state < nextstate < num_states                        # :218
                next_forward_cost = this_forward_cost + convert_to_cost(g[j], a[j])   # :219-220
                if forward_cost[nextstate] > next_forward_cost:              # :221
                    forward_cost[nextstate] = next_forward_cost              # :222
            this_final_cost = this_forward_cost + convert_to_cost(fg[state], fa[state])   # :224-226
            if this_final_cost < best_final_cost:                            # :227
                best_final_cost = this_final_cost                            # :228
        forward = list(forward_cost)
        cutoff = best_final_cost + f64(beam)                                 # :231
        is_final = [not (fg[s] == INF32 and fa[s] == INF32) for s in range(num_states)]   # Final(s) != Weight::Zero()
        cost_keep = np.ones(n_arcs, bool)
        backward_cost = forward_cost                                         # :238 (shared memory)
        for state in range(num_states - 1, -1, -1):                          # :239
            this_forward_cost = forward_cost[state]                          # :240
            this_backward_cost = convert_to_cost(fg[state], fa[state])       # :241
            if this_backward_cost + this_forward_cost > cutoff and this_backward_cost != INF:   # :242-243
                is_final[state] = False                                      # :244 SetFinal(state, Weight::Zero())
            for j in range(off[state], off[state + 1]):                      # :245
                nextstate = int(nxt[j])                                      # :249
                arc_cost = convert_to_cost(g[j], a[j])                       # :251
                arc_backward_cost = arc_cost + backward_cost[nextstate]      # :252
                this_fb_cost = this_forward_cost + arc_backward_cost         # :253
                if arc_backward_cost < this_backward_cost:                   # :254
                    this_backward_cost = arc_backward_cost                   # :255
                if this_fb_cost > cutoff:                                    # :256
                    cost_keep[j] = False                                     # :257-258 nextstate = bad_state
            backward_cost[state] = this_backward_cost                        # :261
    # fst::Connect :263: accessible from the start state and coaccessible (reaches a final state), over the arcs that
    # kept their nextstate (bad_state is not final and has no arcs)
    access = np.zeros(num_states, bool)
    access[start] = True
    for state in range(num_states):
        if access[state]:
            for j in range(off[state], off[state + 1]):
                if cost_keep[j]:
                    access[nxt[j]] = True
    coaccess = np.array(is_final, bool)
    for state in range(num_states - 1, -1, -1):
        for j in range(off[state], off[state + 1]):
            if cost_keep[j] and coaccess[nxt[j]]:
                coaccess[state] = True
    state_keep = access & coaccess
    src = np.repeat(np.arange(num_states), np.diff(off))
    arc_keep = cost_keep & state_keep[src] & state_keep[nxt] if n_arcs else np.zeros(0, bool)
    return dict(forward=np.asarray(forward, f64), backward=np.asarray(backward_cost, f64), best_final_cost=best_final_cost,
                cutoff=cutoff, cost_keep=cost_keep, final_keep=np.asarray(is_final, bool), arc_keep=arc_keep,
                state_keep=state_keep, weights=(g, a, fg, fa))


def _subset(clat, csr, r, g, a, fg, fa):
    """DeleteStates' renumbering: the surviving states densely in the sorted order, arcs in their order within a state;
    g, a, fg, fa = the weights to carry, in CSR order."""
    n = int(csr["n_states"])
    off, nxt = np.asarray(csr["arc_offsets"], np.int64), np.asarray(csr["arc_nextstate"], np.int64)
    new, k = {}, 0
    for s in range(n):
        if r["state_keep"][s]:
            new[s] = k
            k += 1
    if k == 0:
        z, f = np.zeros(0, np.int32), np.zeros(0, f32)
        return dict(n_states=0, start=-1, arc_src=z, arc_dst=z, arc_label=z, arc_g=f, arc_a=f, arc_string=[], final_g=f,
                    final_a=f, final_string=[], complete=True, kept_states=np.zeros(0, np.int64),
                    kept_arcs=np.zeros(0, np.int64), ok=False)
    out = dict(n_states=k, start=new[int(csr["start"])], arc_src=[], arc_dst=[], arc_label=[], arc_g=[], arc_a=[], arc_string=[],
               final_g=[], final_a=[], final_string=[], complete=True, kept_states=[], kept_arcs=[], ok=True)
    for s in range(n):
        if not r["state_keep"][s]:
            continue
        old = int(csr["state_of"][s])
        out["kept_states"].append(old)
        if r["final_keep"][s]:
            out["final_g"].append(fg[s]); out["final_a"].append(fa[s]); out["final_string"].append(np.asarray(clat["final_string"][old], np.int32))
        else:
            out["final_g"].append(INF32); out["final_a"].append(INF32); out["final_string"].append(np.zeros(0, np.int32))
        for j in range(off[s], off[s + 1]):
            if r["arc_keep"][j]:
                dj = int(csr["perm"][j])
                out["kept_arcs"].append(dj)
                out["arc_src"].append(new[s]); out["arc_dst"].append(new[int(nxt[j])]); out["arc_label"].append(int(csr["arc_label"][j]))
                out["arc_g"].append(g[j]); out["arc_a"].append(a[j]); out["arc_string"].append(np.asarray(clat["arc_string"][dj], np.int32))
    for k_, dt in (("arc_src", np.int32), ("arc_dst", np.int32), ("arc_label", np.int32), ("arc_g", f32), ("arc_a", f32),
                   ("final_g", f32), ("final_a", f32), ("kept_states", np.int64), ("kept_arcs", np.int64)):
        out[k_] = np.asarray(out[k_], dt)
    return out


def prune_clat(clat, csr, scale, penalty, beam):
    """... in the layout of api.compact_lattice_prune: the weights after the point."""
    r = prune_lattice(csr, scale, penalty, beam)
    return _subset(clat, csr, r, *r["weights"])


def plain_tool(clat, csr, acoustic_scale, inv_acoustic_scale, beam):
    """latbin/lattice-prune.cc:59-99 for one lattice: the CompactLattice it writes and whether PruneLattice succeeded."""
    acoustic_scale, inv_acoustic_scale = f32(acoustic_scale), f32(inv_acoustic_scale)   # BaseFloat :43-44
    assert acoustic_scale == 1.0 or inv_acoustic_scale == 1.0                # :59
    if inv_acoustic_scale != 1.0:                                            # :60
        acoustic_scale = f32(1.0) / inv_acoustic_scale                       # :61 (stored to a float)
    assert acoustic_scale != 0.0                                             # :75
    there = [[1.0, 0.0], [0.0, f64(acoustic_scale)]]                         # AcousticLatticeScale :82
    r = prune_lattice(csr, there, f32(0.0), beam)                            # :87 (no arc is given a penalty: see below)
    g, a, fg, fa = apply_point(dict(csr, arc_label=np.zeros(len(csr["arc_label"]), np.int32)), there, f32(0.0))   # :82 alone
    back = [[1.0, 0.0], [0.0, f64(1.0) / f64(acoustic_scale)]]               # :98 the DOUBLE 1.0 / acoustic_scale
    g2, a2, fg2, fa2 = g.copy(), a.copy(), fg.copy(), fa.copy()
    for j in range(len(g)):
        g2[j], a2[j] = scale_tuple_weight(g[j], a[j], back)
    for s in range(len(fg)):
        fg2[s], fa2[s] = scale_tuple_weight(fg[s], fa[s], back)
    return _subset(clat, csr, r, g2, a2, fg2, fa2)


def assert_same_clat(got, want, what=""):
    """Exact: numbering, arc order, float bits, strings."""
    assert bool(got["ok"]) == bool(want["ok"]), what
    assert int(got["n_states"]) == int(want["n_states"]) and int(got["start"]) == int(want["start"]), what
    for k in ("arc_src", "arc_dst", "arc_label", "kept_states", "kept_arcs"):
        assert np.array_equal(np.asarray(got[k], np.int64), np.asarray(want[k], np.int64)), (what, k)
    for k in ("arc_g", "arc_a", "final_g", "final_a"):
        assert np.array_equal(np.asarray(got[k], f32).view(np.int32), np.asarray(want[k], f32).view(np.int32)), (what, k)
    for k in ("arc_string", "final_string"):
        assert len(got[k]) == len(want[k]) and all(np.array_equal(x, y) for x, y in zip(got[k], want[k])), (what, k)
