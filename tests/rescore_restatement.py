"""Line-by-line restatements, in plain Python, of what gmm-rescore-lattice runs on a lattice (test infrastructure; the
product is csrc/kh_latrescore.hip and kaldi_io.lattice_to_compact_lattice):

  CompactLatticeStateTimes          lat/lattice-functions.cc:69-106
  RescoreCompactLatticeInternal     lat/lattice-functions.cc:1163-1290 with tmodel = NULL, speedup_factor = 1.0: it really
                                    builds time_to_state and walks t, updating the weights in place
  Factor                            fstext/factor-inl.h:36-151 (GetStateProperties :37-64)
  ConvertLattice                    fstext/lattice-utils-inl.h:33-87 (Lattice -> CompactLattice, invert = true)

A CompactLattice here is the dict of kaldi_io.read_compact_lattice, a Lattice the dict of kaldi_io.read_lattice.  The
decodable is a host matrix ll[frame][pdf] with tid2pdf (LogLikelihood(t, tid) = ll[t][tid2pdf[tid]], IsLastFrame(t) =
t == rows - 1).  Where the reference asserts, this raises AssertionError with the line; the statuses the library gives those
cases are named in rescore()."""
import numpy as np

F = np.float32
INF = F(np.inf)
OK, EMPTY, INCONSISTENT_TIMES, FEATURES_TOO_SHORT, BAD_TID, MISMATCH = range(6)

# StatePropertiesType, fstext/factor.h
K_INITIAL, K_FINAL, K_ARCS_IN, K_MULT_ARCS_IN, K_ARCS_OUT, K_MULT_ARCS_OUT, K_OLABELS_OUT, K_ILABELS_OUT = (1 << i for i in range(8))


class Assertion(AssertionError):
    pass


def is_zero(g, a, string):
    """CompactLatticeWeight::Zero(): LatticeWeight::Zero() (both +inf) and an empty string."""
    return g == INF and a == INF and len(string) == 0


def arcs_by_state(clat):
    n = int(clat["n_states"])
    out = [[] for _ in range(n)]
    for j in range(len(clat["arc_src"])):
        out[int(clat["arc_src"][j])].append(j)
    return out


def is_top_sorted(clat):
    """Properties(kTopSorted, true): no arc to the same or a lower-numbered state."""
    return bool(np.all(np.asarray(clat["arc_dst"]) > np.asarray(clat["arc_src"])))


def compact_lattice_state_times(clat):
    """:69-106 -> (utt_len, times)."""
    assert is_top_sorted(clat), "Input lattice must be topologically sorted."     # :70-71
    if int(clat.get("start", 0)) != 0:
        raise Assertion(":72 lat.Start() == 0")
    n = int(clat["n_states"])
    by = arcs_by_state(clat)
    times = [-1] * n                                                              # :75
    times[0] = 0
    utt_len = -1
    for state in range(n):
        cur_time = times[state]
        for j in by[state]:
            arc_len = len(clat["arc_string"][j])
            nx = int(clat["arc_dst"][j])
            if times[nx] == -1:
                times[nx] = cur_time + arc_len
            elif times[nx] != cur_time + arc_len:
                raise Assertion(":87 times[arc.nextstate] == cur_time + arc_len")
        if not is_zero(clat["final_g"][state], clat["final_a"][state], clat["final_string"][state]):   # :89
            this_utt_len = times[state] + len(clat["final_string"][state])
            if utt_len == -1:
                utt_len = this_utt_len
            elif this_utt_len != utt_len:
                utt_len = max(utt_len, this_utt_len)                              # :93-97
    if utt_len == -1:
        return 0, times                                                           # :101-104
    return utt_len, times


def rescore_compact_lattice_internal(clat, ll, tid2pdf):
    """:1163-1290 on a top-sorted clat (the caller sorts, :1173-1178).  Returns (status, arc_a, final_a): the new float32
    acoustic costs where status is OK, copies of the old ones otherwise (the reference has by then spoilt its argument
    and returns false)."""
    ll = np.asarray(ll, F)
    rows = ll.shape[0]
    num_tids = len(tid2pdf) - 1
    old_a, old_f = np.asarray(clat["arc_a"], F).copy(), np.asarray(clat["final_a"], F).copy()
    if int(clat["n_states"]) == 0 or int(clat.get("start", 0)) < 0:
        return EMPTY, old_a, old_f                                                # :1169-1172
    try:
        utt_len, state_times = compact_lattice_state_times(clat)                  # :1180
    except Assertion:
        return INCONSISTENT_TIMES, old_a, old_f
    time_to_state = [[] for _ in range(utt_len)]                                  # :1182
    by = arcs_by_state(clat)
    n = int(clat["n_states"])
    for state in range(n):
        if state_times[state] < 0:
            return INCONSISTENT_TIMES, old_a, old_f                               # :1187
    for state in range(n):
        t = state_times[state]
        for arc_id, j in enumerate(by[state]):
            arc_string = clat["arc_string"][j]
            for offset in range(len(arc_string)):
                if t < utt_len:                                                   # :1196
                    if t + offset >= utt_len:
                        return MISMATCH, old_a, old_f                             # (the reference writes past the vector)
                    time_to_state[t + offset].append((state, arc_id, int(arc_string[offset])))
                elif t != utt_len:
                    return MISMATCH, old_a, old_f                                 # :1200-1204
        if not is_zero(clat["final_g"][state], clat["final_a"][state], clat["final_string"][state]):   # :1208
            arc_string = clat["final_string"][state]
            for offset in range(len(arc_string)):
                assert t + offset < utt_len                                       # :1212
                time_to_state[t + offset].append((state, -1, int(arc_string[offset])))
    if rows < utt_len:
        return FEATURES_TOO_SHORT, old_a, old_f                                   # :1221-1225 fires at t = rows - 1
    for tuples in time_to_state:
        for _, _, tid in tuples:
            if tid < 1 or tid > num_tids:
                return BAD_TID, old_a, old_f                                      # (the reference indexes unchecked)
    arc_a, final_a = old_a.copy(), old_f.copy()
    for t in range(utt_len):                                                      # :1220
        assert not ((t < utt_len - 1) and t == rows - 1)                          # :1221
        assert time_to_state[t]                                                   # :1233
        for state, arc_id, tid in time_to_state[t]:                               # :1256
            log_like = F(ll[t, int(tid2pdf[tid])])                                # frame_scale = 1.0
            if arc_id == -1:
                final_a[state] = F(F(-log_like) + final_a[state])                 # :1270
            else:
                j = by[state][arc_id]
                arc_a[j] = F(F(-log_like) + arc_a[j])                             # :1283
    return OK, arc_a, final_a


def top_sort(n, start, src, dst):
    """fst::TopSort (fst/topsort.h): order[old] = new, or None on a cycle: reverse finishing order of DfsVisit from the start
    state, then from every unvisited state in number order, a state's arcs in order."""
    out = [[] for _ in range(n)]
    for j in range(len(src)):
        out[int(src[j])].append(int(dst[j]))
    color, finish = [0] * n, []
    for root in [start] + list(range(n)):
        if color[root]:
            continue
        color[root] = 1
        stack = [(root, 0)]
        while stack:
            s, k = stack.pop()
            if k < len(out[s]):
                stack.append((s, k + 1))
                t = out[s][k]
                if color[t] == 0:
                    color[t] = 1
                    stack.append((t, 0))
                elif color[t] == 1:
                    return None
            else:
                color[s] = 2
                finish.append(s)
    order = [0] * n
    for new, s in enumerate(reversed(finish)):
        order[s] = new
    return order


def renumber(clat, order):
    """StateSort: state s becomes order[s]; a state's arcs keep their order."""
    n = int(clat["n_states"])
    inv = np.argsort(np.asarray(order))
    src = np.asarray([order[int(s)] for s in clat["arc_src"]], np.int64)
    perm = np.argsort(src, kind="stable")
    return dict(n_states=n, start=int(order[int(clat.get("start", 0))]), arc_src=src[perm].astype(np.int32),
                arc_dst=np.asarray([order[int(d)] for d in clat["arc_dst"]], np.int32)[perm],
                arc_label=np.asarray(clat["arc_label"], np.int32)[perm], arc_g=np.asarray(clat["arc_g"], F)[perm],
                arc_a=np.asarray(clat["arc_a"], F)[perm], arc_string=[np.asarray(clat["arc_string"][j], np.int32) for j in perm],
                final_g=np.asarray(clat["final_g"], F)[inv], final_a=np.asarray(clat["final_a"], F)[inv],
                final_string=[np.asarray(clat["final_string"][s], np.int32) for s in inv])


def rescore(clat, ll, tid2pdf):
    """RescoreCompactLattice as gmm-rescore-lattice calls it -> (status, clat'): clat' = the rescored lattice in the
    numbering the reference leaves it in (sorted in place when it was not top-sorted), None unless status is OK.
    "cyclic" is returned as the status where TopSort fails (:1174-1177)."""
    c = clat
    if int(clat["n_states"]) > 0 and int(clat.get("start", 0)) >= 0 and not (is_top_sorted(clat) and int(clat.get("start", 0)) == 0):
        order = top_sort(int(clat["n_states"]), int(clat.get("start", 0)), clat["arc_src"], clat["arc_dst"])
        if order is None:
            return "cyclic", None
        c = renumber(clat, order)
    status, arc_a, final_a = rescore_compact_lattice_internal(c, ll, tid2pdf)
    if status != OK:
        return status, None
    out = dict(c)
    out["arc_a"], out["final_a"] = arc_a, final_a
    return status, out


# ---------------------------------------------------------------------------------------------------------------- Factor

def dfs_order(n, start, out_arcs):
    """DfsOrderVisitor over fst::DfsVisit: the states in the order InitState sees them."""
    color, order = [0] * n, []
    for root in [start] + list(range(n)):
        if color[root]:
            continue
        color[root] = 1
        order.append(root)
        stack = [(root, 0)]
        while stack:
            s, k = stack.pop()
            if k < len(out_arcs[s]):
                stack.append((s, k + 1))
                t = out_arcs[s][k][0]
                if color[t] == 0:
                    color[t] = 1
                    order.append(t)
                    stack.append((t, 0))
            else:
                color[s] = 2
    return order


def lattice_arcs(L):
    n = int(L["num_states"])
    out = [[] for _ in range(n)]
    for j in range(len(L["arc_src"])):
        out[int(L["arc_src"][j])].append((int(L["arc_dst"][j]), int(L["arc_il"][j]), int(L["arc_ol"][j]), F(L["arc_g"][j]), F(L["arc_a"][j])))
    return n, out


def state_properties(n, start, out, final):
    """GetStateProperties :37-64."""
    props = [0] * n
    props[start] |= K_INITIAL
    for s in range(n):
        for (nexts, il, ol, _, _) in out[s]:
            if il != 0:
                props[s] |= K_ILABELS_OUT
            if ol != 0:
                props[s] |= K_OLABELS_OUT
            if props[s] & K_ARCS_OUT:
                props[s] |= K_MULT_ARCS_OUT
            props[s] |= K_ARCS_OUT
            if props[nexts] & K_ARCS_IN:
                props[nexts] |= K_MULT_ARCS_IN
            props[nexts] |= K_ARCS_IN
        if final[s]:
            props[s] |= K_FINAL
    return props


def factor(L):
    """Factor :69-151 -> (n_states, start, arcs [(src, dst, symbol, olabel, g, a)] in AddArc order, finals {state: (g, a)},
    symbols [list of label sequences, symbols[0] = []])."""
    n, out = lattice_arcs(L)
    start = int(L["start"])
    if n == 0 or start < 0:
        return 0, -1, [], {}, [[]]
    fg, fa = np.asarray(L["state_final_graph"], F), np.asarray(L["state_final_acoustic"], F)
    final = [not (fg[s] == INF and fa[s] == INF) for s in range(n)]
    order = dfs_order(n, start, out)
    props = state_properties(n, start, out, final)
    remove = [p == (K_ARCS_IN | K_ARCS_OUT) or p == (K_ARCS_IN | K_ARCS_OUT | K_ILABELS_OUT) for p in props]   # :96-98
    mapping = {}
    symbol_mapping = {(): 0}
    arcs, finals = [], {}

    def new_state(s):
        if s not in mapping:
            mapping[s] = len(mapping)                                             # ofst->AddState()
        return mapping[s]
    for state in order:                                                           # :109
        if remove[state]:
            continue
        ns = new_state(state)
        for (nexts, il, ol, g, a) in out[state]:
            this_sym = [] if il == 0 else [il]
            while remove[nexts]:                                                  # :121
                (n2, il2, ol2, g2, a2) = out[nexts][0]
                g, a = F(g + g2), F(a + a2)                                       # Times :125
                assert ol2 == 0
                if il2 != 0:
                    this_sym.append(il2)
                nexts = n2
            nn = new_state(nexts)
            key = tuple(this_sym)
            if key not in symbol_mapping:
                symbol_mapping[key] = len(symbol_mapping)
            arcs.append((ns, nn, symbol_mapping[key], ol, g, a))
        if final[state]:
            finals[ns] = (fg[state], fa[state])
    symbols = [None] * len(symbol_mapping)
    for k, v in symbol_mapping.items():
        symbols[v] = list(k)
    return len(mapping), mapping[start], arcs, finals, symbols


def convert_lattice(L):
    """ConvertLattice :33-87, invert = true -> CompactLattice dict."""
    n, start, arcs, finals, symbols = factor(L)                                   # :46
    if n == 0:
        return dict(n_states=0, start=-1, arc_src=np.zeros(0, np.int32), arc_dst=np.zeros(0, np.int32), arc_label=np.zeros(0, np.int32),
                    arc_g=np.zeros(0, F), arc_a=np.zeros(0, F), arc_string=[], final_g=np.zeros(0, F), final_a=np.zeros(0, F), final_string=[])
    # (VectorFst keeps the arcs of one state in AddArc order)
    arcs = sorted(arcs, key=lambda x: x[0])
    fg, fa = np.full(n, INF, F), np.full(n, INF, F)
    for s, (g, a) in finals.items():
        fg[s], fa[s] = g, a
    c = dict(n_states=n, start=start, arc_src=np.asarray([x[0] for x in arcs], np.int32), arc_dst=np.asarray([x[1] for x in arcs], np.int32),
             arc_label=np.asarray([x[3] for x in arcs], np.int32), arc_g=np.asarray([x[4] for x in arcs], F),
             arc_a=np.asarray([x[5] for x in arcs], F), arc_string=[np.asarray(symbols[x[2]], np.int32) for x in arcs],   # :81-83
             final_g=fg, final_a=fa, final_string=[np.zeros(0, np.int32) for _ in range(n)])                           # :71
    order = top_sort(n, start, c["arc_src"], c["arc_dst"])                        # :54 (left alone when cyclic)
    return c if order is None else renumber(c, order)


def same_clat(got, want, what=""):
    assert int(got["n_states"]) == int(want["n_states"]), what
    assert int(got.get("start", 0)) == int(want.get("start", 0)), what
    for k in ("arc_src", "arc_dst", "arc_label"):
        assert np.array_equal(np.asarray(got[k], np.int64), np.asarray(want[k], np.int64)), (what, k)
    for k in ("arc_g", "arc_a", "final_g", "final_a"):
        assert np.asarray(got[k], F).tobytes() == np.asarray(want[k], F).tobytes(), (what, k)
    for k in ("arc_string", "final_string"):
        assert [list(map(int, x)) for x in got[k]] == [list(map(int, x)) for x in want[k]], (what, k)
