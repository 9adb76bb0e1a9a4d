"""Line-by-line Python restatement of FasterDecoder (decoder/faster-decoder.{h,cc}) as AlignUtteranceWrapper drives it
(decoder/decoder-wrappers.cc:423-505), in two modes.

  mode "reference": the reference as it is written - the HashList's insertion and iteration order (util/hash-list-inl.h),
      the running next_weight_cutoff of ProcessEmitting, first-arrival ties, the LIFO queue of ProcessNonemitting, tokens
      that keep pointing at their predecessor TOKEN.
  mode "library": the rule of include/kaldi_hip.h at kh_align_compiled - acceptance against the frame's FINAL
      next_weight_cutoff, per-(frame, state) backpointers, the eps closure in rounds that each read the round before, equal
      costs to the lowest arc position and the lowest final state, the path's costs formed again along the path.

Doubles are Python floats; every float (BaseFloat) value is a Python float that holds a float32 value exactly, and f32()
is the rounding of a BaseFloat assignment.  No numpy scalar takes part in the arithmetic (numpy would keep a float32 + a
Python float in float32)."""
import numpy as np

INF = float("inf")
FLT_MAX = float(np.finfo(np.float32).max)
DONE, NO_FINAL, NEEDS_ROOM, TOO_LARGE, BOUND, BAD_INPUT = 0, 1, 2, 3, 4, 5


def f32(x):
    with np.errstate(over="ignore"):
        return float(np.float32(x))


class Graph:
    """The CSR dict of kaldi_io.read_fst as Python lists (weights as exact doubles of the float32 values)."""

    def __init__(self, g):
        self.S = int(g["num_states"])
        self.start = int(g["start"])
        self.off = [int(x) for x in g["arc_offsets"]]
        self.il = [int(x) for x in g["ilabel"]]
        self.ol = [int(x) for x in g["olabel"]]
        self.w = [float(x) for x in np.asarray(g["weight"], np.float32).astype(np.float64)]
        self.ns = [int(x) for x in g["nextstate"]]
        self.final = [float(x) for x in np.asarray(g["final"], np.float32).astype(np.float64)]
        self.src = [s for s in range(self.S) for _ in range(self.off[s], self.off[s + 1])]
        self.n_eps = sum(1 for x in self.il if x == 0)


def _loglikes(ll):
    return [[float(x) for x in row] for row in np.asarray(ll, np.float32).astype(np.float64)]


def _cutoff(costs, beam, min_active, beam_delta, stats=None):
    """GetCutoff :151-213 with max_active = INT_MAX, over the token costs in list order.  Returns (weight_cutoff,
    adaptive_beam, index of best_elem or None).  stats counts which branch gave the cutoff: cut_inf (at most min_active
    tokens), cut_select (the (min_active+1)-th smallest float-rounded cost), cut_beam."""
    if stats is not None:
        for k in ("cut_inf", "cut_select", "cut_beam"):
            stats.setdefault(k, 0)
    best, best_i = INF, None
    for i, w in enumerate(costs):
        if w < best:
            best, best_i = w, i
    if min_active == 0:
        if stats is not None:
            stats["cut_beam"] += 1
        return best + beam, beam, best_i
    tmp = [f32(w) for w in costs]                      # tmp_array_ is a vector<BaseFloat>
    beam_cutoff = best + beam
    min_active_cutoff = INF
    if len(tmp) > min_active:
        min_active_cutoff = sorted(tmp)[min_active]    # nth_element
    if stats is not None:
        stats["cut_inf" if len(tmp) <= min_active else "cut_select" if min_active_cutoff > beam_cutoff else "cut_beam"] += 1
    if min_active_cutoff > beam_cutoff:
        return min_active_cutoff, f32(min_active_cutoff - best + beam_delta), best_i
    return beam_cutoff, beam, best_i


def _finish(G, ll, tid2pdf, path, best_state, total, stats):
    """GetBestPath's floats :117-126 along `path` (arc positions in path order), then GetLinearSymbolSequence's order for
    alignment, words and the weight (float sums, the final weight last)."""
    arcs, c, fr = [], 0.0, 0
    for a in path:
        w = G.w[a]
        nc = c + w
        if G.il[a] != 0:
            nc = nc + (-ll[fr][tid2pdf[G.il[a]]])
            fr += 1
        tot = f32(nc - c)
        arcs.append((G.il[a], G.ol[a], w, f32(tot - w)))
        c = nc
    g = a_ = 0.0
    for x in arcs:
        g, a_ = f32(g + x[2]), f32(a_ + x[3])
    g = f32(g + G.final[best_state])
    out = dict(status=DONE, alignment=[x[0] for x in arcs if x[0] != 0], words=[x[1] for x in arcs if x[1] != 0], cost=total,
               path=arcs, weight=(g, a_), like=f32(-f32(g + a_)), path_cost=c, best_state=best_state)
    out.update(stats)
    return out


# ------------------------------------------------------------------------------------------------------------ library
def _closure_lib(G, eps_in, cur, cutoff, bprow, stats):
    if G.n_eps == 0:
        return cur, True
    for _ in range(G.S + 1):
        new, changed = list(cur), False
        for d in range(G.S):
            best, arc = cur[d], -1
            for (src, a, w) in eps_in[d]:
                cs = cur[src]
                if cs < INF and not cs > cutoff:
                    nc = cs + w
                    if not nc > cutoff:
                        if nc < best:
                            best, arc = nc, a
                        elif nc == best and a != (arc if arc >= 0 else bprow[d]):
                            stats["had_tie"] = True
            new[d] = best
            if arc >= 0:
                bprow[d] = arc
                changed = True
        cur = new
        if not changed:
            return cur, True
    return cur, False


def decode_library(g, ll, tid2pdf, beam, min_active=20, beam_delta=0.5):
    """One Decode() + ReachedFinal + GetBestPath by the library's rule.  tid2pdf: indexed by transition-id."""
    G = g if isinstance(g, Graph) else Graph(g)
    ll = _loglikes(ll)
    beam, beam_delta = f32(beam), f32(beam_delta)
    stats = dict(had_tie=False, order_sensitive=False)
    emit_in = [[] for _ in range(G.S)]
    eps_in = [[] for _ in range(G.S)]
    for a in range(len(G.il)):
        if G.il[a] != 0:
            emit_in[G.ns[a]].append((G.src[a], int(tid2pdf[G.il[a]]), a, G.w[a]))
        else:
            eps_in[G.ns[a]].append((G.src[a], a, G.w[a]))
    cur = [INF] * G.S
    cur[G.start] = 0.0
    bp = [[-1] * G.S]
    cur, ok = _closure_lib(G, eps_in, cur, FLT_MAX, bp[0], stats)
    for f in range(len(ll)):
        if not ok:
            break
        weight_cutoff, adaptive_beam, _ = _cutoff([c for c in cur if c < INF], beam, min_active, beam_delta, stats)
        new, row, gmin = [INF] * G.S, [-1] * G.S, INF
        n_at_min = [0] * G.S
        for d in range(G.S):
            for (src, col, a, w) in emit_in[d]:
                cs = cur[src]
                if cs < weight_cutoff:
                    nw = (cs + w) + (-ll[f][col])
                    if nw < new[d]:
                        new[d], row[d], n_at_min[d] = nw, a, 1
                    elif nw == new[d] and nw < INF:
                        n_at_min[d] += 1
            gmin = min(gmin, new[d])
        next_cutoff = gmin + adaptive_beam
        for d in range(G.S):
            if not new[d] < next_cutoff:
                new[d], row[d] = INF, -1
            elif n_at_min[d] > 1:
                stats["had_tie"] = True
        bp.append(row)
        cur, ok = _closure_lib(G, eps_in, new, next_cutoff, row, stats)
    if not ok:
        return dict(status=BOUND, alignment=[], words=[], cost=INF, path=[], **stats)
    best, bs = INF, -1
    for d in range(G.S):
        if cur[d] < INF and G.final[d] != INF:
            tc = cur[d] + G.final[d]
            if tc < best:
                best, bs = tc, d
            elif tc == best:
                stats["had_tie"] = True
    if bs < 0:
        return dict(status=NO_FINAL, alignment=[], words=[], cost=INF, path=[], **stats)
    path, state, frame = [], bs, len(ll)
    for _ in range((len(ll) + 1) * G.S + 1):
        a = bp[frame][state]
        if a < 0:
            break
        path.append(a)
        if G.il[a] != 0:
            frame -= 1
        state = G.src[a]
    assert a < 0 and frame == 0 and state == G.start
    return _finish(G, ll, tid2pdf, path[::-1], bs, best, stats)


# ---------------------------------------------------------------------------------------------------------- reference
class _Token:
    __slots__ = ("arc", "prev", "cost")

    def __init__(self, arc, prev, cost):
        self.arc, self.prev, self.cost = arc, prev, cost


class _HashList:
    """util/hash-list-inl.h: the list is the buckets in the order they were first occupied (:132-146), each bucket's
    elements in insertion order (:147-153); the size survives Clear()."""

    def __init__(self):
        self.size = 0
        self.order, self.bucket = [], {}

    def clear(self):
        lst = self.items()
        self.order, self.bucket = [], {}
        return lst

    def items(self):
        return [e for i in self.order for e in self.bucket[i]]

    def find(self, key):
        for e in self.bucket.get(key % self.size, ()):
            if e[0] == key:
                return e
        return None

    def insert(self, key, val):
        i = key % self.size
        if i not in self.bucket:
            self.bucket[i] = []
            self.order.append(i)
        self.bucket[i].append([key, val])


class ReferenceDecoder:
    """FasterDecoder; the object survives a second Decode() with another beam, as in AlignUtteranceWrapper (the hash keeps
    its size)."""

    def __init__(self, g, tid2pdf, min_active=20, beam_delta=0.5):
        self.G = g if isinstance(g, Graph) else Graph(g)
        self.tid2pdf = tid2pdf
        self.min_active, self.beam_delta = min_active, f32(beam_delta)
        self.toks = _HashList()
        self.toks.size = 1000                                           # :32
        self.stats = dict(had_tie=False, order_sensitive=False, n_sensitive=0)

    def _nonemitting(self, cutoff):                                     # :306-346
        G, toks = self.G, self.toks
        queue = [e[0] for e in toks.items()]
        while queue:
            state = queue.pop()
            tok = toks.find(state)[1]
            if tok.cost > cutoff:
                continue
            for a in range(G.off[state], G.off[state + 1]):
                if G.il[a] == 0:
                    new = _Token(a, tok, tok.cost + G.w[a])
                    if new.cost > cutoff:
                        continue
                    e = toks.find(G.ns[a])
                    if e is None:
                        toks.insert(G.ns[a], new)
                        queue.append(G.ns[a])
                    else:
                        if e[1].cost == new.cost and (e[1].arc != a or e[1].prev is not tok):
                            self.stats["had_tie"] = True
                        if e[1].cost > new.cost:
                            e[1] = new
                            queue.append(G.ns[a])

    def _emitting(self, llrow, beam):                                   # :224-303
        G, toks = self.G, self.toks
        last = toks.clear()
        weight_cutoff, adaptive_beam, best_i = _cutoff([e[1].cost for e in last], beam, self.min_active, self.beam_delta)
        new_sz = int(f32(f32(len(last)) * 2.0))                        # PossiblyResizeHash :215-221, hash_ratio 2.0
        if new_sz > toks.size:
            toks.size = new_sz
        next_cutoff = INF
        if best_i is not None:
            state, tok = last[best_i]
            for a in range(G.off[state], G.off[state + 1]):
                if G.il[a] != 0:
                    new_weight = (G.w[a] + tok.cost) + (-llrow[self.tid2pdf[G.il[a]]])
                    if new_weight + adaptive_beam < next_cutoff:
                        next_cutoff = new_weight + adaptive_beam
        for state, tok in last:
            if tok.cost < weight_cutoff:
                for a in range(G.off[state], G.off[state + 1]):
                    if G.il[a] != 0:
                        new_weight = (G.w[a] + tok.cost) + (-llrow[self.tid2pdf[G.il[a]]])
                        if new_weight < next_cutoff:
                            new = _Token(a, tok, new_weight)
                            e = toks.find(G.ns[a])
                            if new_weight + adaptive_beam < next_cutoff:
                                next_cutoff = new_weight + adaptive_beam
                            if e is None:
                                toks.insert(G.ns[a], new)
                            else:
                                if e[1].cost == new.cost:
                                    self.stats["had_tie"] = True
                                if e[1].cost > new.cost:
                                    e[1] = new
        n = sum(1 for e in toks.items() if not e[1].cost < next_cutoff)   # tokens the frame's final cutoff would refuse
        if n:
            self.stats["order_sensitive"] = True
            self.stats["n_sensitive"] += n
        return next_cutoff

    def decode(self, ll, beam):
        G, toks = self.G, self.toks
        ll = _loglikes(ll)
        toks.clear()                                                     # InitDecoding :36-45
        toks.insert(G.start, _Token(-1, None, 0.0))
        self._nonemitting(FLT_MAX)
        for row in ll:
            self._nonemitting(self._emitting(row, f32(beam)))
        stats = dict(self.stats)
        items = toks.items()
        if not any(e[1].cost != INF and G.final[e[0]] != INF for e in items):   # ReachedFinal :78-85
            return dict(status=NO_FINAL, alignment=[], words=[], cost=INF, path=[], **stats)
        best, best_e = INF, None
        for e in items:                                                  # :103-111
            this_cost = e[1].cost + G.final[e[0]]
            if this_cost == best and this_cost != INF:
                stats["had_tie"] = True
            if this_cost < best and this_cost != INF:
                best, best_e = this_cost, e
        arcs, tok = [], best_e[1]
        while tok is not None:                                           # :117-127
            tot = f32(tok.cost - (tok.prev.cost if tok.prev is not None else 0.0))
            if tok.arc >= 0:
                arcs.append((G.il[tok.arc], G.ol[tok.arc], G.w[tok.arc], f32(tot - G.w[tok.arc])))
            tok = tok.prev
        arcs.reverse()
        g = a_ = 0.0
        for x in arcs:
            g, a_ = f32(g + x[2]), f32(a_ + x[3])
        g = f32(g + G.final[best_e[0]])
        out = dict(status=DONE, alignment=[x[0] for x in arcs if x[0] != 0], words=[x[1] for x in arcs if x[1] != 0], cost=best,
                   path=arcs, weight=(g, a_), like=f32(-f32(g + a_)), best_state=best_e[0])
        out.update(stats)
        return out


def align(g, ll, tid2pdf, beam, retry_beam=0.0, mode="library", min_active=20, beam_delta=0.5):
    """AlignUtteranceWrapper :439-482 for one utterance: Decode, the retry, the best path.  Adds `retried`."""
    if (retry_beam != 0 and retry_beam <= beam) or beam <= 0:
        raise ValueError("Beams do not make sense: beam %g, retry-beam %g" % (beam, retry_beam))
    G = Graph(g)
    if mode == "reference":
        dec = ReferenceDecoder(G, tid2pdf, min_active, beam_delta)
        run = lambda b: dec.decode(ll, b)
    else:
        run = lambda b: decode_library(G, ll, tid2pdf, b, min_active, beam_delta)
    r = run(beam)
    retried = False
    if r["status"] == NO_FINAL and retry_beam != 0:
        retried = True
        r2 = run(retry_beam)
        r2["had_tie"] = r2["had_tie"] or r["had_tie"]
        r2["order_sensitive"] = r2["order_sensitive"] or r["order_sensitive"]
        r = r2
    r["retried"] = retried
    return r
