"""lat/word-align-lattice.cc restated in Python, in two parts.

(1) machine(): class LatticeWordAligner line by line - CreateSuperFinal, the labels of :275-282, the LIFO queue,
    ProcessQueueElement / ProcessFinal with their epsilon arcs, the three Output*Arc scans and OutputArcForce - up to, not
    including, RemoveEpsilonsFromLattice.  Two deliberate differences, both part of the contract in include/kaldi_hip.h: the
    KALDI_ERR of :595-603 is recorded (without its `!*error` guard) instead of thrown, and exploring goes on after it.
(2) align(): the epsilon-free result by the contract's rule, computed FROM (1)'s machine - the epsilon closure of every
    output state over the machine's epsilon arcs, not the pair tables of csrc/kh_latalign.hip.

Lattices are the dicts of kaldi_io.read_compact_lattice (with the strings), top-sorted.  tm: dict(tid2phone,
tid_is_final, tid_is_self_loop); wb: dict(phone_to_type, reorder, silence_label, partial_word_label)."""
import numpy as np

F = np.float32
INF = F(np.inf)
NO, BEGIN, END, SINGLETON, INTERNAL, NONWORD = range(6)
OK, ERROR, EMPTY, TOO_MANY, FATAL = range(5)


class TimesError(ValueError):
    pass


def better(w1, w2):
    """Compare of fstext/lattice-weight.h:295-308; where it is 0, the smaller acoustic cost (the contract's tie rule)."""
    f1, f2 = F(w1[0] + w1[1]), F(w2[0] + w2[1])
    if f1 != f2:
        return f1 < f2
    if w1[0] != w2[0]:
        return w1[0] < w2[0]
    return w1[1] < w2[1]


def better_compact(x, y):
    """Compare of CompactLatticeWeight (:562-576) > 0, x = (weight, string)."""
    if better(x[0], y[0]):
        return True
    if better(y[0], x[0]):
        return False
    if len(x[1]) != len(y[1]):
        return len(x[1]) < len(y[1])
    for p, q in zip(x[1], y[1]):
        if p != q:
            return p > q
    return False


def create_super_final(clat):
    """fstext/fstext-utils-inl.h CreateSuperFinal -> (n_states, arcs per state [(label, (g, a), string, dst)], final state)."""
    n = int(clat["n_states"])
    arcs = [[] for _ in range(n)]
    order = np.argsort(np.asarray(clat["arc_src"]), kind="stable")
    for j in order:
        arcs[int(clat["arc_src"][j])].append((int(clat["arc_label"][j]), (F(clat["arc_g"][j]), F(clat["arc_a"][j])),
                                             tuple(int(t) for t in clat["arc_string"][j]), int(clat["arc_dst"][j])))
    fg, fa = np.asarray(clat["final_g"], F), np.asarray(clat["final_a"], F)
    finals = [s for s in range(n) if not (fg[s] == INF and fa[s] == INF)]
    if len(finals) == 1:
        f = finals[0]
        if fg[f] == 0 and fa[f] == 0 and len(clat["final_string"][f]) == 0 and not arcs[f]:
            return n, arcs, f
    arcs.append([])
    for s in finals:
        arcs[s].append((0, (fg[s], fa[s]), tuple(int(t) for t in clat["final_string"][s]), n))
    return n + 1, arcs, n


def state_times(n, arcs, start):
    tm = [-1] * n
    tm[start] = 0
    for s in range(n):
        if tm[s] < 0:
            continue
        for _, _, string, d in arcs[s]:
            if d <= s:
                raise ValueError("not top-sorted")
            t = tm[s] + len(string)
            if tm[d] >= 0 and tm[d] != t:
                raise TimesError("state %d is reached after %d and after %d transition-ids" % (d, tm[d], t))
            tm[d] = t
    return tm


class Aligner:
    def __init__(self, clat, tm, wb, max_states):
        self.phone = lambda t: int(tm["tid2phone"][t])
        self.final = lambda t: bool(tm["tid_is_final"][t])
        self.self_loop = lambda t: bool(tm["tid_is_self_loop"][t])
        p2t = wb["phone_to_type"]
        self.type = lambda p: int(p2t[p])
        self.reorder = bool(wb["reorder"])
        self.max_states = int(max_states)
        self.n, self.arcs, self.sf = create_super_final(clat)          # :267
        self.start = int(clat.get("start", 0))
        self.sil, self.partial = int(wb["silence_label"]), int(wb["partial_word_label"])
        self.sil_in, self.partial_in = self.sil, self.partial
        if self.partial == 0 or self.sil == 0:                           # :275-282
            unused = 1 + max([0] + [int(x) for x in clat["arc_label"]])
            if self.partial == 0:
                self.partial = unused
            if self.sil == 0:
                self.sil = unused
        self.error = False
        self.fatal = False
        self.too_many = False
        self.map = {}
        self.tuples = []
        self.queue = []
        self.out = []            # per machine state: [(kind 'eps' | 'out', label, weight, string, dst)]
        self.final_w = []        # per machine state: None or (g, a)

    def state_for(self, tup):                                            # GetStateForTuple :159-170
        s = self.map.get(tup)
        if s is None:
            s = len(self.tuples)
            self.map[tup] = s
            self.tuples.append(tup)
            self.out.append([])
            self.final_w.append(None)
            self.queue.append((tup, s))
        return s

    def err(self):
        self.error = True

    # the three scans return None or (label, n consumed, words dropped)
    def normal_word(self, tids, words):                                  # :443-528
        if not tids or not words:
            return None
        begin = self.phone(tids[0])
        if self.type(begin) != BEGIN:
            return None
        n, i = len(tids), 0
        while i < n and not self.final(tids[i]):
            i += 1
        if i == n:
            return None
        i += 1
        if self.reorder:
            while i < n and self.self_loop(tids[i]):
                i += 1
        if i == n:
            return None
        if self.phone(tids[i - 1]) != begin and not self.error:
            self.err()
        while i < n:
            tp = self.type(self.phone(tids[i]))
            if tp == END:
                break
            if tp != INTERNAL and not self.error:
                self.err()
            i += 1
        if i == n:
            return None
        final_phone = self.phone(tids[i])
        while i < n:
            if self.phone(tids[i]) != final_phone and not self.error:
                self.err()
            if self.final(tids[i]):
                break
            i += 1
        if i == n:
            return None
        i += 1
        if self.reorder:
            while i < n and self.self_loop(tids[i]):
                i += 1
        if i == n:
            return None
        if self.phone(tids[i - 1]) != final_phone and not self.error:
            self.err()
        return words[0], i, 1

    def silence(self, tids, words):                                      # :346-389
        if not tids:
            return None
        phone = self.phone(tids[0])
        if self.type(phone) != NONWORD:
            return None
        n, i = len(tids), 1
        while i < n:
            if self.phone(tids[i]) != phone and not self.error:
                self.err()
            if self.final(tids[i]):
                break
            i += 1
        if i == n:
            return None
        i += 1
        if self.reorder:
            while i < n and self.self_loop(tids[i]):
                i += 1
        if i == n:
            return None
        return self.sil, i, 0                                            # :375-379 only warns

    def one_phone_word(self, tids, words):                               # :392-438
        if not tids or not words:
            return None
        phone = self.phone(tids[0])
        if self.type(phone) != SINGLETON:
            return None
        n, i = len(tids), 1
        while i < n:
            if self.final(tids[i]):                                      # :406-410 only warns
                break
            i += 1
        if i == n:
            return None
        i += 1
        if self.reorder:
            while i < n and self.self_loop(tids[i]):
                i += 1
        if i == n:
            return None
        if self.phone(tids[i - 1]) != phone and not self.error:
            self.err()
        return words[0], i, 1

    def plausible(self, tids):                                           # :532-551
        if not tids:
            return False
        first, last = self.phone(tids[0]), self.phone(tids[-1])
        if (self.type(first) == SINGLETON and first == last) or (self.type(first) == BEGIN and self.type(last) == END):
            if not self.reorder:
                return self.final(tids[-1])
            i = len(tids) - 1
            while i > 0 and self.self_loop(tids[i]):
                i -= 1
            return self.final(tids[i])
        return False

    def force(self, tids, words):                                        # :554-635 -> (label, n consumed, words dropped)
        if words and tids:
            if not self.error and not self.plausible(tids):
                self.err()
            return words[0], len(tids), 1
        if words:
            if not self.error:
                self.err()
            return 0, 0, len(words)
        first = self.phone(tids[0])
        if self.type(first) == NONWORD:
            if first != self.phone(tids[-1]):
                self.fatal = True                                        # :595-603, recorded
            elif not self.error:
                i = len(tids) - 1
                if self.reorder:
                    while self.self_loop(tids[i]) and i > 0:
                        i -= 1
                if not self.final(tids[i]):
                    self.err()
            return self.sil, len(tids), 0
        if not self.error:
            self.err()
        return self.partial, len(tids), 0

    def process(self):                                                   # ProcessQueueElement :201-250
        (s_in, tids, words), out_state = self.queue.pop()
        got = self.normal_word(tids, words) or self.silence(tids, words) or self.one_phone_word(tids, words)
        one = (F(0), F(0))
        if got:
            label, k, wd = got
            dst = self.state_for((s_in, tids[k:], words[wd:]))
            assert dst != out_state
            self.out[out_state].append(("out", label, one, tids[:k], dst))
            return
        if s_in == self.sf:                                              # ProcessFinal :172-198
            if not tids and not words:
                self.final_w[out_state] = one
            else:
                label, k, wd = self.force(tids, words)
                dst = self.state_for((s_in, tids[k:], words[wd:]))
                assert dst != out_state
                self.out[out_state].append(("out", label, one, tids[:k], dst))
        for label, w, string, nxt in self.arcs[s_in]:                    # Advance :40-48
            dst = self.state_for((nxt, tids + string, words + ((label,) if label != 0 else ())))
            assert dst != out_state
            self.out[out_state].append(("eps", 0, w, (), dst))

    def run(self):                                                       # AlignLattice :303-328
        self.state_for((self.start, (), ()))
        while self.queue:
            if self.max_states > 0 and len(self.tuples) > self.max_states:
                self.too_many = True
                return self
            self.process()
        return self


def machine(clat, tm, wb, max_states=0):
    return Aligner(clat, tm, wb, max_states).run()


def align(clat, tm, wb, max_states=0):
    """dict(status, n_tuples, n_states, final [n x 2 float32], arcs [(src, dst, label, g, a, string tuple)], state_keys)."""
    if int(clat["n_states"]) == 0 or int(clat.get("start", 0)) < 0:
        return dict(status=EMPTY, n_tuples=0, n_states=0, final=np.zeros((0, 2), F), arcs=[])
    n0, arcs0, _ = create_super_final(clat)
    times = state_times(n0, arcs0, int(clat.get("start", 0)))
    M = machine(clat, tm, wb, max_states)
    if M.too_many:               # n_tuples: by the contract max_states + 1; len(M.tuples) here depends on the LIFO order
        return dict(status=TOO_MANY, n_tuples=int(max_states) + 1, n_states=0, final=np.zeros((0, 2), F), arcs=[])
    if M.fatal:
        return dict(status=FATAL, n_tuples=len(M.tuples), n_states=0, final=np.zeros((0, 2), F), arcs=[])
    status = ERROR if M.error else OK
    nT = len(M.tuples)
    outputs = sorted({0} | {dst for arcs in M.out for kind, _, _, _, dst in arcs if kind == "out"})
    by_input_state = sorted(range(nT), key=lambda t: M.tuples[t][0])
    arcs_of, final_of = {}, {}
    for S in outputs:
        d = {S: (F(0), F(0))}
        arcs, fin = [], None
        for T in by_input_state:                                         # a topological order of the epsilon arcs
            if T not in d:
                continue
            if M.final_w[T] is not None:
                fin = d[T] if fin is None or better(d[T], fin) else fin
            for kind, label, w, string, dst in M.out[T]:
                if kind == "eps":
                    cand = (F(d[T][0] + w[0]), F(d[T][1] + w[1]))
                    if dst not in d or better(cand, d[dst]):
                        d[dst] = cand
                else:
                    arcs.append((label, dst, d[T], string))
        arcs_of[S], final_of[S] = arcs, fin

    def key(S):
        s_in, tids, words = M.tuples[S]
        return (S != 0, times[s_in] - len(tids), s_in, -len(words), words, tids)
    order = sorted(outputs, key=key)
    keep = {}
    for S in reversed(order):
        keep[S] = final_of[S] is not None or any(keep.get(dst, False) for _, dst, _, _ in arcs_of[S])
    if not keep[0]:
        return dict(status=status, n_tuples=nT, n_states=0, final=np.zeros((0, 2), F), arcs=[])
    kept = [S for S in order if keep[S]]
    num = {S: i for i, S in enumerate(kept)}
    final = np.full((len(kept), 2), np.inf, F)
    out = []
    for S in kept:
        if final_of[S] is not None:
            final[num[S]] = final_of[S]
        merged = {}
        for label, dst, w, string in arcs_of[S]:
            if not keep[dst]:
                continue
            k = (num[dst], label)
            if k not in merged or better_compact((w, string), merged[k]):
                merged[k] = (w, string)
        for (dst, label), (w, string) in sorted(merged.items()):
            if (M.sil_in == 0 and label == M.sil) or (M.partial_in == 0 and label == M.partial):
                label = 0
            out.append((num[S], dst, label, w[0], w[1], string))
    return dict(status=status, n_tuples=nT, n_states=len(kept), final=final, arcs=out,
                state_keys=[(times[M.tuples[S][0]] - len(M.tuples[S][1]),) + M.tuples[S] for S in kept])


def to_clat(res):
    """The aligned lattice as a read_compact_lattice dict (None without states)."""
    if res["n_states"] == 0:
        return None
    a = res["arcs"]
    n = res["n_states"]
    return dict(n_states=n, start=0, arc_src=np.asarray([x[0] for x in a], np.int32), arc_dst=np.asarray([x[1] for x in a], np.int32),
                arc_label=np.asarray([x[2] for x in a], np.int32), arc_g=np.asarray([x[3] for x in a], F),
                arc_a=np.asarray([x[4] for x in a], F), arc_string=[np.asarray(x[5], np.int32) for x in a],
                final_g=res["final"][:, 0].copy(), final_a=res["final"][:, 1].copy(),
                final_string=[np.zeros(0, np.int32) for _ in range(n)])


def assert_same(got, want, what=""):
    """Field by field, bit by bit."""
    assert got["status"] == want["status"], (what, got["status"], want["status"])
    assert got["n_tuples"] == want["n_tuples"], (what, got["n_tuples"], want["n_tuples"])
    assert got["n_states"] == want["n_states"], (what, got["n_states"], want["n_states"])
    assert np.asarray(got["final"], F).tobytes() == np.asarray(want["final"], F).tobytes(), (what, got["final"], want["final"])
    assert len(got["arcs"]) == len(want["arcs"]), (what, len(got["arcs"]), len(want["arcs"]))
    for i, (x, y) in enumerate(zip(got["arcs"], want["arcs"])):
        assert tuple(int(v) for v in x[:3]) == tuple(int(v) for v in y[:3]), (what, i, x, y)
        assert F(x[3]).tobytes() == F(y[3]).tobytes() and F(x[4]).tobytes() == F(y[4]).tobytes(), (what, i, x, y)
        assert tuple(int(t) for t in x[5]) == tuple(int(t) for t in y[5]), (what, i, x, y)
