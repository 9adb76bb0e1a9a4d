"""Inputs of the forced-alignment tests: hand cases and a generator of training-graph-like inputs (what compile-train-graphs
makes of a transcript: left-to-right three-state HMM chains with self-loops, optional silence between words, alternative
pronunciations, eps-input arcs that carry the word labels), with random float weights and log-likelihoods so that equal
costs do not occur.  A case is a dict(name, graph [the CSR dict of kaldi_io.read_fst], loglikes [frames x pdfs float32],
tid2pdf [int32, indexed by transition-id, entry 0 unused], beam, retry_beam, min_active)."""
import numpy as np

INF32 = np.float32(np.inf)


def make_graph(n_states, start, arcs, finals):
    """arcs: (src, dst, ilabel, olabel, weight) in any order - kept in the given order within a state; finals: {state: weight}."""
    order = sorted(range(len(arcs)), key=lambda i: arcs[i][0])
    off = np.zeros(n_states + 1, np.int64)
    for a in arcs:
        off[a[0] + 1] += 1
    fin = np.full(n_states, INF32, np.float32)
    for s, w in finals.items():
        fin[s] = w
    col = lambda k, dt: np.asarray([arcs[i][k] for i in order], dt).reshape(-1)
    return dict(num_states=int(n_states), start=int(start), arc_offsets=np.cumsum(off), ilabel=col(2, np.int32),
                olabel=col(3, np.int32), weight=col(4, np.float32), nextstate=col(1, np.int32), final=fin)


def identity_tid2pdf(n_pdf):
    """transition-id t -> pdf t - 1 (entry 0 unused)."""
    return np.concatenate([[0], np.arange(n_pdf)]).astype(np.int32)


def case(name, graph, loglikes, tid2pdf, beam=200.0, retry_beam=0.0, min_active=20):
    return dict(name=name, graph=graph, loglikes=np.ascontiguousarray(loglikes, dtype=np.float32), tid2pdf=np.asarray(tid2pdf, np.int32),
                beam=beam, retry_beam=retry_beam, min_active=min_active)


def _ll(seed, frames, n_pdf, scale=3.0):
    return (np.random.default_rng(seed).standard_normal((frames, n_pdf)) * scale - 4.0).astype(np.float32)


def chain_graph(rng, n_states, eps_every=0, n_pdf=8):
    """A left-to-right chain of n_states states with self-loops, the last one final; every eps_every-th link is an eps arc
    (with an output label) in front of the emitting one.  Needs at least n_states - 1 - (eps links) frames."""
    arcs, w = [], lambda: np.float32(rng.uniform(0.05, 2.0))
    tid = lambda: int(rng.integers(1, n_pdf + 1))
    for s in range(n_states):
        arcs.append((s, s, tid(), 0, w()))
        if s + 1 < n_states:
            if eps_every and s % eps_every == eps_every - 1:
                arcs.append((s, s + 1, 0, 100 + s, w()))
            else:
                arcs.append((s, s + 1, tid(), 0, w()))
    return make_graph(n_states, 0, arcs, {n_states - 1: w()})


def hand_cases():
    out = []
    T2P = identity_tid2pdf(8)
    # one state, start and final, an emitting self-loop
    g = make_graph(1, 0, [(0, 0, 3, 7, 0.25)], {0: 0.5})
    for T in (1, 2, 37):
        out.append(case("one_state_T%d" % T, g, _ll(10 + T, T, 8), T2P))
    # three states, a chain with self-loops
    rng = np.random.default_rng(3)
    g = chain_graph(rng, 3)
    for T in (2, 37):
        out.append(case("three_states_T%d" % T, g, _ll(20 + T, T, 8), T2P))
    # a chain of three eps arcs in front of the first emitting arc (the initial closure), another inside, and an eps arc
    # into the only final state on the last frame; words on the eps arcs
    arcs = [(0, 1, 0, 11, 0.3), (1, 2, 0, 0, 0.7), (2, 3, 0, 12, 0.1), (3, 3, 1, 0, 0.2), (3, 4, 2, 0, 0.9), (4, 4, 3, 0, 0.4),
            (4, 5, 0, 13, 0.6), (5, 6, 0, 0, 0.35), (6, 7, 0, 0, 0.15), (7, 7, 4, 0, 0.8), (7, 8, 5, 14, 0.45), (8, 8, 6, 0, 0.55),
            (8, 9, 0, 15, 0.65)]
    g = make_graph(10, 0, arcs, {9: 0.75})
    out.append(case("eps_chains_T2", g, _ll(31, 2, 8), T2P))
    out.append(case("eps_chains_T37", g, _ll(32, 37, 8), T2P))
    # a state (3) that an eps arc reaches and a cheaper emitting arc reaches too; and one where the eps arc is cheaper
    arcs = [(0, 1, 1, 0, 0.5), (0, 2, 2, 0, 0.25), (0, 3, 3, 21, 0.125), (1, 3, 0, 22, 5.0), (2, 4, 0, 23, 0.0625), (0, 4, 4, 24, 9.0),
            (3, 3, 5, 0, 0.3), (4, 4, 6, 0, 0.2), (3, 5, 7, 0, 1.5), (4, 5, 8, 0, 1.25), (5, 5, 1, 0, 0.1)]
    g = make_graph(6, 0, arcs, {5: 0.0})
    out.append(case("eps_or_emitting", g, _ll(33, 9, 8), T2P))
    # a cycle with an eps arc that is taken on every frame: the path is longer than frames + arcs
    arcs = [(0, 1, 1, 0, 0.5), (1, 2, 0, 31, 0.25), (2, 3, 0, 0, 0.125), (3, 0, 0, 32, 0.375)]
    g = make_graph(4, 0, arcs, {3: 1.0})
    out.append(case("eps_cycle_every_frame", g, _ll(34, 12, 8), T2P))
    # two final states, the dearer token with the cheaper final weight
    arcs = [(0, 1, 1, 41, 0.5), (0, 2, 2, 42, 0.75), (1, 1, 3, 0, 0.3), (2, 2, 4, 0, 0.2)]
    g = make_graph(3, 0, arcs, {1: 6.0, 2: 0.5})
    out.append(case("two_finals", g, _ll(35, 5, 8), T2P))
    out.append(fan_in_case())
    out.append(float_rounding_case())
    return out


def fan_in_case():
    """State 71 has 70 incoming emitting arcs, from states 1..70 that the start state reaches."""
    rng = np.random.default_rng(71)
    w = lambda: np.float32(rng.uniform(0.05, 3.0))
    arcs = []
    for s in range(1, 71):
        arcs.append((0, s, 1 + s % 8, 0, w()))
        arcs.append((s, 71, 1 + (3 * s) % 8, 200 + s, w()))
    arcs.append((71, 71, 2, 0, w()))
    return case("fan_in_70", make_graph(72, 0, arcs, {71: w()}), _ll(71, 3, 8), identity_tid2pdf(8))


def float_rounding_case():
    """min_active = 2 with a beam of 1e-7: after frame 0 the tokens cost 3, 3 + 2^-23 (which rounds to the float 3), 3 + 2^-22,
    7 and 11; two float-rounded costs lie inside the beam, so the cutoff is the third smallest float-rounded cost, 3 + 2^-22,
    and the token that costs exactly that does not propagate while the one at 3 + 2^-23 does."""
    ll = _ll(72, 3, 8)
    ll[0, 0] = -2.0
    arcs = []
    for i, wt in enumerate([1.0, 1.0 + 2.0 ** -23, 1.0 + 2.0 ** -22, 5.0, 9.0]):
        s = 1 + i
        arcs.append((0, s, 1, 300 + i, np.float32(wt)))
        arcs.append((s, s, 2 + i, 0, np.float32(0.3 + 0.01 * i)))
        arcs.append((s, 6, 3 + i, 310 + i, np.float32(0.7 + 0.02 * i)))
    arcs.append((6, 6, 8, 0, np.float32(0.4)))
    return case("float_rounding", make_graph(7, 0, arcs, {6: 0.25}), ll, identity_tid2pdf(8), beam=1e-7, min_active=2)


def negative_eps_cycle_case():
    """An eps cycle of negative weight on the way: the closure never settles, the library ends it at its bound (the
    reference would not end at all - library mode only)."""
    arcs = [(0, 1, 1, 0, 0.5), (1, 2, 0, 0, 0.25), (2, 1, 0, 0, -0.5), (2, 3, 2, 0, 0.5)]
    return case("negative_eps_cycle", make_graph(4, 0, arcs, {3: 0.0}), _ll(73, 4, 8), identity_tid2pdf(8))


def tie_case():
    """Equal costs on purpose (weights and log-likelihoods are small dyadic numbers): two emitting arcs into state 2 with
    the same cost - the lower arc position (from state 0... the arc listed first in the CSR) wins; two eps arcs into the
    final states 3 and 4 with the same total - the lower state wins.  Held to library mode only."""
    arcs = [(0, 1, 1, 51, 0.5), (0, 2, 2, 52, 1.0), (1, 2, 1, 53, 0.5), (1, 1, 1, 0, 0.5), (2, 2, 1, 0, 0.5), (2, 4, 0, 54, 0.25),
            (2, 3, 0, 55, 0.25)]
    g = make_graph(5, 0, arcs, {3: 1.0, 4: 1.0})
    ll = np.full((3, 4), -1.0, np.float32)
    return case("ties", g, ll, identity_tid2pdf(4))


def generate(seed, n_words=3, n_phones=6, max_prons=2, sil_prob=0.7, frames=None, pad_to=0, beam=200.0, retry_beam=0.0,
             min_active=20, ll_scale=3.0):
    """A training-graph-like case.  Phone p (0 = silence) has three HMM states k with pdf 3 p + k, forward transition-id
    1 + 2 (3 p + k) and self-loop transition-id 2 + 2 (3 p + k).  pad_to: grow the graph to that many states with states
    that emitting arcs from the start state reach and that loop on themselves (tokens that never end)."""
    rng = np.random.default_rng(seed)
    w = lambda: np.float32(rng.uniform(0.05, 3.0))
    arcs, n = [], [1]

    def new_state():
        n[0] += 1
        return n[0] - 1

    def hmm(src, p, dst=None, olabel=0):
        """The three states of phone p from src; returns the state behind it."""
        cur = src
        for k in range(3):
            nxt = dst if (k == 2 and dst is not None) else new_state()
            arcs.append((cur, cur, 2 + 2 * (3 * p + k), 0, w()))
            arcs.append((cur, nxt, 1 + 2 * (3 * p + k), olabel if k == 0 else 0, w()))
            cur = nxt
        return cur

    node, min_frames = 0, 0
    for i in range(n_words):
        begin = new_state()
        if rng.uniform() < sil_prob:                  # optional silence: skip it by an eps arc, or take the silence phone
            arcs.append((node, begin, 0, 0, w()))
            hmm(node, 0, dst=begin)
        else:
            arcs.append((node, begin, 0, 0, w()))
        end = new_state()
        n_pron = int(rng.integers(1, max_prons + 1))
        lens = []
        for _ in range(n_pron):
            first = new_state()
            arcs.append((begin, first, 0, 1000 + i, w()))       # the word label on an eps-input arc
            phones = [int(x) for x in rng.integers(1, n_phones, size=int(rng.integers(1, 4)))]
            cur = first
            for j, p in enumerate(phones):
                cur = hmm(cur, p, dst=end if j == len(phones) - 1 else None)
            lens.append(3 * len(phones))
        min_frames += max(lens)
        node = end
    last = new_state()
    arcs.append((node, last, 0, 0, w()))
    hmm(node, 0, dst=last)                            # optional final silence
    base = n[0]
    for s in range(base, max(base, pad_to)):
        new_state()
        arcs.append((0, s, 1 + int(rng.integers(0, 6 * n_phones)), 0, np.float32(rng.uniform(0.05, 6.0))))
        arcs.append((s, s, 1 + int(rng.integers(0, 6 * n_phones)), 0, w()))
    g = make_graph(n[0], 0, arcs, {last: w()})
    n_pdf = 3 * n_phones
    tid2pdf = np.concatenate([[0], np.repeat(np.arange(n_pdf), 2)]).astype(np.int32)
    T = frames if frames is not None else min_frames + int(rng.integers(3, 12))
    ll = (rng.standard_normal((T, n_pdf)) * ll_scale - 4.0).astype(np.float32)
    return case("gen_seed%d" % seed, g, ll, tid2pdf, beam=beam, retry_beam=retry_beam, min_active=min_active)


GENERATOR_SEEDS = list(range(100, 150))


def generated_cases():
    """The committed generator seeds: beams 200 (the tools' default), and 10 with min_active 2 on every fifth."""
    out = []
    for s in GENERATOR_SEEDS:
        if s % 5 == 0:
            out.append(generate(s, n_words=2 + s % 3, beam=10.0, retry_beam=40.0, min_active=2))
        else:
            out.append(generate(s, n_words=2 + s % 3))
    return out


def write_dump(path, cases, beam, min_active, beam_delta=0.5, room=None):
    """The plain dump that tools/align_cpu_baseline.cc and tools/align_host_step.cc read: a batch that shares one tid2pdf,
    beam and min_active.  Floats are written as the decimal value of their bits.
      n_utts beam_bits min_active beam_delta_bits n_tid ll_rows ll_cols / tid2pdf / per utterance: states arcs start frames
      row0 room, the arcs "src dst ilabel olabel weight_bits", the final weights' bits / the matrix's bits, row by row."""
    bits = lambda x: int(np.asarray(x, np.float32).reshape(1).view(np.uint32)[0])
    t2p = cases[0]["tid2pdf"]
    assert all(np.array_equal(c["tid2pdf"], t2p) for c in cases)
    ll = np.concatenate([c["loglikes"] for c in cases])
    with open(path, "w") as f:
        f.write("%d %d %d %d %d %d %d\n" % (len(cases), bits(beam), min_active, bits(beam_delta), len(t2p), ll.shape[0], ll.shape[1]))
        f.write(" ".join(str(int(x)) for x in t2p) + "\n")
        row0 = 0
        for i, c in enumerate(cases):
            g, T = c["graph"], len(c["loglikes"])
            off = g["arc_offsets"]
            f.write("%d %d %d %d %d %d\n" % (g["num_states"], off[-1], g["start"], T, row0, T + 16 if room is None else room))
            for s in range(g["num_states"]):
                for a in range(off[s], off[s + 1]):
                    f.write("%d %d %d %d %d\n" % (s, g["nextstate"][a], g["ilabel"][a], g["olabel"][a], bits(g["weight"][a])))
            f.write(" ".join(str(bits(x)) for x in g["final"]) + "\n")
            row0 += T
        for row in ll.view(np.uint32):
            f.write(" ".join(str(int(x)) for x in row) + "\n")


def read_dump_result(text):
    """What the two programs print: per utterance "status cost_bits best_state path_len" and path_len lines "ilabel olabel
    graph_bits acoustic_bits".  Returns per utterance dict(status, cost, best_state, path)."""
    tok = text.split()
    out, i = [], 0
    f32 = lambda b: float(np.asarray([int(b)], np.uint32).view(np.float32)[0])
    while i < len(tok):
        st, cb, bs, n = int(tok[i]), int(tok[i + 1]), int(tok[i + 2]), int(tok[i + 3])
        i += 4
        path = []
        for _ in range(n if st == 0 else 0):
            path.append((int(tok[i]), int(tok[i + 1]), f32(tok[i + 2]), f32(tok[i + 3])))
            i += 4
        out.append(dict(status=st, cost=float(np.asarray([cb], np.uint64).view(np.float64)[0]), best_state=bs, path_len=n, path=path))
    return out
