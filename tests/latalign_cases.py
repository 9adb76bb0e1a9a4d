"""A toy model and lattices for the word-alignment tests (test_lattice_align_words.py, test_gpu_lattice_align_words.py).

Topology: every phone a 3-state left-to-right HMM; HMM-state h of phone p has two transitions, the self-loop and the one
forward, transition-id 1 + ((p - 1) * 3 + h) * 2 + (0 self-loop | 1 forward); the forward transition of state 2 enters the
topology entry's last state, so it is the IsFinal one.  Phones: 1 silence (nonword); 2, 6 word-begin; 3, 7 word-internal;
4, 8 word-end; 5, 9 singleton."""
import numpy as np

F = np.float32
N_PHONES = 9
PHONE_TYPE = np.asarray([0, 5, 1, 4, 2, 3, 1, 4, 2, 3], np.int32)     # restatement's NO, BEGIN, END, SINGLETON, INTERNAL, NONWORD
LEXICON = {10: [2, 4], 11: [2, 3, 4], 12: [5], 13: [6, 7, 7, 8], 14: [9], 15: [6, 8], 16: [2, 8]}
SIL = 1


def tid(p, h, forward):
    return 1 + ((p - 1) * 3 + h) * 2 + (1 if forward else 0)


def tmodel():
    n = N_PHONES * 6
    phone, fin, loop = np.zeros(n + 1, np.int32), np.zeros(n + 1, bool), np.zeros(n + 1, bool)
    for p in range(1, N_PHONES + 1):
        for h in range(3):
            for fw in (0, 1):
                t = tid(p, h, fw)
                phone[t], fin[t], loop[t] = p, bool(fw and h == 2), not fw
    return dict(tid2phone=phone, tid_is_final=fin, tid_is_self_loop=loop)


def wbinfo(reorder=False, silence_label=0, partial_word_label=0):
    return dict(phone_to_type=PHONE_TYPE.copy(), reorder=reorder, silence_label=silence_label, partial_word_label=partial_word_label)


def phone_ali(p, loops=(0, 0, 0), reorder=False):
    """The transition-ids of one phone: loops[h] self-loops in HMM-state h; reorder puts a state's self-loops behind the
    forward transition that entered it, i.e. behind the forward transition of the same state in this numbering."""
    out = []
    for h in range(3):
        if reorder:
            out += [tid(p, h, 1)] + [tid(p, h, 0)] * loops[h]
        else:
            out += [tid(p, h, 0)] * loops[h] + [tid(p, h, 1)]
    return out


def word_ali(phones, extra=0, reorder=False, rng=None):
    loops = [[0, 0, 0] for _ in phones]
    for k in range(extra):
        i = rng.integers(len(phones) * 3) if rng is not None else k % (len(phones) * 3)
        loops[i // 3][i % 3] += 1
    out = []
    for p, lp in zip(phones, loops):
        out += phone_ali(p, lp, reorder)
    return out


def clat(n_states, arcs, finals, start=0):
    """arcs: (src, dst, label, g, a, tids); finals: {state: (g, a, tids)}."""
    fg, fa = np.full(n_states, np.inf, F), np.full(n_states, np.inf, F)
    fs = [np.zeros(0, np.int32) for _ in range(n_states)]
    for s, (g, a, t) in finals.items():
        fg[s], fa[s], fs[s] = g, a, np.asarray(t, np.int32)
    arcs = sorted(arcs, key=lambda x: x[0])
    return dict(n_states=n_states, start=start, arc_src=np.asarray([x[0] for x in arcs], np.int32),
                arc_dst=np.asarray([x[1] for x in arcs], np.int32), arc_label=np.asarray([x[2] for x in arcs], np.int32),
                arc_g=np.asarray([x[3] for x in arcs], F), arc_a=np.asarray([x[4] for x in arcs], F),
                arc_string=[np.asarray(x[5], np.int32) for x in arcs], final_g=fg, final_a=fa, final_string=fs)


def linear(reorder=False):
    """silence, the two-phone word 10, the singleton word 12, silence: one arc each, every boundary at an arc's end."""
    s = lambda: phone_ali(SIL, (1, 0, 2), reorder)
    return clat(5, [(0, 1, 0, 0.5, 1.25, s()), (1, 2, 10, 1.0, 2.5, word_ali(LEXICON[10], 2, reorder)),
                    (2, 3, 12, 0.25, 0.75, word_ali(LEXICON[12], 1, reorder)), (3, 4, 0, 0.125, 3.0, s())], {4: (0.0, 0.0, [])})


def boundary_inside_and_at_end():
    """Two arcs 0 -> 1 of 9 transition-ids each: word 10 whole, its boundary at the arc's end (not known before the next arc
    is seen), and word 12 followed by a silence, the boundary inside the arc.  State 1 is reached with two pending
    contents: word 10's ids and label, and the silence's ids without a label."""
    w10 = word_ali(LEXICON[10], 3)
    w12sil = word_ali(LEXICON[12]) + phone_ali(SIL, (1, 1, 1))
    return clat(4, [(0, 1, 10, 1.0, 1.0, w10), (0, 1, 12, 0.5, 2.0, w12sil), (1, 2, 14, 0.25, 0.5, word_ali(LEXICON[14])),
                    (2, 3, 0, 0.0, 0.5, phone_ali(SIL))], {3: (1.5, 0.5, [])})


def dedupe():
    """Two paths 0 -> 1 -> 3 and 0 -> 2 -> 3 with the same words and the same transition-ids cut at different places: the
    tuples on state 3 coincide."""
    w = word_ali(LEXICON[11], 2)
    return clat(5, [(0, 1, 11, 1.0, 0.5, w[:4]), (0, 2, 11, 0.75, 0.25, w[:4]), (1, 3, 0, 0.5, 0.5, w[4:]), (2, 3, 0, 2.0, 0.125, w[4:]),
                    (3, 4, 12, 0.25, 0.25, word_ali(LEXICON[12]))], {4: (0.0, 0.0, [])})


def plus_merges():
    """Not deterministic.  (a) Two epsilon paths to the same tuple: parallel arcs with the same label and string and
    different weights (0 -> 1, and two of 2 -> 3).  (b) Two arcs of one output state with the same label and destination:
    word 12's label and first transition-id sit on arc 1 -> 2, so the output state behind word 10 is on state 2; from there
    two alignments of word 12 of the same length and weight lead to the same tuple behind it, and Compare has to go to the
    strings."""
    w = word_ali(LEXICON[10], 1)
    v, v2 = phone_ali(5, (0, 1, 0)), phone_ali(5, (0, 0, 1))
    return clat(5, [(0, 1, 10, 1.0, 2.0, w[:3]), (0, 1, 10, 0.5, 2.25, w[:3]), (1, 2, 12, 0.25, 0.25, w[3:] + v[:1]),
                    (2, 3, 0, 1.0, 1.0, v[1:]), (2, 3, 0, 0.5, 1.25, v[1:]), (2, 3, 0, 0.5, 1.25, v2[1:]),
                    (3, 4, 0, 0.0, 0.0, phone_ali(SIL))], {4: (0.0, 0.0, [])})


def several_finals():
    """Two final states with weights other than One and final strings: state 1 ends with a long silence in its final string;
    state 2 lies behind one more word, the first id of the closing silence on the arc and the rest in the final string."""
    w10, w12, s = word_ali(LEXICON[10]), word_ali(LEXICON[12], 2), phone_ali(SIL, (0, 1, 0))
    return clat(3, [(0, 1, 10, 1.0, 1.0, w10), (1, 2, 12, 0.5, 0.5, w12 + s[:1])],
                {1: (0.25, 0.75, phone_ali(SIL, (2, 2, 2))), 2: (2.0, 1.0, s[1:])})


def shortcut():
    """A single final state with weight One and no arcs: CreateSuperFinal adds nothing; the last word cannot be known to
    have ended, so it is forced out without an error."""
    return clat(2, [(0, 1, 10, 1.0, 1.0, word_ali(LEXICON[10], 1))], {1: (0.0, 0.0, [])})


def forced_partial_word():
    return clat(2, [(0, 1, 0, 1.0, 1.0, word_ali(LEXICON[10])[:4])], {1: (0.0, 0.0, [])})


def forced_words_without_ids():
    return clat(3, [(0, 1, 12, 1.0, 1.0, word_ali(LEXICON[12])), (1, 2, 14, 0.5, 0.25, [])], {2: (0.0, 0.0, [])})


def forced_silence_not_finished():
    return clat(2, [(0, 1, 0, 1.0, 1.0, phone_ali(SIL)[:2])], {1: (0.0, 0.0, [])})


def fatal_broken_silence():
    """Silence that never reaches its final transition, followed by another phone's ids: OutputSilenceArc never fires, and
    OutputArcForce sees the phone change."""
    return clat(2, [(0, 1, 0, 1.0, 1.0, phone_ali(SIL)[:2] + phone_ali(5)[:1])], {1: (0.0, 0.0, [])})


def silence_run(k):
    """One arc with k silences in a row and the single final state: k + 3 tuples on 2 states and 1 arc, far more than the
    first room of the device tables (4 (states + arcs) + 64), every pending string a suffix of the arc's."""
    return clat(2, [(0, 1, 0, 1.0, 2.0, phone_ali(SIL) * k)], {1: (0.0, 0.0, [])})


def empty():
    return dict(n_states=0, start=-1, arc_src=np.zeros(0, np.int32), arc_dst=np.zeros(0, np.int32), arc_label=np.zeros(0, np.int32),
                arc_g=np.zeros(0, F), arc_a=np.zeros(0, F), arc_string=[], final_g=np.zeros(0, F), final_a=np.zeros(0, F), final_string=[])


def inconsistent_times():
    w = word_ali(LEXICON[12])
    return clat(3, [(0, 1, 12, 1.0, 1.0, w), (0, 2, 12, 1.0, 1.0, w + phone_ali(SIL)), (1, 2, 0, 0.0, 0.0, phone_ali(SIL, (1, 0, 0)))],
                {2: (0.0, 0.0, [])})


def generate(seed, n_nodes=None, reorder=False):
    """Lexicon words (with optional silence in front) laid over a random word graph with consistent times, then
    transition-ids shifted across arc boundaries as determinization does: at a node with one incoming arc the arc's last k
    ids move to the front of every outgoing arc (and of the final string); at a node with one outgoing arc and no final
    weight that arc's first k ids move to the end of every incoming arc.  Every path keeps its transition-id sequence."""
    rng = np.random.default_rng(seed)
    n = int(n_nodes if n_nodes is not None else rng.integers(2, 8))
    t = np.concatenate([[0], np.cumsum(rng.integers(6, 18, n - 1))])
    arcs = []
    for i in range(n - 1):
        used = set()                      # deterministic on words: the arcs out of one node carry different words
        for j in (i + 1, i + 2):
            if j >= n or (j == i + 2 and rng.random() < 0.5):
                continue
            for _ in range(int(rng.integers(1, 3))):
                dur = int(t[j] - t[i])
                sil = dur >= 9 and rng.random() < 0.4
                room = dur - (3 if sil else 0)
                words = [w for w, ph in LEXICON.items() if 3 * len(ph) <= room and w not in used]
                if not words:
                    continue
                w = int(rng.choice(words))
                used.add(w)
                ids = (phone_ali(SIL, (0, 0, 0), reorder) if sil else []) + word_ali(LEXICON[w], room - 3 * len(LEXICON[w]), reorder, rng)
                arcs.append([i, j, w, F(rng.integers(0, 64)) / F(8), F(rng.integers(0, 256)) / F(16), ids])
    finals = {n - 1: [F(rng.integers(0, 8)) / F(4), F(rng.integers(0, 8)) / F(2), []]}
    for v in rng.permutation(np.arange(1, n)):
        inc = [a for a in arcs if a[1] == v]
        out = [a for a in arcs if a[0] == v]
        if len(inc) == 1 and len(inc[0][5]) > 1 and rng.random() < 0.7:
            k = int(rng.integers(1, len(inc[0][5])))
            moved, inc[0][5] = inc[0][5][-k:], inc[0][5][:-k]
            for a in out:
                a[5] = moved + a[5]
            if v in finals:
                finals[v][2] = moved + finals[v][2]
        elif len(out) == 1 and v not in finals and len(out[0][5]) > 1 and rng.random() < 0.7:
            k = int(rng.integers(1, len(out[0][5])))
            moved, out[0][5] = out[0][5][:k], out[0][5][k:]
            for a in inc:
                a[5] = a[5] + moved
    return clat(n, [tuple(a) for a in arcs], {s: tuple(f) for s, f in finals.items()})


SEEDS = (11, 12, 13, 14, 15)


def batch(seed, count=40):
    """count lattices of mixed sizes from one seed."""
    return [generate(seed * 1000 + i, n_nodes=2 + (i * 7) % 6) for i in range(count)]


def write_model(path):
    """The toy TransitionModel as a binary model file (what lattice-align-words reads as its second argument)."""
    from conftest import pkg
    kio = pkg("kaldi_io")
    entry = [(0, [(0, 0.5), (1, 0.5)]), (1, [(1, 0.5), (2, 0.5)]), (2, [(2, 0.5), (3, 0.5)]), (-1, [])]
    topo = dict(phones=list(range(1, N_PHONES + 1)), phone2idx=[-1] + [0] * N_PHONES, entries=[entry])
    triples = [(p, h, (p - 1) * 3 + h) for p in range(1, N_PHONES + 1) for h in range(3)]
    log_probs = np.concatenate([[0.0], np.log(np.full(N_PHONES * 6, 0.5))]).astype(np.float32)
    with open(path, "wb") as f:
        f.write(b"\0B")
        kio.write_transition_model(f, topo, triples, log_probs, True)
    return str(path)


def write_word_boundary(path):
    names = {1: "begin", 2: "end", 3: "singleton", 4: "internal", 5: "nonword"}
    with open(path, "w") as f:
        for p in range(1, N_PHONES + 1):
            f.write("%d %s\n" % (p, names[int(PHONE_TYPE[p])]))
    return str(path)
