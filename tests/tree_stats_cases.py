"""Cases for the tree-statistics tests (test infrastructure).

A tiny model: phone 1 (silence) has three emitting states of pdf-classes 0, 1, 2, phones 2 ... 4 share an entry of two
emitting states of pdf-classes 0 and 1; every emitting state has a self-loop and a forward transition, the last one's into
the final state.  Alignments are drawn for a phone sequence in both layouts of a transition-id sequence: not reordered (the
self-loops of a state, then its forward transition) and reordered (the forward transition, then the self-loops).

Kernel cases are (feats, frame_event, num_events): runs of chosen lengths whose frames are interleaved, so that the order
inside an event is the ascending frame order and nothing else.  The order-sensitive cases put magnitudes into one event
whose double sums round differently in another order (3e17, 0.3, -3e17 for the first-order row; 1e8 and then values
below 1 for the second-order row: a square of 1e16 has passed 2^53, so each small square is lost after it and kept before it), and sensitive() shows on the CPU that the restatement tells both mistakes apart: the
frames reversed, and double products in place of float-rounded ones."""
import numpy as np

import tree_stats_restatement as R

TOPO = dict(phones=[1, 2, 3, 4], phone2idx=[-1, 0, 1, 1, 1],
            entries=[[(0, [(0, 0.5), (1, 0.5)]), (1, [(1, 0.5), (2, 0.5)]), (2, [(2, 0.5), (3, 0.5)]), (-1, [])],
                     [(0, [(0, 0.5), (1, 0.5)]), (1, [(1, 0.5), (2, 0.5)]), (-1, [])]])
TRIPLES = [(1, 0, 0), (1, 1, 1), (1, 2, 2), (2, 0, 3), (2, 1, 4), (3, 0, 5), (3, 1, 6), (4, 0, 7), (4, 1, 8)]
NUM_TIDS = 2 * len(TRIPLES)


def tables():
    return R.Tables(TOPO, TRIPLES)


def model_bytes(kio):
    """The transition model as a binary file's bytes, followed by bytes nobody may read."""
    import io
    f = io.BytesIO()
    f.write(b"\0B")
    log_probs = np.concatenate([[0.0], np.log(np.full(NUM_TIDS, 0.5))]).astype(np.float32)
    kio.write_transition_model(f, TOPO, TRIPLES, log_probs, True)
    f.write(b"<NotAnAmDiagGmm> only the transition model is read")
    return f.getvalue()


def product_model(kio):
    import io
    s = kio.Stream(io.BytesIO(model_bytes(kio)))
    assert kio.init_kaldi_input(s)
    return kio.read_transition_model(s, True)


def tids_of(phone, hmm_state):
    """(self-loop, forward) transition-ids of a (phone, HMM-state): two per triple, in triple order."""
    k = [t[:2] for t in TRIPLES].index((phone, hmm_state))
    return 2 * k + 1, 2 * k + 2


def alignment(phones, durations, reordered):
    """The transition-ids of a phone sequence; durations[i][s] >= 1 frames in state s of phone i."""
    out = []
    for phone, dur in zip(phones, durations):
        for s, d in enumerate(dur):
            loop, fwd = tids_of(phone, s)
            out += [fwd] + [loop] * (d - 1) if reordered else [loop] * (d - 1) + [fwd]
    return out


def random_alignment(rng, n_phones, reordered, max_dur=4):
    phones = [int(p) for p in rng.integers(1, 5, n_phones)]
    durations = [[int(d) for d in rng.integers(1, max_dur + 1, 3 if p == 1 else 2)] for p in phones]
    return phones, alignment(phones, durations, reordered)


def features(rng, T, D):
    """float32 rows over six decades, both signs: sums that round."""
    return (rng.standard_normal((T, D)) * 10.0 ** rng.uniform(-3, 3, (T, D))).astype(np.float32)


def kernel_case(rng, D, runs, unused=0):
    """Events e = 0 ... len(runs) - 1 of runs[e] frames, and `unused` frames of event -1, all interleaved."""
    fe = np.concatenate([np.full(n, e, np.int32) for e, n in enumerate(runs)] + [np.full(unused, -1, np.int32)])
    fe = fe[rng.permutation(len(fe))]
    return features(rng, len(fe), D), fe, len(runs)


def edge_runs(tile):
    return [0, 1, 2, tile - 1, tile, tile + 1, 2 * tile + 1]


ORDER_VALUES = [1e8, 1.0, -1e8, 3e17, 0.3, -3e17, 1.1, 7e-3, 2.5e8, -1.0, 1.7]        # the first-order sums round: 3e17 + 0.3
ORDER_SQUARES = [1e8, 0.9, 1.1, 0.7, -0.8, 0.3, 0.95, -0.6, 0.85, 0.75, 0.65]      # the second-order sums round: 1e16 + 0.81


def order_cases(rng):
    """name -> (feats, frame_event, num_events): the sensitive values in one event, alone and between the frames of others."""
    D = 6                                                      # every column meets one of the two lists at another phase
    x = np.stack([np.roll(np.asarray(ORDER_SQUARES if k % 2 else ORDER_VALUES, np.float32), k) for k in range(D)], 1)
    col = x[:, 0]
    alone = (x, np.zeros(len(col), np.int32), 1)
    fe = np.concatenate([np.full(len(col), 1, np.int32), np.full(40, 0, np.int32), np.full(30, 2, np.int32), np.full(9, -1, np.int32)])
    order = rng.permutation(len(fe))
    fe = fe[order]
    feats = features(rng, len(fe), D)
    feats[np.nonzero(fe == 1)[0]] = x                          # ascending frames of event 1 carry x's rows in order
    return dict(alone=alone, among_others=(feats, fe, 3))


def sensitive(case):
    """The restatement's bits change when the frames are reversed (first-order row, second-order row) and when the products
    are made in double (second-order row)."""
    feats, fe, E = case
    _, ref = R.add_stats(feats, fe, E)
    _, rev = R.add_stats(feats[::-1], fe[::-1], E)
    _, dbl = R.add_stats(feats, fe, E, double_products=True)
    bits = lambda a: np.ascontiguousarray(a).view(np.int64)
    return (bool((bits(ref[:, 0]) != bits(rev[:, 0])).any()), bool((bits(ref[:, 1]) != bits(rev[:, 1])).any()),
            bool((bits(ref[:, 1]) != bits(dbl[:, 1])).any()))


def plan_counts(fe, num_events, D):
    """frames with an event, events with a frame, work items (event with a frame x block of 64 columns), longest run."""
    runs = np.bincount(fe[fe >= 0], minlength=num_events) if num_events else np.zeros(0, np.int64)
    used = int((runs > 0).sum())
    return dict(frames=int(runs.sum()), events=used, work_items=used * ((D + 63) // 64), longest=int(runs.max()) if used else 0)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and bool((a.view(np.int64) == b.view(np.int64)).all())
