"""Wide lattices for the lattice kernels' form tests (test_lattice_cases.py asserts their preconditions without a GPU,
test_gpu_lattice_forms.py runs them).  random_lattice (test_lattice_oracle.py) makes frames of at most `width` <= 7 states: an
arc spans ~14 states and a dependency level holds 7.  wide_lattice makes frames of W states, so that arcs span more states
than an LDS window has slots, a level is wider than a workgroup, and a 64-state block has more arcs than a staging area."""
import numpy as np

# name: (T, W, fan, eps_per_frame, window slots the shape is meant to overrun)
SHAPES = {
    "far256": (5, 320, 3, 200, 256),
    "far1024": (4, 1100, 3, 600, 1024),
    "far8192": (4, 7000, 2, 3000, 8192),
    "dense": (4, 1300, 8, 600, 256),
}
SEEDS = {"far256": 256, "far1024": 1024, "far8192": 8192, "dense": 1300}


def _csr(n, src, dst, il, g, a, final):
    order = np.lexsort((dst, src))           # by (source, destination); equal pairs keep their order
    src, dst, il, g, a = src[order], dst[order], il[order], g[order], a[order]
    off = np.zeros(n + 1, np.int64)
    off[1:] = np.cumsum(np.bincount(src, minlength=n))
    return dict(n_states=int(n), arc_offsets=off, arc_ilabel=il.astype(np.int32), arc_nextstate=dst.astype(np.int32),
                arc_graph=g.astype(np.float32), arc_acoustic=a.astype(np.float32), state_final=final.astype(np.float32))


def wide_lattice(rng, T, W, fan, eps_per_frame):
    """State 0, then T frames of W states (frame t = states 1 + (t - 1) W ... t W).  Every state but the last frame's has `fan`
    emitting arcs to random states of the next frame; every state of a frame has one more incoming arc from a random state
    of the frame before (so all are reachable); eps_per_frame epsilon arcs per frame go from a lower to a higher state of
    it.  Labels 1 ... 49, costs uniform in [0, 3), epsilon arcs have acoustic cost 0; the last frame is final; arcs sorted by
    (source, destination).  Top-sorted and time-synchronous: a state of frame t has time t."""
    n = 1 + T * W
    first = lambda t: 1 + (t - 1) * W                       # first state of frame t >= 1
    src, dst = [], []
    for t in range(T):                                      # emitting arcs frame t -> t + 1 (frame 0 = state 0)
        states = np.arange(first(t), first(t) + W) if t > 0 else np.zeros(1, np.int64)
        src.append(np.repeat(states, fan))
        dst.append(first(t + 1) + rng.integers(0, W, len(states) * fan))
        nxt = np.arange(first(t + 1), first(t + 1) + W)     # one more incoming arc for every state of frame t + 1
        src.append(states[rng.integers(0, len(states), W)])
        dst.append(nxt)
    n_emit = sum(len(x) for x in src)
    for t in range(1, T + 1):                               # epsilon arcs inside frame t, lower -> higher
        a, b = rng.integers(0, W, eps_per_frame), rng.integers(0, W - 1, eps_per_frame)
        b = np.where(b >= a, b + 1, b)                      # b != a, uniform
        src.append(first(t) + np.minimum(a, b))
        dst.append(first(t) + np.maximum(a, b))
    src, dst = np.concatenate(src).astype(np.int64), np.concatenate(dst).astype(np.int64)
    m = len(src)
    il = rng.integers(1, 50, m)
    il[n_emit:] = 0
    g, a = rng.random(m) * 3.0, rng.random(m) * 3.0
    a[n_emit:] = 0.0
    final = np.full(n, np.inf)
    final[first(T):] = rng.random(W) * 2.0
    return _csr(n, src, dst, il, g, a, final)


def make(name):
    """The named shape, from its own fixed seed."""
    T, W, fan, eps, _ = SHAPES[name]
    return wide_lattice(np.random.default_rng(SEEDS[name]), T, W, fan, eps)


def arc_sources(L):
    return np.repeat(np.arange(L["n_states"], dtype=np.int64), np.diff(np.asarray(L["arc_offsets"], np.int64)))


def add_arc(L, s, d, ilabel, graph, acoustic):
    """A copy of L with one more arc s -> d, kept sorted by (source, destination) (after the equal pairs)."""
    src = np.concatenate([arc_sources(L), [s]])
    cat = lambda k, v: np.concatenate([np.asarray(L[k]), [v]])
    return _csr(L["n_states"], src, cat("arc_nextstate", d).astype(np.int64), cat("arc_ilabel", ilabel), cat("arc_graph", graph),
                cat("arc_acoustic", acoustic), np.asarray(L["state_final"]))


def levels(L):
    """Dependency level of every state: the longest distance from a state without incoming arcs."""
    src, dst = arc_sources(L), np.asarray(L["arc_nextstate"], np.int64)
    lv = np.zeros(L["n_states"], np.int64)
    for _ in range(L["n_states"] + 1):
        nl = lv.copy()
        np.maximum.at(nl, dst, lv[src] + 1)
        if np.array_equal(nl, lv):
            return lv
        lv = nl
    raise ValueError("the lattice has a cycle")


def facts(L, slots):
    """What a lattice makes the kernels do: states, arcs; the share of arcs that span more than `slots` states (their operand
    has left a window of that many slots) and fewer than 64; per block of 64 consecutive states the largest number of incoming
    and of outgoing arcs and the number of blocks over 384 and over 192 (the staging areas); the widest dependency level."""
    n = L["n_states"]
    src, dst = arc_sources(L), np.asarray(L["arc_nextstate"], np.int64)
    span = dst - src
    n_blk = (n + 63) // 64
    inc, out = np.bincount(dst // 64, minlength=n_blk), np.bincount(src // 64, minlength=n_blk)
    return dict(states=n, arcs=len(src), far=float((span > slots).mean()), near=float((span < 64).mean()),
                max_in_block=int(inc.max()), max_out_block=int(out.max()),
                in_blocks_over_384=int((inc > 384).sum()), out_blocks_over_384=int((out > 384).sum()),
                in_blocks_over_192=int((inc > 192).sum()), out_blocks_over_192=int((out > 192).sum()),
                widest_level=int(np.bincount(levels(L)).max()))
