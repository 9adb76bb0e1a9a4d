"""The case table of tests/test_gpu_ivector_shapes.py and the CPU helpers around it (no GPU import): model shapes that
reach the branches of csrc/kh_ivector.hip which the round sizes of tests/test_gpu_ivector.py never take.  The reference is
oracle/ivector_oracle.py; tests/test_ivector_cases.py asserts on the CPU that every case's "reaches" entries are true for
the kernel's constants (read from the .hip source) and that the inputs are well separated (below).

Precondition on the inputs.  The device and the oracle compute the feature chain after the CMVN and the UBM scores in
float with different summation orders, so a frame whose num_gselect-th and next posteriors nearly tie may select another
Gaussian, and a posterior near min_post may flip its pruning - legitimately.  For each case separation() measures, from the
oracle alone, delta = the largest |float32 log-likelihood - float64 recomputation (splice, LDA and scores in double from
the same normalised features)| and the two relative margins; a posterior is exp(log-likelihood) normalised, so an
error delta of the scores moves a ratio of posteriors by at most ~2 delta.  The seeds below were chosen on the CPU so that
both margins are at least 20 delta (asserted by the CPU test, for every run of the case including the second round of the
state chain).  Measured with the committed seeds ("-" = the case has no such margin: G >= I, min_post = 0 or one Gaussian;
for the cases with a state chain the worst of the plain run and the two rounds):

    case           delta     selection margin   min_post margin
    one_gauss      4.9e-6    -                  -
    item_split     4.7e-6    -                  -
    gselect_over   4.0e-6    -                  1.4e-1
    odd_dims       7.4e-6    1.6e-3             2.9e-3
    odd_k          8.5e-6    1.0e-3             1.2e-3      (seed 1236; 1234 leaves 1.3e-4 = 12 delta in the second round)
    two_waves      7.5e-6    3.3e-3             3.4e-4
    one_wave       8.0e-6    1.1e-3             1.6e-3
    max_gauss      1.0e-5    8.4e-4             1.1e-3      (seed 1236; 1234 leaves a selection margin of 1.0e-4 = 6 delta)
    max_base       5.8e-6    2.2e-3             3.1e-2
    multi_block    1.4e-5    -                  -
    lds_edge       5.8e-6    1.1e-2             1.1e-2
    lds_edge_acc   1.0e-5    2.4e-3             2.0e-2

Per-Gaussian counts: over all these runs the counts accumulated from the oracle's float32 posteriors and from the float64
recomputation differ by at most 5.2e-6 relative (odd_k, second round), with the same Gaussians at zero: COUNT_RTOL."""
import functools
import importlib
import math
import os
import re

import numpy as np

from oracle import ivector_oracle as IO

workloads = importlib.import_module("old-kaldi-git_amd.workloads")
HIP_SOURCE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "old-kaldi-git_amd", "csrc", "kh_ivector.hip")
PRIOR_OFFSET = 5.0
MARGIN_FACTOR = 20.0
COUNT_RTOL = 4 * 5.2e-6     # 4 x the measured float32-vs-float64 difference (above), for the device's other summation order
MAX_REMEMBERED = 50.0       # LimitFrames between the rounds of the state chain (as test_speaker_adaptation_state_chain)


def case(seed, base, splice, feat, I, S, lengths, reaches, adapt=False, streams=False, max_rows=None, feat_stride=None, **overrides):
    return dict(seed=seed, base=base, splice=splice, feat=feat, I=I, S=S, lengths=lengths, reaches=reaches, adapt=adapt,
                streams=streams, max_rows=max_rows, feat_stride=feat_stride, overrides=overrides)


# "reaches": facts(case) must give exactly these values (tests/test_ivector_cases.py).  The vocabulary is in facts().
CASES = {
    # I = 1, S = 1: spmv runs zero four-wide trips, qdim 1 (odd), K = 1.  With KH_IVECTOR_MAX_ROWS = 1024 every utterance is
    # a chunk of its own: work items of 512 + 1, of exactly 2 x 512, of one posting.  The posterior is exactly 1.
    "one_gauss": case(1234, 5, 1, 6, 1, 1, [513, 1024, 1], num_gselect=1, max_rows=1024,
                      reaches=dict(k_tail=True, wide=False, spmv_trips=0, spmv_tail=1, per_lane=1, gselect_padding=False,
                                   chunk_item_sizes=[[512, 1], [512, 512], [1]], all_kept=True)),
    # more than 512 postings of each Gaussian; S = 3: spmv scalar only; N = 6, K = 2: even, so `wide`, with an A quad and a
    # B row that both run past the edge.  G >= I and min_post = 0: nothing to select or prune.
    "item_split": case(1234, 5, 1, 6, 2, 3, [700, 30], num_gselect=2, min_post=0.0,
                       reaches=dict(k_tail=True, wide=True, a_quad_partial=True, spmv_trips=0, spmv_tail=3, items_max=2,
                                    gselect_padding=False, all_kept=True)),
    # num_gselect > num_gauss: the zero-padded posting slots; K = 3 and N = 15 odd: every GEMM load scalar.
    "gselect_over": case(1234, 5, 1, 6, 3, 5, [40, 9], num_gselect=5,
                         reaches=dict(k_tail=True, wide=False, spmv_trips=1, spmv_tail=1, gselect_padding=True)),
    # K = 50 = 3 x 16 + 2: the K-tail; N = 91 odd, so scalar loads (the K-tail under `wide` is multi_block's and max_base's);
    # S % 4 = 1; feat_dim 15: the feature rows are padded to a stride of 16.
    "odd_dims": case(1234, 13, 2, 15, 50, 13, [60, 37, 5], num_gselect=4, adapt=True, streams=True,
                     reaches=dict(k_tail=True, wide=False, spmv_trips=3, spmv_tail=1, dstride_pad=True, per_lane=1,
                                  period_chunks=1)),
    # K = 65: odd, one past a wave (two values in lane 0, one elsewhere); G = 16 fills s_w; period 25 > kWChunk: an estimation
    # point spans two chunks of weights outside greedy mode; N = 45.
    "odd_k": case(1236, 13, 2, 15, 65, 9, [60, 37, 5], num_gselect=16, min_post=0.01, ivector_period=25, adapt=True,
                  reaches=dict(k_tail=True, wide=False, spmv_trips=2, spmv_tail=1, per_lane=2, ragged_lanes=True, s_w_full=True,
                               period_chunks=2)),
    # S = 65: the second wave of the solve holds one lane; I = 100: two values per lane, ragged; N = 2145 odd.
    "two_waves": case(1234, 13, 1, 10, 100, 65, [45, 12], adapt=True,
                      reaches=dict(k_tail=True, wide=False, spmv_trips=16, spmv_tail=1, solve_waves=2, per_lane=2, ragged_lanes=True)),
    # S = 64: exactly one wave; N = 2080 and K = 100 even: `wide` with whole quads of A past K zero-filled.
    "one_wave": case(1234, 13, 1, 10, 100, 64, [45, 12],
                     reaches=dict(k_tail=True, wide=True, a_quad_partial=False, b_edge_mixed=False, spmv_trips=16, spmv_tail=0,
                                  solve_waves=1, per_lane=2, ragged_lanes=True)),
    # num_gauss = 64 x kMaxPerLane, num_gselect = kMaxGselect: the accepted maxima of the posterior, count and scatter kernels.
    "max_gauss": case(1236, 8, 1, 8, 2048, 6, [40, 21], num_gselect=16,
                      reaches=dict(k_tail=False, wide=False, per_lane_is_max=True, ragged_lanes=False, s_w_full=True, spmv_trips=1,
                                   spmv_tail=2)),
    # base_dim 64: every lane of the CMVN wave, the accepted maximum; no splicing; the features are a column block of a
    # wider device matrix (stride 70).  K = 20, N = 28: `wide` with a K-tail and a B row that is part wide, part scalar.
    "max_base": case(1234, 64, 0, 9, 20, 7, [33, 8], feat_stride=70,
                     reaches=dict(base_is_max=True, stride_over_base=True, k_tail=True, wide=True, b_edge_mixed=True, spmv_trips=1,
                                  spmv_tail=3, dstride_pad=True)),
    # 18 636 postings: five blocks of the count and scatter kernels reserve their positions through the same cursors; every
    # Gaussian's postings are split into work items; with KH_IVECTOR_MAX_ROWS = 700 the chunks start at non-zero rows and
    # points.  K = 12, N = 210: `wide`, K-tail, mixed B row.  G >= I and min_post = 0: nothing to select or prune.
    "multi_block": case(1234, 13, 2, 16, 12, 20, [600, 500, 450, 3], num_gselect=12, min_post=0.0, streams=True, max_rows=700,
                        reaches=dict(n_post=18636, sort_blocks=5, items_min=4, k_tail=True, wide=True, b_edge_mixed=True,
                                     gselect_padding=False, spmv_tail=0, chunks=[[0], [1], [2, 3]])),
    # the largest iVector dimension create() accepts (IvSolveKernel: static + dynamic LDS within the limit); the per-utterance
    # and the streams kernels need more and refuse / stand aside at this size - lds_edge_acc is their own edge.
    "lds_edge": case(1234, 13, 1, 12, 24, 118, [25, 11],
                     reaches=dict(solve_fits=True, solve_fits_plus_one=False, acc_fits=False, solve_waves=2, spmv_tail=2)),
    # the largest iVector dimension at which IvStatsKernel and IvStreamKernel fit (feat_dim 12, num_gselect 5)
    "lds_edge_acc": case(1234, 13, 1, 12, 24, 114, [25, 11], streams=True,
                         reaches=dict(solve_fits=True, acc_fits=True, acc_fits_plus_one=False, solve_waves=2, spmv_tail=2)),
}

# the streams-only over-limit shape: create() accepts it, OnlineIvectorStreams must refuse it at construction
STREAMS_OVER = dict(base=13, splice=1, feat=40, I=8, S=110, num_gselect=16)

# LinearCgd's exact fall-back at odd dimensions (the Jacobi sweep pairs the last index with a dummy that never rotates):
# test_exact_solve_fallback_is_solve_quadratic_problem's recipe.  At most 8 utterances: one workgroup each, 16 scratch slots.
# The oracle falls back 6 times at S = 13 and 7 times at S = 65 with these seeds (S = 65 with seed 1234: 3 times).
FALLBACK = {
    "fallback_13": dict(seed=1234, S=13, lengths=[61, 37, 45, 80, 23, 55], min_exact=3),
    "fallback_65": dict(seed=1236, S=65, lengths=[61, 37, 45, 80, 23, 55], min_exact=3),
}


def kernel_constants():
    """The constants of kh_ivector.hip the table depends on, read from the source."""
    src = open(HIP_SOURCE).read()
    out = {}
    for name in ("kGemmM", "kGemmN", "kGemmK", "kLinItem", "kSortChunk", "kMaxPerLane", "kMaxGselect", "kWChunk", "kLinTile",
                 "kJacobiPairs", "kEigSlots", "kIvThreads"):
        found = re.findall(r"constexpr int [^;]*\b%s = (\d+)" % name, src)
        assert len(found) == 1, name
        out[name] = int(found[0])
    found = re.findall(r"constexpr size_t kLdsLimit = (\d+) \* (\d+);", src)
    assert len(found) == 1
    out["kLdsLimit"] = int(found[0][0]) * int(found[0][1])
    # the static LDS the host code assumes per kernel: the expressions beside the declarations, evaluated here
    env = dict(out)
    sizes = {"double": 8, "float": 4, "int": 4, "int32_t": 4}
    for name in ("kRedLds", "kExactLds", "kStatsStaticLds", "kLinStaticLds", "kSolveStaticLds", "kStreamStaticLds"):
        found = re.findall(r"constexpr size_t %s = ([^;]+);" % name, src)
        assert len(found) == 1, name
        expr = re.sub(r"sizeof\((\w+)\)", lambda mo: str(sizes[mo.group(1)]), found[0])
        assert re.fullmatch(r"[\w\s+*()]+", expr), expr
        env[name] = out[name] = int(eval(expr, {"__builtins__": {}}, env))
    return out


def lds_need(K, D, S, G):
    """Static + dynamic LDS per workgroup of the four kernels that keep model-sized data there (bytes)."""
    tri = S * (S + 1) // 2
    acc = 8 * (tri + 5 * S + D + G * S)
    return dict(lin=K["kLinStaticLds"] + 8 * (D * S + K["kLinTile"] * D), solve=K["kSolveStaticLds"] + 8 * (tri + 5 * S),
                stats=K["kStatsStaticLds"] + acc, stream=K["kStreamStaticLds"] + acc)


def make_utts(rng, dim, lengths):
    # a per-utterance offset (the speaker/channel the iVector is there to capture)
    return [(rng.standard_normal((T, dim)) * 1.2 + rng.standard_normal(dim) * 0.5).astype(np.float32) for T in lengths]


def make_model(seed, base, splice, feat, I, S, **overrides):
    rng = np.random.default_rng(seed)
    m = workloads.make_ivector_extractor(rng, base_dim=base, splice=splice, feat_dim=feat, num_gauss=I, ivector_dim=S,
                                         prior_offset=PRIOR_OFFSET)
    m.update(overrides)
    return m, rng


@functools.lru_cache(maxsize=None)
def build(name):
    """(model, utterances, second-round utterances) of a case; shared by the tests, never modified."""
    c = CASES[name]
    m, rng = make_model(c["seed"], c["base"], c["splice"], c["feat"], c["I"], c["S"], **c["overrides"])
    utts = make_utts(rng, c["base"], c["lengths"])
    utts2 = make_utts(rng, c["base"], c["lengths"][::-1])[::-1] if c["adapt"] else None
    return m, utts, utts2


def adapt_model(m):
    return dict(m, greedy_most_recent=True, max_count=3.0)


@functools.lru_cache(maxsize=None)
def build_fallback(name):
    f = FALLBACK[name]
    S = f["S"]
    m, rng = make_model(f["seed"], 13, 2, 16, 48, S)
    scale = np.exp(np.linspace(0.0, np.log(300.0), S))            # condition number of the quadratic term ~ 1e5
    m["M"] = (np.asarray(m["M"]) * scale[None, None, :]).copy()
    m.update(greedy_most_recent=False, max_count=0.0, posterior_scale=0.5, num_cg_iters=1, ivector_period=5)
    return m, make_utts(rng, 13, f["lengths"])


@functools.lru_cache(maxsize=None)
def fallback_oracle(name):
    """(rows per utterance, number of exact solves the oracle did)."""
    m, utts = build_fallback(name)
    before = IO.STATS["exact_solves"]
    want = [IO.extract(u, m) for u in utts]
    return want, IO.STATS["exact_solves"] - before


# ---- the oracle's intermediate quantities ----------------------------------------------------------------------------
def posterior_entry_f64(ll, num_gselect, min_post):
    """hmm/posterior.cc:427-466 in double (IO.vector_to_posterior_entry is the float statement)."""
    p = np.exp(ll - ll.max())
    p /= p.sum()
    order = np.argsort(-p, kind="stable")[:min(num_gselect, len(p))]
    ent = [(int(g), p[g]) for g in order]
    while len(ent) > 1 and ent[-1][1] < min_post:
        ent.pop()
    s = sum(v for _, v in ent)
    return [(g, v / s) for g, v in ent]


def trace(X, m, cmvn_state=None):
    """What the oracle computes on the way for one utterance, restated with its own functions: the float32 log-likelihoods
    and posterior entries IO.extract uses, and a float64 recomputation (splice, LDA, scores, softmax in double from the same
    normalised features).  Returns dict(ll32, ll64 [T x I], post32, post64 = per frame [(gauss, weight incl. posterior_scale)],
    p32 [T x I] = the float32 softmax)."""
    Xn = IO.online_cmvn(X, m, cmvn_state)
    Fn = IO.splice_lda(Xn, m)
    g, mi, iv = IO.ubm_params(m)
    T = X.shape[0]
    L, R = m["splice_left"], m["splice_right"]
    idx = np.clip(np.arange(T)[:, None] + np.arange(-L, R + 1)[None, :], 0, T - 1)
    Sp = Xn.astype(np.float64)[idx].reshape(T, -1)
    lda = np.asarray(m["lda_mat"], np.float64)
    Fn64 = Sp @ lda[:, :Sp.shape[1]].T + (lda[:, -1] if lda.shape[1] == Sp.shape[1] + 1 else 0.0)
    g64, mi64, iv64 = g.astype(np.float64), mi.astype(np.float64), iv.astype(np.float64)
    ps = m["posterior_scale"]
    out = dict(ll32=[], ll64=[], post32=[], post64=[], p32=[])
    for t in range(T):
        x = Fn[t]
        ll = (g + mi @ x - 0.5 * (iv @ (x * x))).astype(np.float32)          # as IO.extract
        x64 = Fn64[t]
        ll64 = g64 + mi64 @ x64 - 0.5 * (iv64 @ (x64 * x64))
        post, _ = IO.vector_to_posterior_entry(ll, m["num_gselect"], m["min_post"])
        out["post32"].append([(gi, float(np.float32(w * np.float32(ps * 1.0)))) for gi, w in post])
        out["post64"].append([(gi, w * ps) for gi, w in posterior_entry_f64(ll64, m["num_gselect"], m["min_post"])])
        e = np.exp(ll - ll.max(), dtype=np.float32)
        out["p32"].append((e * np.float32(1.0 / np.float32(e.sum(dtype=np.float32)))).astype(np.float32))
        out["ll32"].append(ll)
        out["ll64"].append(ll64)
    for k in ("ll32", "ll64", "p32"):
        out[k] = np.stack(out[k])
    return out


def separation(tr, m):
    """(delta, selection margin, min_post margin) of a trace; a margin the case does not have is inf."""
    delta = float(np.abs(tr["ll32"].astype(np.float64) - tr["ll64"]).max())
    I = tr["p32"].shape[1]
    G = min(m["num_gselect"], I)
    srt = -np.sort(-tr["p32"].astype(np.float64), axis=1)
    sel = float(((srt[:, G - 1] - srt[:, G]) / srt[:, G - 1]).min()) if I > G else math.inf
    mp = float(m["min_post"])
    prune = float((np.abs(srt[:, 1:G] - mp) / mp).min()) if (mp > 0.0 and G > 1) else math.inf   # (the first entry is never pruned)
    return delta, sel, prune


def counts(post, I):
    """Per-Gaussian counts of an utterance from its posterior entries (AccStats skips zero weights)."""
    c = np.zeros(I)
    for ent in post:
        for gi, w in ent:
            if w != 0.0:
                c[gi] += w
    return c


@functools.lru_cache(maxsize=None)
def oracle_runs(name):
    """Every run of a case the GPU test compares with the oracle, computed once: a list of
    dict(label, model, utts, states_in (oracle states or None), want = [(rows, state_out)], traces)."""
    c = CASES[name]
    m, utts, utts2 = build(name)
    runs = []
    want = [IO.extract(u, m, None, True) for u in utts]
    runs.append(dict(label="plain", model=m, utts=utts, states_in=[None] * len(utts), want=want, traces=[trace(u, m) for u in utts]))
    if c["adapt"]:
        ma = adapt_model(m)
        w1 = [IO.extract(u, ma, None, True) for u in utts]
        runs.append(dict(label="adapt_round0", model=ma, utts=utts, states_in=[None] * len(utts), want=w1,
                         traces=[trace(u, ma) for u in utts]))
        st = []
        for _, s in w1:
            s = dict(cmvn=s["cmvn"].copy(), quad=s["quad"].copy(), lin=s["lin"].copy(), num_frames=float(s["num_frames"]))
            IO.limit_frames(s, ma, MAX_REMEMBERED)
            st.append(s)
        w2 = [IO.extract(u, ma, s, True) for u, s in zip(utts2, st)]
        runs.append(dict(label="adapt_round1", model=ma, utts=utts2, states_in=st, want=w2,
                         traces=[trace(u, ma, s["cmvn"]) for u, s in zip(utts2, st)]))
    return runs


def chunks(lengths, max_rows):
    """The chunks of utterances kh_ivector_extract_adapt forms under KH_IVECTOR_MAX_ROWS (lists of utterance indices)."""
    off = np.concatenate([[0], np.cumsum(lengths)])
    out, u0 = [], 0
    while u0 < len(lengths):
        u1 = u0 + 1
        while u1 < len(lengths) and off[u1 + 1] - off[u0] <= max_rows:
            u1 += 1
        out.append(list(range(u0, u1)))
        u0 = u1
    return out


def facts(name, K=None):
    """What a case reaches, recomputed from its sizes, the oracle's posteriors and the kernel's constants K."""
    K = K or kernel_constants()
    c = CASES[name]
    m, utts, _ = build(name)
    I, S, D, G, B = c["I"], c["S"], c["feat"], m["num_gselect"], c["base"]
    qdim = S * (S + 1) // 2
    wide = I % 2 == 0 and qdim % 2 == 0
    run = oracle_runs(name)[0]
    per_utt = [counts([[(gi, float(w != 0.0)) for gi, w in ent] for ent in tr["post32"]], I).astype(np.int64) for tr in run["traces"]]   # postings
    f = dict(
        k_tail=I % K["kGemmK"] != 0, wide=wide,
        a_quad_partial=wide and I % 4 != 0,                                   # a thread's four k straddle K: the scalar arm under `wide`
        b_edge_mixed=wide and qdim % 8 != 0 and qdim % K["kGemmN"] >= 8,      # a B row: wide pieces, then a scalar piece past N
        spmv_trips=S // 4, spmv_tail=S % 4, solve_waves=-(-S // 64),
        per_lane=-(-I // 64), per_lane_is_max=-(-I // 64) == K["kMaxPerLane"], ragged_lanes=I % 64 != 0,
        gselect_padding=G > I, s_w_full=G == K["kMaxGselect"], period_chunks=-(-m["ivector_period"] // K["kWChunk"]),
        dstride_pad=D % 4 != 0, base_is_max=B == 64, stride_over_base=(c["feat_stride"] or B) > B,
        n_post=sum(c["lengths"]) * G, sort_blocks=-(-sum(c["lengths"]) * G // K["kSortChunk"]),
    )
    need = lds_need(K, D, S, G)
    need1 = lds_need(K, D, S + 1, G)
    lim = K["kLdsLimit"]
    f.update(solve_fits=max(need["lin"], need["solve"]) <= lim, solve_fits_plus_one=max(need1["lin"], need1["solve"]) <= lim,
             acc_fits=max(need["stats"], need["stream"]) <= lim, acc_fits_plus_one=max(need1["stats"], need1["stream"]) <= lim)
    # work items of IvLinKernel: a Gaussian's postings (non-zero weights) of a chunk of utterances in pieces of kLinItem
    tot = np.sum(per_utt, 0)
    f["items_max"] = int(-(-tot.max() // K["kLinItem"]))
    f["items_min"] = int(-(-tot.min() // K["kLinItem"]))
    f["all_kept"] = bool(all((p.sum() == T * min(G, I)) for p, T in zip(per_utt, c["lengths"])))     # nothing pruned, no weight of zero
    if c["max_rows"]:
        f["chunks"] = chunks(c["lengths"], c["max_rows"])
        f["chunk_item_sizes"] = []       # of the Gaussian with the most postings, per chunk
        for members in f["chunks"]:
            n = int(sum(per_utt[u] for u in members).max())
            f["chunk_item_sizes"].append([min(K["kLinItem"], n - o) for o in range(0, n, K["kLinItem"])])
    return f
