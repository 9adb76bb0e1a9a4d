"""The lazy schedule's final backward pass (FinalBackward in csrc/kh_decoder.hip) at the smallest shapes at which its
visit loop can go wrong.  A dense visit reads the emitting links' destinations first - eight slots per lane in one round,
the rest of a larger frame in a remainder loop - resolves them against the hand-off map, reads link_src / link_k only of
the survivors, and requests the next frame's destinations a visit ahead.  Every case is held bit-exact to the oracle's raw
lattice and best path (run_case of test_gpu_decoder.py), and asserts on the decoder's own counters that it reached the
path it is for.

The per-frame slot counts are not an output of the decoder; they follow from its counters over PREFIXES of one score
matrix (a frame's expansion depends on the scores up to it only, and the lazy schedule leaves the arenas unpruned):
with M(T) = candidates_materialised and L(T) = counters()["num_links"] (link arena slots in use) after T frames, frame
f's emitting block has M(f + 1) - M(f) slots and starts at slot L(f) for f >= 1 (the arena holds, in order, epsilon
block 0, emitting block 0, epsilon block 1, ...), and epsilon block f has (L - M)(f) - (L - M)(f - 1) slots.

All five cases of the list are here, the epsilon-heavy one (more epsilon link slots than threads in a frame) included:
make_hclg_like's eps_frac produces it at a few thousand tokens per frame."""
import importlib

import numpy as np
import pytest
import torch

from oracle import binding as B
from test_gpu_decoder import assert_same_best_path, assert_same_lattice, graph_like_hclg, run_case

pytestmark = pytest.mark.gpu
workloads = importlib.import_module("old-kaldi-git_amd.workloads")

NT = 1024            # threads of a decoder workgroup (csrc/kh_decoder_types.h KH_NT)
SLOTS_UP_FRONT = 8   # link slots per lane of a dense visit's first round (kBU * kFinalPre in FinalBackward)
DENSE_TOKENS = 12288  # tokens of the largest frame a visit keeps in LDS (kFinalDense)


def prefix_slots(api, graph, ll, cfg, Ts, **kw):
    """(M, L, N) for the prefixes ll[:T], T in Ts - M and L of the docstring, N = token arena slots in use (the tokens of
    frames 0 .. T) - from one batch, no lattice built."""
    dec = api.LatticeFasterDecoder(api.Fst(graph), cfg, max_batch=len(Ts), max_frames=max(Ts), **kw)
    off = np.concatenate([[0], np.cumsum(Ts)]).astype(np.int32)
    dec.decode(torch.from_numpy(np.concatenate([ll[:T] for T in Ts], 0)).cuda(), off)
    M = [dec.search_counters(u)["candidates_materialised"] for u in range(len(Ts))]
    L = [dec.counters(u)["num_links"] for u in range(len(Ts))]
    N = [dec.counters(u)["num_tokens"] for u in range(len(Ts))]
    return np.array(M, np.int64), np.array(L, np.int64), np.array(N, np.int64)


@pytest.mark.parametrize("rule", ["reference", "canonical"])
def test_utterances_of_one_two_and_three_frames(api, rule):
    """One visit with nothing requested ahead, the first request ahead, a request ahead that follows one; blocks of every
    length mod 4 (the 16-byte access and its tail) and a block that does not start on a multiple of 4."""
    kw = {} if rule == "reference" else dict(exact_reference_order=False)
    cfg = api.decoder_config(beam=10.0, lattice_beam=6.0)
    lengths, starts = set(), set()
    for seed in range(101, 107):
        rng = np.random.default_rng(seed)
        g = graph_like_hclg(rng, 3000, 50)
        ll = workloads.make_loglikes(rng, 3, 50)
        dec = run_case(api, g, [ll[:1], ll[:2], ll], cfg, rules=(rule,))
        for u, T in enumerate((1, 2, 3)):
            c = dec.schedule_counters(u)
            assert c["dense_final_visits"] == T and c["general_final_visits"] == 0, (seed, u, c)
        M, L, _ = prefix_slots(api, g, ll, cfg, (1, 2, 3), **kw)
        lengths |= {int(M[0]) % 4, int(M[1] - M[0]) % 4, int(M[2] - M[1]) % 4}
        starts |= {int(L[0]) % 4, int(L[1]) % 4}
    assert lengths == {0, 1, 2, 3}, lengths
    assert starts - {0}, starts


@pytest.mark.parametrize("rule", ["reference", "canonical"])
def test_more_slots_than_the_first_round_and_every_route(api, rule):
    """The dense-graph shape of test_lazy_schedule_large_frames_and_many_survivors, the first 13 frames of its first utterance: frames of more
    link slots than a visit requests up front (the remainder loop, next to a request ahead), a dense visit directly after
    a general one (extra_costs through memory, nothing requested ahead) and directly after a hand-off through memory."""
    kw = {} if rule == "reference" else dict(exact_reference_order=False)
    rng = np.random.default_rng(79)
    g = graph_like_hclg(rng, 300000, 300)
    ll = workloads.make_loglikes(rng, 45, 300)[:13]   # (that utterance's first 13 frames: 9 dense visits, 4 general ones)
    cfg = api.decoder_config(beam=13.0, max_active=2147483647, min_active=200, lattice_beam=11.0)
    dec = run_case(api, g, [ll], cfg, rules=(rule,))
    c = dec.schedule_counters(0)
    assert c["general_final_visits"] > 0 and c["handoffs_through_memory"] > 0 and c["dense_final_visits"] > 0, c
    # a DENSE frame (at most 12288 tokens: the search is still widening) with more slots than the first round covers
    Ts = tuple(range(1, 14))
    M, _, N = prefix_slots(api, g, ll, cfg, Ts, **kw)
    tokens = np.diff(N)        # tokens of frames 2 .. 13
    slots = np.diff(M)[1:]     # emitting link slots of frames 2 .. 12
    assert ((tokens[:-1] <= DENSE_TOKENS) & (slots > NT * SLOTS_UP_FRONT)).any(), (tokens, slots)


def test_converted_frames_below_fresh_ones(api, monkeypatch):
    """The small arenas of test_lazy_schedule_collects_garbage_when_the_arenas_fill_up: the slot prunes and compacts on the
    way, so the walk crosses from frames whose links still carry tot_cost to converted ones."""
    monkeypatch.setenv("KH_DECODER_ARENA_GB", "0")
    monkeypatch.setenv("KH_DECODER_SLOTS", "1")
    monkeypatch.setenv("KH_DECODER_TOKENS_PER_FRAME", "8192")
    monkeypatch.setenv("KH_DECODER_WINDOW_TOKENS_PER_FRAME", "256")
    monkeypatch.setenv("KH_DECODER_STABLE_TOKENS_PER_FRAME", "16")
    rng = np.random.default_rng(78)
    g = graph_like_hclg(rng, 50000, 400)
    lls = [workloads.make_loglikes(rng, 300, 400)]
    dec = run_case(api, g, lls, api.decoder_config(beam=11.0, max_active=900, min_active=100, lattice_beam=5.0), rules=("reference",))
    c = dec.schedule_counters(0)
    assert c["garbage_collections"] >= 1 and c["dense_final_visits"] > 0, c


def test_more_epsilon_link_slots_than_threads(api):
    """An epsilon-heavy graph: frames whose epsilon block has more than NT slots relax it from memory, a barrier per round."""
    rng = np.random.default_rng(83)
    g = graph_like_hclg(rng, 20000, 100, eps_frac=0.5)
    ll = workloads.make_loglikes(rng, 24, 100)
    cfg = api.decoder_config(beam=12.0, max_active=6000, min_active=200, lattice_beam=7.0)
    dec = run_case(api, g, [ll], cfg, rules=("reference",))
    c = dec.schedule_counters(0)
    assert c["dense_final_visits"] == 24 and c["general_final_visits"] == 0, c
    Ts = (21, 22, 23)
    M, L, _ = prefix_slots(api, g, ll, cfg, Ts)
    eps_blocks = np.diff(L - M)    # epsilon blocks of frames 22 and 23, both visited by the 24-frame walk
    assert eps_blocks.max() > NT, eps_blocks


def test_lazy_online_stream_in_random_chunks(api):
    """One lazy online stream fed in random chunks and finalized (OnlineKernel's FinalBackward), compared as
    test_gpu_online_decoder.py compares: the oracle's lattice, the offline decoder's, best path and statistics."""
    rng = np.random.default_rng(85)
    g = workloads.make_hclg_like(rng, 8000, 60)
    cfg = api.decoder_config(beam=11.0, max_active=1500, min_active=100, lattice_beam=6.0, prune_interval=9)
    fst = api.Fst(g)
    T = 131
    ll = workloads.make_loglikes(rng, T, 60)
    dev = torch.from_numpy(ll).cuda()
    lazy = api.LatticeFasterOnlineDecoder(fst, cfg, num_streams=1, max_frames=160)
    lazy.set_lazy_prune(True)
    lazy.init_decoding([0])
    fed = 0
    while fed < T:
        k = int(min(T - fed, rng.integers(0, 30)))
        lazy.advance_decoding([0], [dev[fed:fed + k]])
        fed += k
        assert lazy.num_frames_decoded(0) == fed
    lazy.finalize_decoding([0])
    offline = api.LatticeFasterDecoder(fst, cfg, max_batch=1, max_frames=T)
    offline.decode(dev, np.array([0, T], np.int32))
    assert offline.schedule_counters(0)["dense_final_visits"] == T
    oc = B.DecoderOracle(g, cfg, "reference")
    assert oc.decode(ll)
    got = lazy.get_raw_lattice(0)
    assert_same_lattice(got, oc.raw_lattice())
    assert_same_lattice(got, offline.get_raw_lattice(0))
    assert_same_best_path(lazy.get_best_path(0), oc.best_path())
    so, sg = oc.stats(), lazy.stats(0)
    for k in ("num_frames", "reached_final", "num_tokens", "num_links", "tokens_created", "max_tokens_frame"):
        assert so[k] == sg[k], (k, so[k], sg[k])
    assert np.float32(so["final_relative_cost"]).tobytes() == np.float32(sg["final_relative_cost"]).tobytes()
