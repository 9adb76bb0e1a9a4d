#!/usr/bin/env python3
"""The scoring stage alone: best paths of the CompactLattices of a config-3-sized decode (the utterances
tools/dump_bench_lattices.py samples, determinized as the decoder's completion threads do) for the 36 score points of
local/score.sh.  python tools/bench_lattice_best_path.py [n_utterances [copies [--small]]]

 (a) one kh_compact_lattice_best_paths call with 36 points, split as kh_compact_lattice_best_paths_last_timings splits it
     (call_ms = the whole C call by the host's clock; wall_ms includes the Python packing around it);
 (b) the same lattices through 36 calls with one point each;
 (c) tools/latbest_cpu_baseline.cc (g++ -O2, one thread) run 36 times over the same arrays: what the 36 CPU jobs of
     score.sh compute, minus their I/O.
Prints one JSON object; bytes by the algorithmic count: arcs x 20 B read once per call + states x points x 12 B written
and read."""
import ctypes as C
import importlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "old-kaldi-git_amd"


def cpu_baseline():
    src = os.path.join(ROOT, "tools", "latbest_cpu_baseline.cc")
    so = os.path.join(ROOT, PKG, "build", "liblatbest_cpu_baseline.so")
    os.makedirs(os.path.dirname(so), exist_ok=True)
    if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++14", "-shared", "-fPIC", src, "-o", so])
    fn = C.CDLL(so).latbest_cpu
    fn.restype = C.c_int64
    return fn


def decoded_compact_lattices(api, n_take, small):
    import torch
    if small:
        W = importlib.import_module(PKG + ".workloads")
        rng = np.random.default_rng(5)
        P, T = 600, 300
        g = W.make_hclg_structured(rng, 200_000, P)
        tp = np.zeros(2 * P + 1, np.int32)
        tp[1::2] = 1 + np.arange(P)
        lls = []
        for q in W.sample_paths(rng, g, [T] * n_take):
            x = (rng.standard_normal((T, P)) * 0.28 - 0.37).astype(np.float32)
            x[np.arange(T), q] = (0.5 + 0.3 * rng.standard_normal(T)).astype(np.float32)
            lls.append(x)
        cfg = api.decoder_config(beam=13.0, max_active=7000, min_active=200, lattice_beam=8.0)
        dec = api.LatticeFasterDecoder(api.Fst(g), cfg, max_batch=n_take, max_frames=T)
        dec.decode(torch.from_numpy(np.concatenate(lls)).cuda(), (np.arange(n_take + 1) * T).astype(np.int32))
        raws = [dec.get_raw_lattice(u) for u in range(n_take)]
        return api.determinize_lattices(raws, 8.0, tid_phone=tp), n_take * T
    bench = importlib.import_module("bench")
    net, priors, g, protos = bench.build_model_and_graph(3456, 10_000_000, False)
    feats, off = bench.build_utterances(3456, 0, 2620, net, g, protos, False)
    order = np.argsort(np.diff(off))
    pick = sorted(set(int(order[i]) for i in np.linspace(0, len(order) - 1, n_take).astype(int)))
    f2, o2 = bench.take_utterances(feats, off, pick)
    nnet = api.Nnet(net, priors)
    n_pdf = net[-1]["output_dim"]
    ll = torch.empty((int(o2[-1]), (n_pdf + 3) // 4 * 4), dtype=torch.float32, device="cuda")[:, :n_pdf]
    bench.forward_all(nnet, torch.from_numpy(f2).cuda(), o2, ll, max_rows=60000)
    dec = api.LatticeFasterDecoder(api.Fst(g), api.decoder_config(**bench.DECODE_CFG), max_batch=len(pick), max_frames=int(np.diff(o2).max()))
    dec.decode(ll, o2)
    raws = [dec.get_raw_lattice(j) for j in range(len(pick))]
    t2p = g["tid2pdf"]
    tid_phone = np.zeros(len(t2p), np.int32)
    tid_phone[1::2] = 1 + t2p[1::2]
    return api.determinize_lattices(raws, bench.DECODE_CFG["lattice_beam"], tid_phone=tid_phone), int(o2[-1])


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    n_take = int(args[0]) if args else 40
    copies = int(args[1]) if len(args) > 1 else 8
    api = importlib.import_module(PKG + ".api")
    api.select_gpu(0)
    clats, frames = decoded_compact_lattices(api, n_take, "--small" in sys.argv)
    csrs = [api.compact_lattice_to_csr(c) for c in clats] * copies
    points = [api.score_point(inv_acoustic_scale=float(l), word_ins_penalty=w) for w in (0.0, 0.5, 1.0) for l in range(9, 21)]
    states, arcs = sum(c["n_states"] for c in csrs), sum(len(c["arc_label"]) for c in csrs)
    out = dict(lattices=len(csrs), distinct_lattices=len(clats), frames=frames * copies, states=states, arcs=arcs, points=len(points))

    def timed(fn, reps=4):
        best = None
        for _ in range(reps):
            t0 = time.perf_counter()
            r = fn()
            dt = (time.perf_counter() - t0) * 1e3
            if best is None or dt < best[0]:
                best = (dt, r, api.compact_lattice_best_paths_last_timings())
        return best

    a_ms, a_res, a_split = timed(lambda: api.compact_lattice_best_paths_raw(csrs, points))
    out["a_one_call_36_points"] = dict(wall_ms=a_ms, **a_split)

    def one_by_one():
        k = 0.0
        for pt in points:
            api.compact_lattice_best_paths_raw(csrs, [pt])
            k += api.compact_lattice_best_paths_last_timings()["kernel_ms"]
        return k
    b_ms, b_kernel, _ = timed(one_by_one, reps=2)
    out["b_36_calls_1_point"] = dict(wall_ms=b_ms, kernel_ms=b_kernel)

    n, soff, aoff = len(csrs), np.zeros(len(csrs) + 1, np.int32), [np.zeros(1, np.int64)]
    base = 0
    for i, L in enumerate(csrs):
        soff[i + 1] = soff[i] + L["n_states"]
        aoff.append(np.asarray(L["arc_offsets"], np.int64)[1:] + base)
        base += int(L["arc_offsets"][-1])
    aoff = np.ascontiguousarray(np.concatenate(aoff))
    cat = lambda k, dt: np.ascontiguousarray(np.concatenate([np.asarray(L[k], dt) for L in csrs]))
    lab, nx, g, a = cat("arc_label", np.int32), cat("arc_nextstate", np.int32), cat("arc_graph", np.float32), cat("arc_acoustic", np.float32)
    fg, fa = cat("final_graph", np.float32), cat("final_acoustic", np.float32)
    fn = cpu_baseline()
    ip, fp = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    plen, tg, ta = np.empty((len(points), n), np.int32), np.empty((len(points), n), np.float32), np.empty((len(points), n), np.float32)

    def cpu():
        for p, (scale, pen) in enumerate(points):
            sc = np.ascontiguousarray(scale, np.float64)
            fn(C.c_int(n), soff.ctypes.data_as(ip), aoff.ctypes.data_as(C.POINTER(C.c_int64)), lab.ctypes.data_as(ip), nx.ctypes.data_as(ip),
               g.ctypes.data_as(fp), a.ctypes.data_as(fp), fg.ctypes.data_as(fp), fa.ctypes.data_as(fp), sc.ctypes.data_as(C.POINTER(C.c_double)),
               C.c_float(float(pen)), plen[p].ctypes.data_as(ip), tg[p].ctypes.data_as(fp), ta[p].ctypes.data_as(fp))
    c_ms, _, _ = timed(cpu, reps=3)
    out["c_cpu_one_thread_36_runs"] = dict(wall_ms=c_ms)
    # the baseline and the library agree (lengths and the totals' bits) - a guard on the comparison, not the test of either
    out["baseline_agrees"] = bool(np.array_equal(plen.T, a_res[0]) and np.array_equal(tg.T.view(np.int32), a_res[3].view(np.int32))
                                  and np.array_equal(ta.T.view(np.int32), a_res[4].view(np.int32)))
    out["c_over_a_wall"] = c_ms / a_ms
    out["c_over_a_kernel"] = c_ms / a_split["kernel_ms"]
    out["c_over_a_call"] = c_ms / a_split["call_ms"]      # the whole C call: allocations, events and the host's scatter included
    out["b_over_a_wall"] = b_ms / a_ms
    out["b_over_a_kernel"] = b_kernel / a_split["kernel_ms"]
    nbytes = arcs * 20 + states * len(points) * 12 * 2
    out["algorithmic_bytes"] = nbytes
    out["kernel_GB_per_s"] = nbytes / (a_split["kernel_ms"] * 1e-3) / 1e9
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
