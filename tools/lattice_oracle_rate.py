#!/usr/bin/env python3
"""The oracle stage alone: kh_compact_lattice_oracle on the determinized CompactLattices of a structured decode (those of
tools/lattice_prune_rate.py), each against a reference drawn from one of its own paths with about one word in eight
substituted, dropped or doubled.  python tools/lattice_oracle_rate.py [n_utterances [copies]] [--out FILE]

At 1 point (no masks: everything kept) and at 16 pruning beams (1 ... 8.5 in steps of 0.5, acoustic scale 0.1):
 (a) the C call(s), split as kh_compact_lattice_oracle_last_timings splits it (call_ms = the whole C call by the host's
     clock; wall_ms includes the Python packing around it); at 16 beams the pruning call that makes the masks is timed too;
 (b) the whole Python call api.compact_lattice_oracle: CSR conversion, the C call(s), the per-point dicts;
 (c) tools/latoracle_cpu_baseline.cc (g++ -O2, one thread) over the same arrays and mask words, and whether it agrees
     with the library in every output.
Prints one JSON object with lattices per second for each and writes it to profiles/lattice_oracle_bench.json (or --out);
`dominant` names the part of the Python call that takes longest.  No threshold is set on any of these."""
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


def cpu_baseline(out_dir=None):
    """tools/latoracle_cpu_baseline.cc as a shared library (built when missing or older than its source)."""
    src = os.path.join(ROOT, "tools", "latoracle_cpu_baseline.cc")
    so = os.path.join(out_dir or os.path.join(ROOT, PKG, "build"), "liblatoracle_cpu_baseline.so")
    os.makedirs(os.path.dirname(so), exist_ok=True)
    if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
        subprocess.check_call(["g++", "-O2", "-std=c++14", "-shared", "-fPIC", src, "-o", so])
    fn = C.CDLL(so).latoracle_cpu
    fn.restype = C.c_int64
    return fn


def pack(csrs, starts, refs, wildcards, is_final):
    """The batch as the C call takes it (api.compact_lattice_oracle_raw's packing, without the frames)."""
    n = len(csrs)
    soff = np.zeros(n + 1, np.int32)
    soff[1:] = np.cumsum([int(L["n_states"]) for L in csrs])
    aoff, base = [np.zeros(1, np.int64)], 0
    for L in csrs:
        o = np.asarray(L["arc_offsets"], np.int64)
        aoff.append(o[1:] + base)
        base += int(o[-1])
    cat = lambda k: np.ascontiguousarray(np.concatenate([np.asarray(L[k], np.int32) for L in csrs]))
    roff = np.zeros(n + 1, np.int64)
    roff[1:] = np.cumsum([len(r) for r in refs])
    return dict(n=n, soff=soff, start=np.ascontiguousarray(np.asarray(starts, np.int32)), aoff=np.ascontiguousarray(np.concatenate(aoff)),
                label=cat("arc_label"), next=cat("arc_nextstate"),
                is_final=np.ascontiguousarray(np.concatenate([np.asarray(f, bool) for f in is_final]).astype(np.int32)), roff=roff,
                ref=np.ascontiguousarray(np.concatenate([np.asarray(r, np.int32).reshape(-1) for r in refs] + [np.zeros(0, np.int32)])),
                wild=np.ascontiguousarray(np.unique(np.asarray(list(wildcards), np.int32))))


def run_cpu(fn, B, K=1, arc_keep_words=None, final_keep_words=None):
    """The baseline on pack()'s arrays and, for K > 1 or a masked point, the pruning call's mask words.  Returns
    compact_lattice_oracle_raw's dict without the frame sums."""
    n = B["n"]
    room = np.repeat(np.maximum(np.diff(B["soff"]).astype(np.int64) - 1, 1), K)
    poff = np.zeros(n * K + 1, np.int64)
    poff[1:] = np.cumsum(room)
    err, cnt = np.empty(n * K, np.int32), np.empty(n * K * 4, np.int32)
    plen, pfin, parcs = np.empty(n * K, np.int32), np.empty(n * K, np.int32), np.empty(int(poff[-1]), np.int32)
    ip, lp, up = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_uint64)
    ptr = lambda a, t: None if a is None else a.ctypes.data_as(t)
    ak = None if arc_keep_words is None else np.ascontiguousarray(arc_keep_words, np.uint64)
    fk = None if final_keep_words is None else np.ascontiguousarray(final_keep_words, np.uint64)
    rc = fn(C.c_int(n), ptr(B["soff"], ip), ptr(B["start"], ip), ptr(B["aoff"], lp), ptr(B["label"], ip), ptr(B["next"], ip),
            ptr(B["is_final"], ip), ptr(B["roff"], lp), ptr(B["ref"], ip), C.c_int(len(B["wild"])), ptr(B["wild"], ip), C.c_int(K),
            ptr(ak, up), ptr(fk, up), ptr(err, ip), ptr(cnt, ip), ptr(plen, ip), ptr(parcs, ip), ptr(poff, lp), ptr(pfin, ip))
    if rc < 0:
        raise ValueError("latoracle_cpu: arguments refused")
    paths = [[parcs[poff[i * K + p]:poff[i * K + p] + max(int(plen[i * K + p]), 0)].copy() for p in range(K)] for i in range(n)]
    return dict(errors=err.reshape(n, K), counts=cnt.reshape(n, K, 4), path_len=plen.reshape(n, K), paths=paths,
                final_state=pfin.reshape(n, K))


def same_answer(a, b):
    return bool(all(np.array_equal(a[k], b[k]) for k in ("errors", "counts", "path_len", "final_state")) and
                all(np.array_equal(x, y) for ra, rb in zip(a["paths"], b["paths"]) for x, y in zip(ra, rb)))


def references(rng, csrs):
    """One reference per lattice: the words along a random path from the start state, about one in eight of them
    substituted, dropped or doubled."""
    refs = []
    for L in csrs:
        off, nxt, lab = L["arc_offsets"], L["arc_nextstate"], L["arc_label"]
        s, words = int(L["start"]), []
        while off[s + 1] > off[s]:
            a = int(rng.integers(off[s], off[s + 1]))
            if lab[a] != 0:
                words.append(int(lab[a]))
            s = int(nxt[a])
        vocab = np.unique(lab[lab != 0])
        ref = []
        for w in words:
            u = rng.random()
            if u < 1 / 24:
                continue
            ref.append(int(rng.choice(vocab)) if u < 2 / 24 else w)
            if u > 23 / 24:
                ref.append(w)
        refs.append(ref)
    return refs


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_path = os.path.join(ROOT, "profiles", "lattice_oracle_bench.json")
    if "--out" in sys.argv:
        out_path = sys.argv[sys.argv.index("--out") + 1]
        args = [a for a in args if a != out_path]
    n_take = int(args[0]) if args else 16
    copies = int(args[1]) if len(args) > 1 else 4
    fn = cpu_baseline()
    api = importlib.import_module(PKG + ".api")
    api.select_gpu(0)
    from tools.lattice_prune_rate import decoded_compact_lattices
    clats, frames = decoded_compact_lattices(api, n_take)
    clats = clats * copies
    csrs = [api._oracle_csr(c) for c in clats]
    starts = [L["start"] for L in csrs]
    refs = references(np.random.default_rng(11), csrs[:n_take]) * copies
    n = len(clats)
    states, arcs = sum(L["n_states"] for L in csrs), sum(len(L["arc_label"]) for L in csrs)
    beams = [1.0 + 0.5 * i for i in range(16)]
    point = api.score_point(acoustic_scale=0.1)
    out = dict(lattices=n, distinct_lattices=n // copies, frames=frames * copies, states=states, arcs=arcs,
               ref_words=sum(len(r) for r in refs), cells_per_point=sum(L["n_states"] * (len(r) + 1) for L, r in zip(csrs, refs)))
    B = pack(csrs, starts, refs, (), [L["is_final"] for L in csrs])

    def timed(fn_, reps=4, getter=api.compact_lattice_oracle_last_timings):
        best = None
        for _ in range(reps):
            t0 = time.perf_counter()
            r = fn_()
            dt = (time.perf_counter() - t0) * 1e3
            if best is None or dt < best[0]:
                best = (dt, r, getter())
        return best

    per_s = lambda ms: n / (ms * 1e-3)
    for K in (1, 16):
        leg = dict(points=K)
        masks, prune_ms = None, 0.0
        if K > 1:
            leg["beams"], leg["acoustic_scale"] = beams, 0.1
            prune_ms, masks, psplit = timed(lambda: api.compact_lattice_prune_raw(csrs, starts, [point] * K, beams),
                                            getter=api.compact_lattice_prune_last_timings)
            leg["a_prune_raw_call"] = dict(wall_ms=prune_ms, **psplit)
            leg["arcs_kept_fraction_per_beam"] = [float(x) for x in masks["arc_keep"].mean(axis=0)]
        a_ms, raw, split = timed(lambda: api.compact_lattice_oracle_raw(csrs, starts, refs, (), masks))
        leg["a_oracle_raw_call"] = dict(wall_ms=a_ms, lattices_per_s=per_s(a_ms + prune_ms), **split)
        leg["kernel_cells_per_us"] = out["cells_per_point"] * K / (split["kernel_ms"] * 1e3)
        if K == 1:
            b_ms, res, _ = timed(lambda: api.compact_lattice_oracle(clats, refs), reps=3)
        else:
            b_ms, res, _ = timed(lambda: api.compact_lattice_oracle(clats, refs, points=[point], beams=beams), reps=3)
        t0 = time.perf_counter()
        [api._oracle_csr(c) for c in clats]
        csr_ms = (time.perf_counter() - t0) * 1e3
        rest_ms = b_ms - csr_ms - a_ms - prune_ms
        leg["b_python_call"] = dict(wall_ms=b_ms, lattices_per_s=per_s(b_ms), csr_ms=csr_ms, raw_calls_ms=a_ms + prune_ms, assembly_ms=rest_ms)
        words = (None, None) if masks is None else (masks["arc_keep_words"], masks["final_keep_words"])
        c_ms, cpu, _ = timed(lambda: run_cpu(fn, B, K, *words), reps=3)
        leg["c_cpu_one_thread"] = dict(wall_ms=c_ms, lattices_per_s=per_s(c_ms), agrees=same_answer(cpu, raw))
        leg["mean_errors"] = float(np.where(raw["errors"] >= 0, raw["errors"], 0).mean())
        leg["no_path"] = int((raw["errors"] < 0).sum())
        parts = dict(csr=csr_ms, prune_call=prune_ms, host_prep=split["host_prep_ms"], upload=split["upload_ms"], kernel=split["kernel_ms"],
                     download=split["download_ms"], assembly=rest_ms)
        leg["dominant"] = max(parts, key=parts.get)
        out["points_%d" % K] = leg
    text = json.dumps(out, indent=1)
    print(text)
    with open(out_path, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
