#!/usr/bin/env python3
"""The pruning stage alone: one compact_lattice_prune call on the determinized CompactLattices of a structured decode, the
36 score points of the scoring grid, beam 5.  python tools/lattice_prune_rate.py [n_utterances [copies]] [--out FILE]

 (a) the C call, split as kh_compact_lattice_prune_last_timings splits it (call_ms = the whole C call by the host's clock);
 (b) the whole Python call api.compact_lattice_prune: CSR conversion, the C call, the assembly of lattices x points
     CompactLattice dicts;
 (c) for scale, the line-by-line restatement (tests/latprune_restatement.py) on ONE lattice and ONE point.
Prints one JSON object and writes it to profiles/lattice_prune_bench.json (or --out); `dominant` names the part of the
Python call that takes longest.  No threshold is set on any of these."""
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "old-kaldi-git_amd"


def decoded_compact_lattices(api, n_take):
    import torch
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


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_path = os.path.join(ROOT, "profiles", "lattice_prune_bench.json")
    if "--out" in sys.argv:
        out_path = sys.argv[sys.argv.index("--out") + 1]
        args = [a for a in args if a != out_path]
    n_take = int(args[0]) if args else 16
    copies = int(args[1]) if len(args) > 1 else 4
    api = importlib.import_module(PKG + ".api")
    api.select_gpu(0)
    clats, frames = decoded_compact_lattices(api, n_take)
    clats = clats * copies
    points = [api.score_point(inv_acoustic_scale=float(l), word_ins_penalty=w) for w in (0.0, 0.5, 1.0) for l in range(9, 21)]
    beam = 5.0
    csrs = [api.compact_lattice_to_prune_csr(c) for c in clats]
    starts = [c["start"] for c in csrs]
    states, arcs = sum(c["n_states"] for c in csrs), sum(len(c["arc_label"]) for c in csrs)
    out = dict(lattices=len(clats), distinct_lattices=len(clats) // copies, frames=frames * copies, states=states, arcs=arcs,
               points=len(points), beam=beam)

    def timed(fn, reps=4):
        best = None
        for _ in range(reps):
            t0 = time.perf_counter()
            r = fn()
            dt = (time.perf_counter() - t0) * 1e3
            if best is None or dt < best[0]:
                best = (dt, r, api.compact_lattice_prune_last_timings())
        return best

    a_ms, raw, split = timed(lambda: api.compact_lattice_prune_raw(csrs, starts, points, beam))
    out["a_raw_call"] = dict(wall_ms=a_ms, **split)
    b_ms, res, _ = timed(lambda: api.compact_lattice_prune(clats, points, beam), reps=3)
    t0 = time.perf_counter()
    [api.compact_lattice_to_prune_csr(c) for c in clats]
    csr_ms = (time.perf_counter() - t0) * 1e3
    out["b_python_call"] = dict(wall_ms=b_ms, csr_ms=csr_ms, raw_call_ms=a_ms, assembly_ms=b_ms - csr_ms - a_ms)
    out["arcs_kept_fraction"] = float(raw["arc_keep"].mean())
    out["states_kept_fraction"] = float(raw["state_keep"].mean())
    # bytes by the algorithmic count: arcs x 40 B read (two sweeps of 16 B, 8 B for reachability) + states x 64 lanes x 8 B
    # written and read twice + the mask words
    nbytes = arcs * 40 + states * 64 * 8 * 4 + (2 * arcs + 4 * states) * 8
    out["algorithmic_bytes"] = nbytes
    out["kernel_GB_per_s"] = nbytes / (split["kernel_ms"] * 1e-3) / 1e9
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import latprune_restatement as R
    t0 = time.perf_counter()
    r = R.prune_lattice(csrs[0], points[0][0], points[0][1], beam)
    c_ms = (time.perf_counter() - t0) * 1e3
    out["c_restatement_one_lattice_one_point"] = dict(wall_ms=c_ms, arcs=len(csrs[0]["arc_label"]),
                                                      agrees=bool(np.array_equal(r["arc_keep"], raw["arc_keep"][:raw["arc_offsets"][1], 0])))
    parts = dict(csr=csr_ms, host_prep=split["host_prep_ms"], upload=split["upload_ms"], kernel=split["kernel_ms"],
                 download=split["download_ms"], assembly=b_ms - csr_ms - a_ms)
    out["dominant"] = max(parts, key=parts.get)
    text = json.dumps(out, indent=1)
    print(text)
    with open(out_path, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
