#!/usr/bin/env python3
"""LDA statistics accumulation alone (the inner loop of acc-lda), two routes over a generated set: --frames (200000) frames
of N(0, 1) features times a per-dimension scale in [0.25, 4], every frame carrying one of 1800 pdfs with weight 1, in
utterances of --utt-frames (500) frames, at D = 117 (13-dimensional features spliced +-4) and D = 460 (40-dimensional
features spliced +-4 with a 100-dimensional iVector), for --rand-prune=0 and 4.0:
 (a) the library: api.rand_prune_at on a copy of the weights (seeded, so every pass prunes alike), the upload of the
     features, and api.lda_acc_stats with the utterances as segments, timed after a warming pass over --passes (15) passes:
     medians with minimum and maximum of the wall time of the pruning, of the upload, of the whole accumulation call, of
     its host plan (host clock: lda_last_timings) and of its kernels alone between device events, and the useful
     floating-point rate 2 n Q / t of the kernels and of the call (the second-order statistic alone);
 (b) tools/lda_cpu_baseline.cc (g++ -O2 -ffp-contract=off, one thread, a process of its own; its own clock around the
     pruning and the accumulation, file reading excluded) with the same seed, and how far its statistics are from the
     device's.
  python tools/lda_rate.py [--frames=200000] [--utt-frames=500] [--passes=15] [--dims=117,460] [--prune=0,4.0] [--cpu=1] [--out=FILE]
Prints one JSON object and writes it to profiles/lda_rate.json (or --out).  No threshold is set on any of these."""
import importlib
import json
import math
import os
import struct
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "old-kaldi-git_amd"
SEED = 4321
NUM_PDFS = 1800


def cpu_baseline(out_dir=None, extra_flags=()):
    """tools/lda_cpu_baseline.cc as a program (built when missing or older than its source); returns its path."""
    src = os.path.join(ROOT, "tools", "lda_cpu_baseline.cc")
    exe = os.path.join(out_dir or os.path.join(ROOT, PKG, "build"), "lda_cpu_baseline")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    if not os.path.exists(exe) or os.path.getmtime(exe) < os.path.getmtime(src):
        subprocess.check_call(["g++", "-O2", "-std=c++14", "-ffp-contract=off"] + list(extra_flags) + [src, "-o", exe])
    return exe


def write_input(path, feats, ent, num_classes, prune, seed):
    """The baseline's input file (layout in tools/lda_cpu_baseline.cc)."""
    with open(path, "wb") as f:
        f.write(struct.pack("<5if", feats.shape[0], feats.shape[1], num_classes, len(ent["pdf"]), -1 if seed is None else int(seed), float(prune)))
        for x, dt in ((feats, "<f4"), (ent["feo"], "<i8"), (ent["pdf"], "<i4"), (ent["weight"], "<f4")):
            f.write(np.ascontiguousarray(x, dt).tobytes())


def read_output(path, E, C, D):
    buf = open(path, "rb").read()
    Q = D * (D + 1) // 2
    pruned = np.frombuffer(buf, "<f4", E, 0).copy()
    pos = 4 * E
    items = int(np.frombuffer(buf, "<i8", 1, pos)[0])
    zero = np.frombuffer(buf, "<f8", C, pos + 8).copy()
    first = np.frombuffer(buf, "<f8", C * D, pos + 8 + 8 * C).copy().reshape(C, D)
    second = np.frombuffer(buf, "<f8", Q, pos + 8 + 8 * C + 8 * C * D).copy()
    assert pos + 8 + 8 * (C + C * D + Q) == len(buf)
    return dict(pruned=pruned, items=items, zero=zero, first=first, second=second)


def run_cpu(exe, feats, ent, num_classes, prune, seed, work_dir):
    """-> (the baseline's outputs, [ms of the pruning, of the accumulation])."""
    inp, outp = os.path.join(work_dir, "lda_in.bin"), os.path.join(work_dir, "lda_out.bin")
    write_input(inp, feats, ent, num_classes, prune, seed)
    p = subprocess.run([exe, inp, outp], capture_output=True, text=True)
    if p.returncode != 0:
        raise ValueError("lda_cpu_baseline: " + p.stderr.strip())
    ms = [float(x) for x in p.stdout.split()[1:3]]
    return read_output(outp, len(ent["pdf"]), num_classes, feats.shape[1]), ms


def make_set(T, D, seed=SEED):
    rng = np.random.default_rng(seed)
    feats = (rng.standard_normal((T, D), dtype=np.float32) * np.exp(rng.uniform(math.log(0.25), math.log(4.0), D)).astype(np.float32))
    ent = dict(feo=np.arange(T + 1, dtype=np.int64), pdf=rng.integers(0, NUM_PDFS, T).astype(np.int32), weight=np.ones(T, np.float32))
    return np.ascontiguousarray(feats, np.float32), ent


def main(argv):
    opt = dict(frames="200000", passes="15", dims="117,460", prune="0,4.0", cpu="1", out=os.path.join(ROOT, "profiles", "lda_rate.json"))
    opt["utt-frames"] = "500"
    for a in argv:
        k, _, v = a.lstrip("-").partition("=")
        opt[k] = v
    import torch
    api = importlib.import_module(PKG + ".api")
    api.select_gpu(0)
    T, U = int(opt["frames"]), int(opt["utt-frames"])
    segments = np.asarray(list(range(0, T, U)) + [T], np.int64)
    result = dict(frames=T, pdfs=NUM_PDFS, utterance_frames=U, segments=len(segments) - 1, passes=int(opt["passes"]), chunk=api.lda_chunk(),
                  max_slices=api.lda_max_slices(), max_dim=api.lda_max_dim(), runs={})
    for D in [int(v) for v in opt["dims"].split(",")]:
        feats, ent = make_set(T, D)
        Q = D * (D + 1) // 2

        def device(prune):
            t0 = time.perf_counter()
            w = ent["weight"].copy()
            api.rand_prune_at(w, prune, SEED, 0)
            t1 = time.perf_counter()
            x = torch.from_numpy(feats).cuda()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            acc = api.lda_acc_stats(x, dict(ent, weight=w), NUM_PDFS, segments=segments)
            t3 = time.perf_counter()
            t = api.lda_last_timings()
            t.update(prune_ms=(t1 - t0) * 1e3, upload_ms=(t2 - t1) * 1e3, wall_ms=(t3 - t0) * 1e3)
            return acc, t

        for prune in [float(v) for v in opt["prune"].split(",")]:
            device(prune)                                       # warm: allocations, code load
            passes = [device(prune) for _ in range(int(opt["passes"]))]
            acc, t = passes[0]
            keys = [k for k in t if k.endswith("_ms")]
            med = {k: float(np.median([p[1][k] for p in passes])) for k in keys}
            spread = {k: [float(min(p[1][k] for p in passes)), float(max(p[1][k] for p in passes))] for k in keys}
            n = int(t["items"])
            flop = 2.0 * n * Q
            run = dict(dim=D, rand_prune=prune, items=n, slices=int(t["slices"]), workgroups=int(t["workgroups"]), passes=int(t["passes"]),
                       feature_megabytes=feats.nbytes / 1e6, device_ms=med, device_ms_min_max=spread,
                       kernels_useful_tflops=flop / (med["kernels_ms"] * 1e-3) / 1e12 if n else 0.0,
                       call_useful_tflops=flop / (med["call_ms"] * 1e-3) / 1e12 if n else 0.0)
            if int(opt["cpu"]):
                with tempfile.TemporaryDirectory() as d:
                    cpu, ms = run_cpu(cpu_baseline(), feats, ent, NUM_PDFS, prune, SEED, d)
                assert cpu["items"] == n and np.array_equal(cpu["zero"], acc["zero"])      # weights 1 and 4: every order is exact
                run.update(cpu_ms=dict(prune_ms=ms[0], accumulate_ms=ms[1]), cpu_useful_gflops=flop / (ms[1] * 1e-3) / 1e9 if n else 0.0,
                           max_difference_over_max_value={k: float(np.abs(acc[k] - cpu[k]).max() / np.abs(cpu[k]).max()) for k in ("first", "second")},
                           speedup_accumulate_call=ms[1] / med["call_ms"], speedup_accumulate_kernels=ms[1] / med["kernels_ms"],
                           speedup_prune_upload_call=sum(ms) / (med["prune_ms"] + med["upload_ms"] + med["call_ms"]))
            result["runs"]["D%d_prune%g" % (D, prune)] = run
    os.makedirs(os.path.dirname(opt["out"]), exist_ok=True)
    with open(opt["out"], "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
