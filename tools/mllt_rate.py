#!/usr/bin/env python3
"""MLLT statistics accumulation alone (the inner loop of gmm-acc-mllt), two routes over the generated set of
tools/gmm_acc_rate.py: the cfg 2 model shape of the benchmark (1800 pdfs, 9000 Gaussians, 40 dimensions) over --frames
(200000) frames, every frame carrying its pdf with weight 1.  The Gaussian posteriors are computed once
(api.gmm_acc_component_posteriors) and brought to the host; then, for --rand-prune=0, 0.25 and 4.0:
 (a) the library: api.rand_prune on a copy (seeded, so every pass prunes alike), the host beta, the upload and
     api.mllt_acc_stats, timed after a warming pass over --passes (7) passes: medians with minimum and maximum of the wall
     time of the pruning and beta, of the upload, of the whole accumulation call, of its host plan (the posteriors'
     download and the item list; host clock: mllt_last_timings) and of its two kernels alone between device events, and the
     useful floating-point rate 2 n D Q / t of the kernels and of the call;
 (b) tools/mllt_cpu_baseline.cc (g++ -O2 -ffp-contract=off, one thread, a process of its own; its own clock around the
     pruning and the accumulation, file reading excluded) with the same seed, and how far its G is from the device's.
  python tools/mllt_rate.py [--frames=200000] [--passes=7] [--prune=0,0.25,4.0] [--cpu=1] [--out=FILE]
Prints one JSON object and writes it to profiles/mllt_rate.json (or --out).  No threshold is set on any of these."""
import importlib
import json
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


def cpu_baseline(out_dir=None, extra_flags=()):
    """tools/mllt_cpu_baseline.cc as a program (built when missing or older than its source); returns its path."""
    src = os.path.join(ROOT, "tools", "mllt_cpu_baseline.cc")
    exe = os.path.join(out_dir or os.path.join(ROOT, PKG, "build"), "mllt_cpu_baseline")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    if not os.path.exists(exe) or os.path.getmtime(exe) < os.path.getmtime(src):
        subprocess.check_call(["g++", "-O2", "-std=c++14", "-ffp-contract=off"] + list(extra_flags) + [src, "-o", exe])
    return exe


def write_input(path, am, feats, ent, post, prune, seed):
    """The baseline's input file (layout in tools/mllt_cpu_baseline.cc); am: dict(means_invvars, inv_vars, pdf_offsets)."""
    off = np.asarray(am["pdf_offsets"], np.int32)
    with open(path, "wb") as f:
        f.write(struct.pack("<6if", feats.shape[0], feats.shape[1], len(off) - 1, int(off[-1]), len(ent["pdf"]),
                            -1 if seed is None else int(seed), float(prune)))
        for x, dt in ((feats, "<f4"), (am["means_invvars"], "<f4"), (am["inv_vars"], "<f4"), (off, "<i4"), (ent["feo"], "<i8"),
                      (ent["pdf"], "<i4"), (post, "<f4")):
            f.write(np.ascontiguousarray(x, dt).tobytes())


def read_output(path, D):
    buf = open(path, "rb").read()
    n_post = int(np.frombuffer(buf, "<i8", 1, 0)[0])
    pos = 8
    pruned = np.frombuffer(buf, "<f4", n_post, pos).copy()
    pos += 4 * n_post
    items = int(np.frombuffer(buf, "<i8", 1, pos)[0])
    beta = float(np.frombuffer(buf, "<f8", 1, pos + 8)[0])
    Q = D * (D + 1) // 2
    G = np.frombuffer(buf, "<f8", D * Q, pos + 16).copy().reshape(D, Q)
    assert pos + 16 + 8 * D * Q == len(buf)
    return dict(pruned=pruned, items=items, beta=beta, G=G)


def run_cpu(exe, am, feats, ent, post, prune, seed, work_dir):
    """-> (the baseline's outputs, [ms of the pruning, of the accumulation])."""
    inp, outp = os.path.join(work_dir, "mllt_in.bin"), os.path.join(work_dir, "mllt_out.bin")
    write_input(inp, am, feats, ent, post, prune, seed)
    p = subprocess.run([exe, inp, outp], capture_output=True, text=True)
    if p.returncode != 0:
        raise ValueError("mllt_cpu_baseline: " + p.stderr.strip())
    ms = [float(x) for x in p.stdout.split()[1:3]]
    return read_output(outp, feats.shape[1]), ms


def main(argv):
    opt = dict(frames="200000", passes="7", prune="0,0.25,4.0", cpu="1", out=os.path.join(ROOT, "profiles", "mllt_rate.json"))
    for a in argv:
        k, _, v = a.lstrip("-").partition("=")
        opt[k] = v
    import torch
    api = importlib.import_module(PKG + ".api")
    rate = importlib.import_module("tools.gmm_acc_rate")
    api.select_gpu(0)
    T = int(opt["frames"])
    model, feats, ent = rate.make_set(api, T)
    am = api.AmDiagGmm(model["gconsts"], model["means_invvars"], model["inv_vars"], model["pdf_offsets"])
    x = torch.from_numpy(feats).cuda()
    post_dev, _ = api.gmm_acc_component_posteriors(am, x, ent)
    post0 = np.ascontiguousarray(post_dev.cpu().numpy())
    D = 40
    Q = D * (D + 1) // 2
    result = dict(frames=T, dim=D, pdfs=1800, gaussians=9000, gaussian_posteriors=int(post0.size), passes=int(opt["passes"]),
                  chunk=api.mllt_chunk(), max_slices=api.mllt_max_slices(), runs={})

    def device(prune):
        t0 = time.perf_counter()
        post = post0.copy()
        api.rand_prune(post, prune, seed=SEED)
        beta = float(np.cumsum(api._entry_sums(post, ent["goff"]))[-1])
        t1 = time.perf_counter()
        p = torch.from_numpy(post).cuda()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        G = api.mllt_acc_stats(am, x, ent, p)
        t3 = time.perf_counter()
        t = api.mllt_last_timings()
        t.update(prune_and_beta_ms=(t1 - t0) * 1e3, upload_ms=(t2 - t1) * 1e3, wall_ms=(t3 - t0) * 1e3)
        return G, beta, t

    for prune in [float(v) for v in opt["prune"].split(",")]:
        device(prune)                                       # warm: allocations, code load
        passes = [device(prune) for _ in range(int(opt["passes"]))]
        G, beta, t = passes[0]
        keys = [k for k in t if k.endswith("_ms")]
        med = {k: float(np.median([p[2][k] for p in passes])) for k in keys}
        spread = {k: [float(min(p[2][k] for p in passes)), float(max(p[2][k] for p in passes))] for k in keys}
        n = int(t["items"])
        flop = 2.0 * n * D * Q
        run = dict(items=n, slices=int(t["slices"]), workgroups=int(t["workgroups"]), beta=beta, device_ms=med, device_ms_min_max=spread,
                   kernels_useful_tflops=flop / (med["kernels_ms"] * 1e-3) / 1e12 if n else 0.0,
                   call_useful_tflops=flop / (med["call_ms"] * 1e-3) / 1e12 if n else 0.0)
        if int(opt["cpu"]):
            with tempfile.TemporaryDirectory() as d:
                cpu, ms = run_cpu(cpu_baseline(), model, feats, ent, post0, prune, SEED, d)
            assert cpu["items"] == n and cpu["beta"] == beta
            run.update(cpu_ms=dict(prune_ms=ms[0], accumulate_ms=ms[1]), cpu_useful_gflops=flop / (ms[1] * 1e-3) / 1e9 if n else 0.0,
                       max_difference_over_max_value=float(np.abs(G - cpu["G"]).max() / np.abs(cpu["G"]).max()),
                       speedup_accumulate_call=ms[1] / med["call_ms"], speedup_accumulate_kernels=ms[1] / med["kernels_ms"],
                       speedup_prune_beta_upload_call=sum(ms) / (med["prune_and_beta_ms"] + med["upload_ms"] + med["call_ms"]))
        result["runs"]["%g" % prune] = run
    os.makedirs(os.path.dirname(opt["out"]), exist_ok=True)
    with open(opt["out"], "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
