#!/usr/bin/env python3
"""GMM statistics accumulation alone (the E-step of gmm-acc-stats-ali), two routes over one generated set: the cfg 2 model shape
of the benchmark (1800 pdfs, 9000 Gaussians, 40 dimensions; workloads.make_am_gmm) over --frames (200000) frames, every frame
drawn from a Gaussian of its pdf and carrying that pdf with weight 1.  The pdfs are drawn with a heavy head: each of the
first 4 pdfs with probability 0.05 - together a fifth of the frames, as silence holds in an alignment - and the other 1796
uniformly with the remaining 0.8, so 4 pdfs have runs of about 10000 entries (40 chunks) and the rest about 90 (one chunk):
 (a) the library: api.gmm_acc_component_posteriors then api.gmm_acc_stats, timed after a warming pass over --passes (15)
     passes: medians with minimum and maximum of the wall time, of each stage's whole call (host clock:
     gmm_acc_last_timings) and of the accumulation's two kernels alone between device events, and the bytes those kernels
     actually read (every workgroup's x rows, posteriors, row and offset arrays; the partial sums the second kernel adds)
     against that time;
 (b) tools/gmm_acc_cpu_baseline.cc (g++ -O2 -ffp-contract=off, one thread, a process of its own; its own clock around each
     stage, file reading excluded), and how far its accumulators are from the device's.
  python tools/gmm_acc_rate.py [--frames=200000] [--passes=15] [--out=FILE]
Prints one JSON object with frames/s per route and writes it to profiles/gmm_acc_rate.json (or --out).  No threshold is set on
any of these."""
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
HEAD_PDFS, HEAD_SHARE = 4, 0.2


def cpu_baseline(out_dir=None, extra_flags=()):
    """tools/gmm_acc_cpu_baseline.cc as a program (built when missing or older than its source); returns its path."""
    src = os.path.join(ROOT, "tools", "gmm_acc_cpu_baseline.cc")
    exe = os.path.join(out_dir or os.path.join(ROOT, PKG, "build"), "gmm_acc_cpu_baseline")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    if not os.path.exists(exe) or os.path.getmtime(exe) < os.path.getmtime(src):
        subprocess.check_call(["g++", "-O2", "-std=c++14", "-ffp-contract=off"] + list(extra_flags) + [src, "-o", exe])
    return exe


def write_input(path, am, feats, feats2, ent, flags):
    """The baseline's input file (layout in tools/gmm_acc_cpu_baseline.cc); am: dict(gconsts, means_invvars, inv_vars, pdf_offsets)."""
    off = np.asarray(am["pdf_offsets"], np.int32)
    with open(path, "wb") as f:
        f.write(struct.pack("<7i", feats.shape[0], feats.shape[1], feats2.shape[1], len(off) - 1, int(off[-1]), len(ent["pdf"]), int(flags)))
        for x, dt in ((feats, "<f4"), (feats2, "<f4"), (am["gconsts"], "<f4"), (am["means_invvars"], "<f4"), (am["inv_vars"], "<f4"),
                      (off, "<i4"), (ent["feo"], "<i8"), (ent["pdf"], "<i4"), (ent["weight"], "<f4")):
            f.write(np.ascontiguousarray(x, dt).tobytes())


def read_output(path, M, D2, E):
    buf = open(path, "rb").read()
    pos = [0]

    def take(dt, n):
        a = np.frombuffer(buf, dt, n, pos[0]).copy()
        pos[0] += a.nbytes
        return a
    n_post = int(take("<i8", 1)[0])
    out = dict(post=take("<f4", n_post), like=take("<f4", E), occ=take("<f8", M), mean_acc=take("<f8", M * D2).reshape(M, D2),
               var_acc=take("<f8", M * D2).reshape(M, D2))
    out["total_like"], out["total_frames"] = (float(x) for x in take("<f8", 2))
    assert pos[0] == len(buf)
    return out


def run_cpu(exe, am, feats, feats2, ent, flags, work_dir):
    """-> (the baseline's outputs, [ms of the posteriors, of the accumulation])."""
    inp, outp = os.path.join(work_dir, "gmm_acc_in.bin"), os.path.join(work_dir, "gmm_acc_out.bin")
    write_input(inp, am, feats, feats2, ent, flags)
    p = subprocess.run([exe, inp, outp], capture_output=True, text=True)
    if p.returncode != 0:
        raise ValueError("gmm_acc_cpu_baseline: " + p.stderr.strip())
    ms = [float(x) for x in p.stdout.split()[1:3]]
    return read_output(outp, int(am["pdf_offsets"][-1]), feats2.shape[1], len(ent["pdf"])), ms


def make_set(api, frames, seed=13000):
    workloads = importlib.import_module(PKG + ".workloads")
    rng = np.random.default_rng(seed)
    am = workloads.make_am_gmm(rng, 1800, 9000, 40)
    mi, iv = workloads.gmm_inv_params(am)
    g, _ = api.gmm_compute_gconsts(am["weights"], mi, iv)
    model = dict(gconsts=g, means_invvars=mi, inv_vars=iv, pdf_offsets=am["pdf_offsets"])
    p = np.full(1800, (1.0 - HEAD_SHARE) / (1800 - HEAD_PDFS))
    p[:HEAD_PDFS] = HEAD_SHARE / HEAD_PDFS
    pdf = rng.choice(1800, size=frames, p=p).astype(np.int32)
    sizes = np.diff(am["pdf_offsets"])
    gauss = am["pdf_offsets"][pdf] + (rng.random(frames) * sizes[pdf]).astype(np.int64)
    feats = (am["means"][gauss] + np.sqrt(am["vars"][gauss]) * rng.standard_normal((frames, 40))).astype(np.float32)
    ent = dict(feo=np.arange(frames + 1, dtype=np.int64), pdf=pdf, weight=np.ones(frames, np.float32),
               goff=np.concatenate([[0], np.cumsum(sizes[pdf])]).astype(np.int64))
    return model, feats, ent


def kernel_bytes(pdf_offsets, ent, D, chunk):
    """(bytes the accumulation kernel reads, bytes the chunk-sum kernel reads): per (chunk, 16-Gaussian row tile) workgroup the
    entries' x rows (D floats), row index (4) and posterior offset (8), and the tile's posteriors; per chunk G (2 D + 1) doubles."""
    sizes = np.diff(np.asarray(pdf_offsets, np.int64))
    n = np.bincount(ent["pdf"], minlength=len(sizes)).astype(np.int64)
    row_tiles = (sizes + 15) // 16
    acc = int((n * row_tiles * (4 * D + 12) + n * sizes * 4).sum())
    red = int((((n + chunk - 1) // chunk) * sizes * (2 * D + 1) * 8).sum())
    return acc, red


def main(argv):
    opt = dict(frames="200000", passes="15", out=os.path.join(ROOT, "profiles", "gmm_acc_rate.json"))
    for a in argv:
        k, _, v = a.lstrip("-").partition("=")
        opt[k] = v
    import torch
    api = importlib.import_module(PKG + ".api")
    api.select_gpu(0)
    T = int(opt["frames"])
    model, feats, ent = make_set(api, T)
    am = api.AmDiagGmm(model["gconsts"], model["means_invvars"], model["inv_vars"], model["pdf_offsets"])
    x = torch.from_numpy(feats).cuda()

    def device():
        t0 = time.perf_counter()
        post, _ = api.gmm_acc_component_posteriors(am, x, ent)
        acc = api.gmm_acc_stats(am, x, ent, post)
        wall = time.perf_counter() - t0
        t = api.gmm_acc_last_timings()
        return acc, wall, t
    device()                                            # warm: allocations, code load
    passes = [device() for _ in range(int(opt["passes"]))]
    acc = passes[0][0]
    walls = sorted(p[1] for p in passes)
    wall = walls[len(walls) // 2]
    keys = [k for k in passes[0][2] if k.endswith("_ms")]
    tm = {k: float(np.median([p[2][k] for p in passes])) for k in keys}
    spread = {k: [float(min(p[2][k] for p in passes)), float(max(p[2][k] for p in passes))] for k in keys}
    b_acc, b_red = kernel_bytes(model["pdf_offsets"], ent, 40, api.gmm_acc_chunk())
    counts = {k: int(passes[0][2][k]) for k in ("groups", "chunks", "workgroups")}
    n = np.bincount(ent["pdf"], minlength=1800)
    result = dict(frames=T, dim=40, pdfs=1800, gaussians=9000, head_pdfs=HEAD_PDFS, head_share=float(n[:HEAD_PDFS].sum()) / T,
                  largest_pdf_entries=int(n.max()), passes=len(passes), device_wall_ms=wall * 1e3,
                  device_wall_ms_min_max=[walls[0] * 1e3, walls[-1] * 1e3], device_stage_ms=tm, device_stage_ms_min_max=spread,
                  device_frames_per_s=T / wall, accumulate_counts=counts, accumulate_kernel_bytes_read=b_acc,
                  chunk_sum_kernel_bytes_read=b_red, kernels_read_gb_per_s=(b_acc + b_red) / (tm["kernels_ms"] * 1e-3) / 1e9)
    with tempfile.TemporaryDirectory() as d:
        cpu, ms = run_cpu(cpu_baseline(), model, feats, feats, ent, 7, d)
    rel = lambda a, b: float(np.abs(a - b).max() / np.abs(b).max())           # the largest difference over the largest value
    result.update(cpu_stage_ms=dict(component_posteriors_ms=ms[0], accumulate_ms=ms[1]), cpu_ms=sum(ms), cpu_frames_per_s=T / (sum(ms) / 1e3),
                  cpu_accumulate_frames_per_s=T / (ms[1] / 1e3), device_accumulate_frames_per_s=T / (tm["call_ms"] / 1e3),
                  max_difference_over_max_value=dict(occ=rel(acc["occ"], cpu["occ"]), mean_acc=rel(acc["mean_acc"], cpu["mean_acc"]),
                                               var_acc=rel(acc["var_acc"], cpu["var_acc"])),
                  speedup_accumulate_call=ms[1] / tm["call_ms"], speedup_accumulate_kernels=ms[1] / tm["kernels_ms"],
                  speedup_all=sum(ms) / (wall * 1e3))
    os.makedirs(os.path.dirname(opt["out"]), exist_ok=True)
    with open(opt["out"], "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
