#!/usr/bin/env python3
"""fMLLR estimation alone, two routes over one generated set: --speakers (40) speakers of --frames (2500) frames each, the cfg 2
model shape of the benchmark (1800 pdfs, 9000 Gaussians, 40 dimensions; workloads.make_am_gmm), every frame drawn from a
Gaussian of the model and carrying one pdf with weight 1, a diagonal distortion per speaker:
 (a) the library's four stages (api.gmm_component_posteriors, fmllr_frame_stats, fmllr_accumulate, fmllr_update), timed after a
     warming pass over --passes (15) passes: medians with minimum and maximum, the per-stage times of api.fmllr_last_timings
     (whole calls, on the host clock) and the time of the accumulation's two kernels alone between device events;
 (b) tools/fmllr_cpu_baseline.cc (g++ -O2, one thread, a process of its own; its own clock around each stage, file reading
     excluded), and how far its transforms are from the device's.
  python tools/fmllr_rate.py [--speakers=40] [--frames=2500] [--update-type=full] [--passes=15] [--out=FILE]
Prints one JSON object with frames/s and speakers/s per route and writes it to profiles/fmllr_rate.json (or --out).  No
threshold is set on any of these."""
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
TYPES = ["full", "diag", "offset", "none"]


def cpu_baseline(out_dir=None, extra_flags=()):
    """tools/fmllr_cpu_baseline.cc as a program (built when missing or older than its sources); returns its path."""
    src = os.path.join(ROOT, "tools", "fmllr_cpu_baseline.cc")
    hdr = os.path.join(ROOT, PKG, "csrc", "kh_fmllr_update.h")
    exe = os.path.join(out_dir or os.path.join(ROOT, PKG, "build"), "fmllr_cpu_baseline")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.check_call(["g++", "-O2", "-std=c++14", "-ffp-contract=off"] + list(extra_flags) + [src, "-o", exe])
    return exe


def write_input(path, am, feats, utt_row_offsets, spk_utt_offsets, ent, update_type, min_count, num_iters):
    """The baseline's input file (layout in tools/fmllr_cpu_baseline.cc); am: dict(gconsts, means_invvars, inv_vars, pdf_offsets)."""
    T, D = feats.shape
    off = np.asarray(am["pdf_offsets"], np.int32)
    with open(path, "wb") as f:
        f.write(struct.pack("<9i", T, D, len(off) - 1, int(off[-1]), len(utt_row_offsets) - 1, len(spk_utt_offsets) - 1, len(ent["pdf"]),
                            TYPES.index(update_type), int(num_iters)))
        f.write(struct.pack("<f", float(min_count)))
        for x, dt in ((feats, "<f4"), (am["gconsts"], "<f4"), (am["means_invvars"], "<f4"), (am["inv_vars"], "<f4"), (off, "<i4"),
                      (utt_row_offsets, "<i4"), (spk_utt_offsets, "<i4"), (ent["feo"], "<i8"), (ent["pdf"], "<i4"), (ent["weight"], "<f4")):
            f.write(np.ascontiguousarray(x, dt).tobytes())


def read_output(path, D, n_spk, E):
    buf = open(path, "rb").read()
    pos = [0]

    def take(dt, n):
        a = np.frombuffer(buf, dt, n, pos[0]).copy()
        pos[0] += a.nbytes
        return a
    P = (D + 1) * (D + 2) // 2
    n_post = int(take("<i8", 1)[0])
    out = dict(post=take("<f4", n_post), like=take("<f4", E))
    R = int(take("<i4", 1)[0])
    out.update(run_row=take("<i4", R), spk_run_offsets=take("<i4", n_spk + 1), a=take("<f4", R * D).reshape(R, D), b=take("<f4", R * D).reshape(R, D),
               count=take("<f8", R), beta=take("<f8", n_spk), K=take("<f8", n_spk * D * (D + 1)).reshape(n_spk, D, D + 1),
               G=take("<f8", n_spk * D * P).reshape(n_spk, D, P), W=take("<f4", n_spk * D * (D + 1)).reshape(n_spk, D, D + 1),
               impr=take("<f4", n_spk), count_f=take("<f4", n_spk))
    assert pos[0] == len(buf)
    return out


def run_cpu(exe, am, feats, utt_row_offsets, spk_utt_offsets, ent, update_type, min_count, num_iters, work_dir):
    """-> (the baseline's outputs, [ms of A1, A2, B, C])."""
    inp, outp = os.path.join(work_dir, "fmllr_in.bin"), os.path.join(work_dir, "fmllr_out.bin")
    write_input(inp, am, feats, utt_row_offsets, spk_utt_offsets, ent, update_type, min_count, num_iters)
    p = subprocess.run([exe, inp, outp], capture_output=True, text=True)
    if p.returncode != 0:
        raise ValueError("fmllr_cpu_baseline: " + p.stderr.strip())
    ms = [float(x) for x in p.stdout.split()[1:5]]
    return read_output(outp, feats.shape[1], len(spk_utt_offsets) - 1, len(ent["pdf"])), ms


def make_set(api, n_spk, frames, seed=12000):
    workloads = importlib.import_module(PKG + ".workloads")
    rng = np.random.default_rng(seed)
    am = workloads.make_am_gmm(rng, 1800, 9000, 40)
    mi, iv = workloads.gmm_inv_params(am)
    g, _ = api.gmm_compute_gconsts(am["weights"], mi, iv)
    model = dict(gconsts=g, means_invvars=mi, inv_vars=iv, pdf_offsets=am["pdf_offsets"])
    T = n_spk * frames
    pdf = rng.integers(0, 1800, T).astype(np.int32)
    gauss = (am["pdf_offsets"][pdf] + (rng.random(T) * np.diff(am["pdf_offsets"])[pdf]).astype(np.int64))
    x = am["means"][gauss] + np.sqrt(am["vars"][gauss]) * rng.standard_normal((T, 40))
    scale = np.exp(rng.uniform(np.log(0.8), np.log(1.25), (n_spk, 40)))
    shift = rng.uniform(-0.5, 0.5, (n_spk, 40))
    feats = (x.reshape(n_spk, frames, 40) * scale[:, None] + shift[:, None]).reshape(T, 40).astype(np.float32)
    utt = (np.arange(n_spk + 1) * frames).astype(np.int32)
    ent = dict(feo=np.arange(T + 1, dtype=np.int64), pdf=pdf, weight=np.ones(T, np.float32),
               goff=np.concatenate([[0], np.cumsum(np.diff(am["pdf_offsets"])[pdf])]).astype(np.int64))
    return model, feats, utt, np.arange(n_spk + 1, dtype=np.int32), ent


def main(argv):
    opt = dict(speakers="40", frames="2500", out=os.path.join(ROOT, "profiles", "fmllr_rate.json"))
    opt["update-type"] = "full"
    opt["passes"] = "15"
    for a in argv:
        k, _, v = a.lstrip("-").partition("=")
        opt[k] = v
    import torch
    api = importlib.import_module(PKG + ".api")
    api.select_gpu(0)
    n_spk, frames, ty = int(opt["speakers"]), int(opt["frames"]), opt["update-type"]
    model, feats, utt, spk, ent = make_set(api, n_spk, frames)
    T = len(feats)
    am = api.AmDiagGmm(model["gconsts"], model["means_invvars"], model["inv_vars"], model["pdf_offsets"])
    x = torch.from_numpy(feats).cuda()

    def device():
        t0 = time.perf_counter()
        post, _ = api.gmm_component_posteriors(am, x, ent)
        fs = api.fmllr_frame_stats(am, x, utt, spk, ent, post)
        stats = api.fmllr_accumulate(x, fs)
        W, impr, count = api.fmllr_update(stats, ty, 500.0, 40)
        return W, time.perf_counter() - t0, api.fmllr_last_timings()
    device()                                            # warm: allocations, code load
    passes = [device() for _ in range(int(opt["passes"]))]
    W = passes[0][0]
    walls = sorted(p[1] for p in passes)
    wall = walls[len(walls) // 2]
    keys = [k for k in passes[0][2] if k.endswith("_ms")]
    tm = {k: float(np.median([p[2][k] for p in passes])) for k in keys}
    spread = {k: [float(min(p[2][k] for p in passes)), float(max(p[2][k] for p in passes))] for k in keys}
    result = dict(speakers=n_spk, frames_per_speaker=frames, frames=T, dim=40, gaussians=9000, update_type=ty, passes=len(passes),
                  device_wall_ms=wall * 1e3, device_wall_ms_min_max=[walls[0] * 1e3, walls[-1] * 1e3], device_stage_ms=tm,
                  device_stage_ms_min_max=spread, device_frames_per_s=T / wall, device_speakers_per_s=n_spk / wall)
    print(json.dumps(result), flush=True)
    with tempfile.TemporaryDirectory() as d:
        cpu, ms = run_cpu(cpu_baseline(), model, feats, utt, spk, ent, ty, 500.0, 40, d)
    result.update(cpu_stage_ms=dict(component_posteriors_ms=ms[0], frame_stats_ms=ms[1], accumulate_ms=ms[2], update_ms=ms[3]),
                  cpu_ms=sum(ms), cpu_frames_per_s=T / (sum(ms) / 1e3), cpu_speakers_per_s=n_spk / (sum(ms) / 1e3),
                  max_transform_difference=float(np.abs(cpu["W"].astype(np.float64) - W).max()),
                  speedup_accumulate_call=ms[2] / tm["accumulate_ms"], speedup_accumulate_kernels=ms[2] / tm["accumulate_kernels_ms"],
                  speedup_all=sum(ms) / (wall * 1e3))
    print(json.dumps(result), flush=True)
    os.makedirs(os.path.dirname(opt["out"]), exist_ok=True)
    with open(opt["out"], "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(dict(written=opt["out"])))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
