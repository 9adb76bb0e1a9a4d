#!/usr/bin/env python3
"""Gaussian selection and the global GMM accumulation alone (the inner loops of gmm-gselect and gmm-global-acc-stats
--gselect), two routes over --frames (200000) generated frames of D = --dim (40), in two configurations: 512 Gaussians with
n = 30 and 2048 Gaussians with n = 5:
 (a) the library, timed after a warming pass over --passes (3) passes, medians: api.gmm_gselect (the wall time of the wrapper,
     which also brings the lists to the host and cuts them per frame; the whole library call; its score kernels and its
     selection kernels between device events: gselect_last_timings), then api.accumulate_global_gmm_stats over the selected
     lists (the wrapper's wall time; the whole kh_gmm_preselect_posteriors call and its kernel; the whole kh_gmm_acc_stats call,
     its host plan and its two kernels: gmm_acc_last_timings);
 (b) tools/gselect_cpu_baseline.cc (g++ -O2 -ffp-contract=off, one thread, a process of its own; its own clock around each
     stage, file reading excluded): the same arithmetic, the sums frame by frame.
What is compared and recorded, not thresholded: whether the lists are equal on every frame; how many frame likelihoods and
posteriors differ in bits (the two routes' double exp / log / log1p are different libraries'; rounded to float they differ
only where a double lies within an ulp of a float rounding boundary); the accumulators' largest difference relative to the
bound (n + 2) 2^-53 sum |t| each route has against the exact sum (they add in different orders).
  python tools/gselect_rate.py [--frames=200000] [--dim=40] [--passes=3] [--cpu=1] [--out=FILE]
Prints one JSON object and writes it to profiles/gselect_rate.json (or --out).  No ratio is required of any figure."""
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
SEED = 1357
CONFIGS = [(512, 30), (2048, 5)]


def cpu_baseline(out_dir=None, extra_flags=()):
    """tools/gselect_cpu_baseline.cc as a program (built when missing or older than its source); returns its path."""
    src = os.path.join(ROOT, "tools", "gselect_cpu_baseline.cc")
    exe = os.path.join(out_dir or os.path.join(ROOT, PKG, "build"), "gselect_cpu_baseline")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    if not os.path.exists(exe) or os.path.getmtime(exe) < os.path.getmtime(src):
        subprocess.check_call(["g++", "-O2", "-std=c++14", "-ffp-contract=off"] + list(extra_flags) + [src, "-o", exe])
    return exe


def run_cpu(exe, model, feats, n, work_dir, preselect=None, repeats=1):
    """-> dict(lists, frame_like, post (per frame, over its selected list), post_like, occ, mean_acc, var_acc, ms); the
    layouts are in the source."""
    inp, outp = os.path.join(work_dir, "gselect_in.bin"), os.path.join(work_dir, "gselect_out.bin")
    T, D = feats.shape
    G = len(model["gconsts"])
    with open(inp, "wb") as f:
        f.write(struct.pack("<5i", T, D, G, n, 0 if preselect is None else 1))
        for x in (feats, model["gconsts"], model["means_invvars"], model["inv_vars"]):
            f.write(np.ascontiguousarray(x, "<f4").tobytes())
        if preselect is not None:
            f.write(np.cumsum([0] + [len(v) for v in preselect]).astype("<i8").tobytes())
            f.write(np.concatenate([np.asarray(v, "<i4") for v in preselect]).astype("<i4").tobytes())
    p = subprocess.run([exe, inp, outp, str(repeats)], capture_output=True, text=True)
    if p.returncode != 0:
        raise ValueError("gselect_cpu_baseline: " + p.stderr.strip())
    buf = open(outp, "rb").read()
    n_out, pos = min(n, G), 0

    def take(dt, count):
        nonlocal pos
        a = np.frombuffer(buf, dt, count, pos).copy()
        pos += a.nbytes
        return a
    sel = take("<i4", T * n_out).reshape(T, n_out)
    count = take("<i4", T)
    like = take("<f4", T)
    post = take("<f4", int(count.sum()))
    post_like = take("<f4", T)
    occ, mean, var = take("<f8", G), take("<f8", G * D).reshape(G, D), take("<f8", G * D).reshape(G, D)
    assert pos == len(buf)
    cuts = np.cumsum(count)[:-1]
    return dict(lists=[sel[t, :count[t]] for t in range(T)], frame_like=like, post=np.split(post, cuts) if T else [], post_like=post_like,
                occ=occ, mean_acc=mean, var_acc=var, ms=json.loads(p.stdout))


def make_set(T, D, G, seed=SEED):
    """-> (model dict(weights, gconsts-less arrays), feats [T, D] float32): frames drawn around the Gaussians' means."""
    rng = np.random.default_rng(seed + G)
    var = rng.uniform(0.5, 2.0, (G, D))
    mu = rng.standard_normal((G, D)) * 2.0
    pick = rng.integers(0, G, T)
    feats = (mu[pick] + rng.standard_normal((T, D)) * np.sqrt(var[pick])).astype(np.float32)
    iv = (1.0 / var).astype(np.float32)
    return dict(weights=np.full(G, 1.0 / G, np.float32), means_invvars=(mu / var).astype(np.float32), inv_vars=iv), feats


def median_of(passes):
    keys = [k for k in passes[0] if k.endswith("_ms")]
    return {k: float(np.median([p[k] for p in passes])) for k in keys}


def main(argv):
    opt = dict(frames="200000", dim="40", passes="3", cpu="1", out=os.path.join(ROOT, "profiles", "gselect_rate.json"))
    for a in argv:
        k, _, v = a.lstrip("-").partition("=")
        opt[k] = v
    import torch
    api = importlib.import_module(PKG + ".api")
    api.select_gpu(0)
    T, D = int(opt["frames"]), int(opt["dim"])
    result = dict(frames=T, dim=D, passes=int(opt["passes"]), device=torch.cuda.get_device_name(0), configurations=[])
    for G, n in CONFIGS:
        m, feats = make_set(T, D, G)
        gmm = api.diag_gmm(m["weights"], m["means_invvars"], m["inv_vars"])
        m["gconsts"] = gmm.gconsts.cpu().numpy()
        x = torch.from_numpy(feats).cuda()

        def select():
            t0 = time.perf_counter()
            r = api.gmm_gselect(gmm, x, n)
            t = {k: v for k, v in api.gselect_last_timings().items() if k in ("gselect_call_ms", "score_kernels_ms", "select_kernels_ms", "row_chunks")}
            t["gselect_wrapper_ms"] = (time.perf_counter() - t0) * 1e3
            return r, t

        def accumulate(lists):
            t0 = time.perf_counter()
            acc = api.accumulate_global_gmm_stats(gmm, x, lists)
            wall = (time.perf_counter() - t0) * 1e3
            g, a = api.gselect_last_timings(), api.gmm_acc_last_timings()
            return acc, dict(accumulate_wrapper_ms=wall, posteriors_call_ms=g["posteriors_call_ms"], posteriors_kernel_ms=g["posteriors_kernel_ms"],
                             acc_stats_call_ms=a["call_ms"], acc_stats_plan_ms=a["plan_ms"], acc_stats_kernels_ms=a["kernels_ms"])
        sel, _ = select()                                            # warm: allocations, code load
        acc, _ = accumulate(sel["lists"])
        sp, ap = [], []
        for _ in range(int(opt["passes"])):
            sel, t = select()
            sp.append(t)
            acc, t = accumulate(sel["lists"])
            ap.append(t)
        cfg = dict(gauss=G, n=n, row_chunks=int(sp[0]["row_chunks"]), nan_frames=int(sel["status"].sum()), ms=dict(median_of(sp), **median_of(ap)),
                   dense_posterior_megabytes=T * G * 4 / 1e6, dense_accumulation_gflop_fp64=2.0 * T * G * (2 * D + 1) / 1e9,
                   selected_items=int(sum(len(v) for v in sel["lists"])))
        if int(opt["cpu"]):
            with tempfile.TemporaryDirectory() as d:
                cpu = run_cpu(cpu_baseline(), m, feats, n, d)
            post, _, used = api.gmm_preselect_posteriors(gmm, x, sel["lists"])
            post = post.cpu().numpy()
            dev_post = [post[t, sel["lists"][t]] for t in range(T)]
            bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.int32)
            worst = 0.0
            for k in ("occ", "mean_acc", "var_acc"):
                diff = np.abs(acc[k] - cpu[k])
                scale = np.abs(cpu[k]) if k == "occ" else None              # the posteriors are positive: sum |t| is the sum
                if scale is None:                                       # sum |t| per element, from the device's posteriors
                    scale = np.zeros((G, D))
                    xa = np.abs(feats.astype(np.float64)) ** (1 if k == "mean_acc" else 2)
                    for t in range(T):
                        scale[sel["lists"][t]] += np.outer(dev_post[t].astype(np.float64), xa[t])
                bound = 2.0 * (T + 2) * 2.0 ** -53 * np.maximum(scale, 1e-300)
                worst = max(worst, float((diff / bound).max()))
            cfg.update(cpu_ms=cpu["ms"],
                       lists_equal_on_every_frame=bool(all(np.array_equal(a, b) for a, b in zip(cpu["lists"], sel["lists"]))),
                       frame_like_unequal_bits=int((bits(cpu["frame_like"]) != bits(sel["frame_like"])).sum()),
                       posteriors_unequal_bits=int(sum(int((bits(a) != bits(b)).sum()) for a, b in zip(cpu["post"], dev_post))),
                       posteriors_compared=int(sum(len(v) for v in dev_post)),
                       accumulators_worst_difference_over_bound=worst)
        result["configurations"].append(cfg)
    result["not_measured"] = ("reading and decompressing the archives, the tools' host work per utterance, a sparse accumulation kernel "
                              "(the dense form's extra arithmetic is the figure dense_accumulation_gflop_fp64)")
    os.makedirs(os.path.dirname(opt["out"]), exist_ok=True)
    with open(opt["out"], "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
