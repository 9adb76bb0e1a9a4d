#!/usr/bin/env python3
"""The acoustic-rescoring stage alone: api.gmm_rescore_compact_lattices on state-level lattices converted as
gmm-rescore-lattice's reader converts them.  python tools/gmm_rescore_rate.py [n_utterances [copies]] [--lattices FILE.npz] [--out FILE]

The lattices: --lattices takes the file tools/dump_bench_lattices.py writes (raw lattices of the benchmark's utterances with
their tid2pdf); without it the raw lattices of the structured decode of tools/lattice_prune_rate.py are used (600 pdfs, 300
frames each).  Either way the model is a random diagonal GMM with one mixture of --mix (8) Gaussians per pdf in 39
dimensions and the features are random frames: the time of this stage does not depend on what the scores are.
 (a) the library route, split: host preparation / upload / rescoring kernels / download as
     kh_rescore_compact_lattice_last_timings splits the C call, the scoring (AmDiagGmm.pdf_log_likelihoods, the dense frame x
     pdf matrix) by HIP events around it, and the wall time of the whole api.gmm_rescore_compact_lattices call;
 (b) tools/gmm_rescore_cpu_baseline.cc (g++ -O2, one thread, a process of its own, its own clock, file reading excluded):
     the per-(frame, pdf) cache and the in-place update, over the same arrays; the largest difference between its costs and
     the library's is reported (the scorers differ in their last bits, so it is not zero).
Prints one JSON object and writes it to profiles/gmm_rescore_rate.json (or --out).  No threshold is set on any of these."""
import importlib
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "old-kaldi-git_amd"


def cpu_baseline(out_dir=None):
    src = os.path.join(ROOT, "tools", "gmm_rescore_cpu_baseline.cc")
    exe = os.path.join(out_dir or os.path.join(ROOT, PKG, "build"), "gmm_rescore_cpu_baseline")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    if not os.path.exists(exe) or os.path.getmtime(exe) < os.path.getmtime(src):
        subprocess.check_call(["g++", "-O2", "-std=c++14", "-ffp-contract=off", src, "-o", exe])
    return exe


def pack(csrs, rows, tid2pdf, feats, gm):
    """The batch as the baseline reads it: the arrays of api.compact_lattice_rescore_raw, the features and the model, each
    behind its int64 count."""
    soff = np.concatenate([[0], np.cumsum([int(L["n_states"]) for L in csrs])]).astype(np.int32)
    aoff, base = [np.zeros(1, np.int64)], 0
    for L in csrs:
        o = np.asarray(L["arc_offsets"], np.int64)
        aoff.append(o[1:] + base)
        base += int(o[-1])
    cat = lambda k, dt: np.concatenate([np.asarray(L[k], dt).reshape(-1) for L in csrs] + [np.zeros(0, dt)])
    a_str = [x for L in csrs for x in L["arc_string"]]
    f_str = [x for L in csrs for x in L["final_string"]]
    aso = np.concatenate([[0], np.cumsum([len(x) for x in a_str])]).astype(np.int64)
    fso = (np.concatenate([[0], np.cumsum([len(x) for x in f_str])]) + aso[-1]).astype(np.int64)
    flat = np.concatenate([np.asarray(x, np.int32).reshape(-1) for x in a_str + f_str] + [np.zeros(0, np.int32)])
    feats = np.asarray(feats, np.float32)
    parts = [soff, np.concatenate(aoff), cat("arc_nextstate", np.int32), cat("arc_acoustic", np.float32), aso, cat("final_graph", np.float32),
             cat("final_acoustic", np.float32), fso, flat, np.asarray(rows, np.int32), np.asarray(tid2pdf, np.int32),
             np.asarray([feats.shape[1]], np.int32), feats.reshape(-1), np.asarray(gm["gconsts"], np.float32),
             np.asarray(gm["means_invvars"], np.float32).reshape(-1), np.asarray(gm["inv_vars"], np.float32).reshape(-1),
             np.asarray(gm["pdf_offsets"], np.int32)]
    le = lambda x: np.ascontiguousarray(x).astype(x.dtype.newbyteorder("<")).tobytes()
    return b"".join(le(np.asarray([x.size], np.int64)) + le(x) for x in parts)


def run_cpu(exe, packed, repeat=1):
    """The baseline, as a process, on pack()'s bytes -> (arc costs followed by final costs, float32; milliseconds of its best pass)."""
    with tempfile.TemporaryDirectory() as d:
        fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        with open(fin, "wb") as f:
            f.write(packed)
        r = subprocess.run([exe, fin, fout, str(repeat)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        if r.returncode != 0:
            raise ValueError(r.stderr.decode(errors="replace").strip() or "gmm_rescore_cpu_baseline: exit status %d" % r.returncode)
        return np.fromfile(fout, "<f4"), float(r.stdout.decode().strip())


def raw_lattices(api, n_take, path):
    """(raw lattices, tid2pdf [num_tids + 1])."""
    if path:
        z = np.load(path)
        n = min(int(z["n"]), n_take)
        keys = ("arc_src", "arc_dst", "arc_il", "arc_ol", "arc_g", "arc_a", "state_final")
        return [{k: z["%d_%s" % (j, k)] for k in keys} for j in range(n)], np.asarray(z["tid2pdf"], np.int32)
    import torch
    W = importlib.import_module(PKG + ".workloads")
    rng = np.random.default_rng(5)
    P, T = 600, 300
    g = W.make_hclg_structured(rng, 200_000, P)
    lls = []
    for q in W.sample_paths(rng, g, [T] * n_take):
        x = (rng.standard_normal((T, P)) * 0.28 - 0.37).astype(np.float32)
        x[np.arange(T), q] = (0.5 + 0.3 * rng.standard_normal(T)).astype(np.float32)
        lls.append(x)
    cfg = api.decoder_config(beam=13.0, max_active=7000, min_active=200, lattice_beam=8.0)
    dec = api.LatticeFasterDecoder(api.Fst(g), cfg, max_batch=n_take, max_frames=T)
    dec.decode(torch.from_numpy(np.concatenate(lls)).cuda(), (np.arange(n_take + 1) * T).astype(np.int32))
    return [dec.get_raw_lattice(u) for u in range(n_take)], np.asarray(g["tid2pdf"], np.int32)


def random_gmm(api, n_pdfs, mix, dim, rng):
    M = n_pdfs * mix
    means = rng.standard_normal((M, dim)).astype(np.float32)
    inv_vars = np.exp(0.2 * rng.standard_normal((M, dim))).astype(np.float32)
    weights = np.full(M, 1.0 / mix, np.float32)
    mi = (means * inv_vars).astype(np.float32)
    gconsts, _ = api.gmm_compute_gconsts(weights, mi, inv_vars)
    off = (np.arange(n_pdfs + 1) * mix).astype(np.int32)
    return dict(gconsts=np.asarray(gconsts, np.float32), means_invvars=mi, inv_vars=inv_vars, pdf_offsets=off)


def main():
    import torch
    argv = sys.argv[1:]
    opt = {}
    for name in ("--lattices", "--out", "--mix"):
        if name in argv:
            i = argv.index(name)
            opt[name] = argv[i + 1]
            del argv[i:i + 2]
    n_take = int(argv[0]) if argv else 16
    copies = int(argv[1]) if len(argv) > 1 else 4
    out_path = opt.get("--out", os.path.join(ROOT, "profiles", "gmm_rescore_rate.json"))
    mix, dim = int(opt.get("--mix", 8)), 39
    exe = cpu_baseline()
    api = importlib.import_module(PKG + ".api")
    kio = importlib.import_module(PKG + ".kaldi_io")
    api.select_gpu(0)
    raws, tid2pdf = raw_lattices(api, n_take, opt.get("--lattices"))
    t0 = time.perf_counter()
    clats = [kio.lattice_to_compact_lattice(L) for L in raws]
    convert_ms = (time.perf_counter() - t0) * 1e3
    clats = clats * copies
    csrs = [api.compact_lattice_align_csr(c) for c in clats]
    n = len(csrs)
    rng = np.random.default_rng(9)
    n_pdfs = int(tid2pdf[1:].max()) + 1
    gm = random_gmm(api, n_pdfs, mix, dim, rng)
    am = api.AmDiagGmm(gm["gconsts"], gm["means_invvars"], gm["inv_vars"], gm["pdf_offsets"])
    # one row per frame of the lattice: utt_len from a first call on an empty matrix layout is not needed - the times are the
    # lattice's own: a zero-row probe gives utt_len with the status FEATURES_TOO_SHORT
    probe = torch.zeros((1, n_pdfs), dtype=torch.float32, device="cuda")
    _, utt_len, _, _ = api.compact_lattice_rescore_raw(csrs, probe, np.zeros(n + 1, np.int32), tid2pdf)
    rows = np.concatenate([[0], np.cumsum(utt_len)]).astype(np.int32)
    feats_h = rng.standard_normal((int(rows[-1]), dim)).astype(np.float32)
    feats = torch.from_numpy(feats_h).cuda()
    strings = sum(len(x) for L in csrs for x in L["arc_string"])
    out = dict(lattices=n, distinct_lattices=n // copies, frames=int(rows[-1]), pdfs=n_pdfs, gaussians=n_pdfs * mix, dim=dim,
               states=sum(int(L["n_states"]) for L in csrs), arcs=sum(len(L["arc_nextstate"]) for L in csrs), transition_ids=strings,
               convert_lattice_ms_per_distinct_set=convert_ms)
    best = None
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for _ in range(4):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ev[0].record()
        ll = am.pdf_log_likelihoods(feats, log_sum_exp_prune=-1.0)
        ev[1].record()
        status, _, arcs, finals = api.compact_lattice_rescore_raw(csrs, ll, rows, tid2pdf)
        wall = (time.perf_counter() - t0) * 1e3
        torch.cuda.synchronize()
        if best is None or wall < best[0]:
            best = (wall, ev[0].elapsed_time(ev[1]), api.compact_lattice_rescore_last_timings(), status, arcs, finals)
    wall, score_ms, split, status, arcs, finals = best
    t0 = time.perf_counter()
    api.gmm_rescore_compact_lattices(am, feats, rows, clats, tid2pdf)
    api_wall = (time.perf_counter() - t0) * 1e3
    device_ms = score_ms + split["call_ms"]
    out["statuses"] = np.bincount(status, minlength=6).tolist()
    out["a_library"] = dict(scoring_ms=score_ms, wall_ms=wall, api_call_with_python_packing_ms=api_wall, scoring_plus_c_call_ms=device_ms,
                            kernel_share_of_c_call=split["kernel_ms"] / split["call_ms"],
                            kernel_share_of_scoring_plus_c_call=split["kernel_ms"] / device_ms, lattices_per_s=n / (device_ms * 1e-3), **split)
    # (b) the host baseline on the same arrays
    res, c_ms = run_cpu(exe, pack(csrs, rows, tid2pdf, feats_h, gm), repeat=3)
    got = np.concatenate(arcs + finals)
    fin_mask = np.isfinite(got) & np.isfinite(res)
    out["b_cpu_one_thread"] = dict(ms=c_ms, lattices_per_s=n / (c_ms * 1e-3),
                                   max_abs_difference_from_library=float(np.abs(got[fin_mask] - res[fin_mask]).max()) if fin_mask.any() else 0.0,
                                   same_infinities=bool(np.array_equal(np.isfinite(got), np.isfinite(res))))
    out["library_over_cpu"] = c_ms / device_ms
    text = json.dumps(out, indent=1)
    print(text)
    with open(out_path, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
