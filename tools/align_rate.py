#!/usr/bin/env python3
"""Forced alignment alone, three routes over one generated set (tests/align_cases.py generate(): training-graph-like graphs of
500-3000 states, utterances of 300-1500 frames, random log-likelihoods), at batches of 1, 16, 64 and 256 utterances:
 (a) api.align_compiled_raw - one kh_align_compiled call per batch - with the split of kh_align_compiled_last_timings;
 (b) tools/align_cpu_baseline.cc (g++ -O2, one thread, a process of its own; its own clock around the search, file reading
     excluded) over the first --cpu-max utterances of the same batch, and whether it agrees with the device bit for bit;
 (c) what the library offered before: one LatticeFasterDecoder per utterance (its own device graph and launch) plus its best
     path, as the fst_table branch of tools/latgen_faster.py does it (lattice-beam 0.1, determinization off) - a different
     search, timed for scale only, over at most --route-c utterances per batch size.
  python tools/align_rate.py [--batches=1,16,64,256] [--beam=200] [--route-c=16] [--cpu-max=64] [--out=FILE]
Prints one JSON object with utterances/s and frames/s per route and batch and writes it to profiles/align_rate.json (or
--out).  No threshold is set on any of these."""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
PKG = "old-kaldi-git_amd"


def cpu_baseline(out_dir=None, extra_flags=()):
    """tools/align_cpu_baseline.cc as a program (built when missing or older than its source); returns its path."""
    src = os.path.join(ROOT, "tools", "align_cpu_baseline.cc")
    exe = os.path.join(out_dir or os.path.join(ROOT, PKG, "build"), "align_cpu_baseline")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    if not os.path.exists(exe) or os.path.getmtime(exe) < os.path.getmtime(src):
        subprocess.check_call(["g++", "-O2", "-std=c++14", "-ffp-contract=off"] + list(extra_flags) + [src, "-o", exe])
    return exe


def run_cpu(exe, cases, beam, min_active, work_dir, repeat=0, room=None):
    """The baseline over a batch of cases; returns (per utterance dicts, milliseconds per pass or None)."""
    import align_cases as C
    path = os.path.join(work_dir, "align_dump.txt")
    C.write_dump(path, cases, beam, min_active, room=room)
    p = subprocess.run([exe, path] + ([str(repeat)] if repeat else []), capture_output=True, text=True)
    if p.returncode != 0:
        raise ValueError("align_cpu_baseline: " + p.stderr.strip())
    ms = [float(l.split()[1]) for l in p.stderr.splitlines() if l.startswith("ms_per_pass")]
    return C.read_dump_result(p.stdout), (ms[0] if ms else None)


def make_set(n, seed=9000):
    import align_cases as C
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        frames, states = int(rng.integers(300, 1501)), int(rng.integers(500, 3001))
        n_words = max(2, min(frames // 12, states // 14))          # a word costs about 13 states and at most 9 frames
        out.append(C.generate(seed + 1 + i, n_words=n_words, n_phones=10, max_prons=2, frames=frames, pad_to=states))
    return out


def main(argv):
    opt = dict(batches="1,16,64,256", beam="200", out=os.path.join(ROOT, "profiles", "align_rate.json"))
    opt["route-c"] = "16"
    opt["cpu-max"] = "64"
    for a in argv:
        k, _, v = a.lstrip("-").partition("=")
        opt[k] = v
    import torch
    api = importlib.import_module(PKG + ".api")
    api.select_gpu(0)
    batches = [int(x) for x in opt["batches"].split(",")]
    beam, min_active = float(opt["beam"]), 20
    cases = make_set(max(batches))
    exe = cpu_baseline()
    result = dict(beam=beam, min_active=min_active, states=[int(c["graph"]["num_states"]) for c in cases],
                  frames=[len(c["loglikes"]) for c in cases], rows=[])
    with tempfile.TemporaryDirectory() as d:
        for n in batches:
            sub = cases[:n]
            frames = sum(len(c["loglikes"]) for c in sub)
            ll = torch.from_numpy(np.ascontiguousarray(np.concatenate([c["loglikes"] for c in sub]))).cuda()
            ro = np.concatenate([[0], np.cumsum([len(c["loglikes"]) for c in sub])]).astype(np.int32)
            graphs = [c["graph"] for c in sub]
            api.align_compiled_raw(graphs, ll, ro, sub[0]["tid2pdf"], beam, min_active)       # warm: allocations, code load
            t0 = time.perf_counter()
            got = api.align_compiled_raw(graphs, ll, ro, sub[0]["tid2pdf"], beam, min_active)
            wall = time.perf_counter() - t0
            tm = api.align_compiled_last_timings()
            k = min(n, int(opt["cpu-max"]))         # the dump is text: the baseline runs the first k utterances of the batch
            cpu, cpu_ms = run_cpu(exe, sub[:k], beam, min_active, d, repeat=1, room=4000)
            cpu_frames = int(ro[k])
            same = all(g["status"] == c["status"] and g["cost"] == c["cost"] and
                       [(a[0], a[1], float(a[2]), float(a[3])) for a in g["path"]] == c["path"] for g, c in zip(got, cpu))
            row = dict(batch=n, frames=frames, device_wall_ms=wall * 1e3, device=tm, device_utts_per_s=n / wall, device_frames_per_s=frames / wall,
                       cpu_utts=k, cpu_ms=cpu_ms, cpu_utts_per_s=k / (cpu_ms / 1e3), cpu_frames_per_s=cpu_frames / (cpu_ms / 1e3), cpu_equal=bool(same),
                       done=sum(g["status"] == 0 for g in got))
            # (c) one LatticeFasterDecoder per utterance and its best path
            m = min(n, int(opt["route-c"]))
            cfg = api.decoder_config(beam=beam, max_active=2147483647, min_active=min_active, lattice_beam=0.1)
            t0 = time.perf_counter()
            for u in range(m):
                g = dict(graphs[u], tid2pdf=sub[u]["tid2pdf"])
                T = int(ro[u + 1] - ro[u])
                dec = api.LatticeFasterDecoder(api.Fst(g), cfg, max_batch=1, max_frames=T)
                dec.set_determinize(False)
                dec.decode(ll[int(ro[u]):int(ro[u + 1])], np.asarray([0, T], np.int32))
                dec.get_best_path(0)
            lat = time.perf_counter() - t0
            row.update(lattice_route_utts=m, lattice_route_utts_per_s=m / lat, lattice_route_frames_per_s=int(ro[m]) / lat)
            result["rows"].append(row)
            print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(opt["out"]), exist_ok=True)
    with open(opt["out"], "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(dict(written=opt["out"])))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
