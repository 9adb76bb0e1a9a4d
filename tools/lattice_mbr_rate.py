#!/usr/bin/env python3
"""The minimum-Bayes-risk stage alone: kh_compact_lattice_mbr on the determinized CompactLattices of a structured decode
(those of tools/lattice_prune_rate.py).  python tools/lattice_mbr_rate.py [n_utterances [copies]] [--out FILE]

At 1 score point (inverse acoustic scale 10) and at 16 (inverse acoustic scales 7 ... 22: local/score_mbr.sh's loop):
 (a) the C call, split as kh_compact_lattice_mbr_last_timings splits it (call_ms = the whole C call by the host's clock;
     wall_ms includes the Python packing around it), with its rounds, launches and AccStats() calls;
 (b) the whole Python call api.compact_lattice_mbr: preparation (super-final state, state times, CSR), the best paths that
     give the initial hypotheses, the C call, the per-point dicts;
 (c) tools/latmbr_cpu_baseline.cc (g++ -O2, one thread, a process of its own) over the same arrays and hypotheses, and
     whether it agrees with the library in every output bit for bit.
Prints one JSON object with lattices per second for each and writes it to profiles/lattice_mbr_bench.json (or --out);
`dominant` names the part of the Python call that takes longest.  No threshold is set on any of these."""
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


def cpu_baseline(out_dir=None, extra_flags=()):
    """tools/latmbr_cpu_baseline.cc as a program (built when missing or older than its source); returns its path."""
    src = os.path.join(ROOT, "tools", "latmbr_cpu_baseline.cc")
    exe = os.path.join(out_dir or os.path.join(ROOT, PKG, "build"), "latmbr_cpu_baseline")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    if not os.path.exists(exe) or os.path.getmtime(exe) < os.path.getmtime(src):
        subprocess.check_call(["g++", "-O2", "-std=c++14", "-ffp-contract=off"] + list(extra_flags) + [src, "-o", exe])
    return exe


def pack(csrs, points, hyps, do_mbr=True):
    """The batch as the baseline reads it (api.compact_lattice_mbr_raw's packing): the bytes of its input file."""
    n, K = len(csrs), len(points)
    soff = np.zeros(n + 1, np.int32)
    soff[1:] = np.cumsum([int(L["n_states"]) for L in csrs])
    aoff, base = [np.zeros(1, np.int64)], 0
    for L in csrs:
        o = np.asarray(L["arc_offsets"], np.int64)
        aoff.append(o[1:] + base)
        base += int(o[-1])
    aoff = np.concatenate(aoff)
    cat = lambda k, dt: np.concatenate([np.asarray(L[k], dt).reshape(-1) for L in csrs])
    flat = [np.asarray(hyps[i][p], np.int32).reshape(-1) for i in range(n) for p in range(K)]
    hoff = np.zeros(n * K + 1, np.int64)
    hoff[1:] = np.cumsum([len(h) for h in flat])
    hw = np.concatenate(flat + [np.zeros(0, np.int32)]).astype(np.int32)
    head = np.array([n, K, 1 if do_mbr else 0, int(soff[-1]), int(aoff[-1]), len(hw)], np.int64)
    parts = [head, soff, aoff.astype(np.int64), cat("arc_label", np.int32), cat("arc_nextstate", np.int32), cat("arc_graph", np.float32),
             cat("arc_acoustic", np.float32), cat("state_times", np.int32),
             np.stack([np.asarray(s, np.float64).reshape(4) for s, _ in points]).reshape(-1),
             np.asarray([p for _, p in points], np.float32), hoff, hw]
    return b"".join(np.ascontiguousarray(x).astype(x.dtype.newbyteorder("<")).tobytes() for x in parts), n, K


def unpack(data, n, K):
    """The baseline's output file -> api.compact_lattice_mbr_raw's list of lists of dicts."""
    at = 0

    def take(dt, count):
        nonlocal at
        x = np.frombuffer(data, np.dtype(dt).newbyteorder("<"), count, at)
        at += x.nbytes
        return x.astype(dt)

    out = []
    for i in range(n):
        row = []
        for p in range(K):
            nw, nb, ns, it = (int(x) for x in take(np.int32, 4))
            L = float(take(np.float64, 1)[0])
            words, obt, obc = take(np.int32, nw), take(np.float32, 2 * nw).reshape(-1, 2), take(np.float32, nw)
            sizes, bt = take(np.int32, nb), take(np.float32, 2 * nb).reshape(-1, 2)
            sw, sp = take(np.int32, ns), take(np.float32, ns)
            ends = np.cumsum(sizes)
            stats = [list(zip(sw[e - k:e].tolist(), sp[e - k:e])) for k, e in zip(sizes.tolist(), ends.tolist())]
            row.append(dict(words=words, bayes_risk=L, iterations=it, sausage_stats=stats, sausage_times=bt, one_best_times=obt,
                            one_best_confidences=obc))
        out.append(row)
    if at != len(data):
        raise ValueError("latmbr_cpu_baseline: %d bytes of output, %d read" % (len(data), at))
    return out


def run_cpu(exe, packed, work_dir=None):
    """The baseline, as a process, on pack()'s bytes.  Returns (unpack()'s result, seconds the process took).  Raises
    ValueError with the program's message when it refuses its input."""
    data, n, K = packed
    with tempfile.TemporaryDirectory(dir=work_dir) as d:
        fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        with open(fin, "wb") as f:
            f.write(data)
        t0 = time.perf_counter()
        r = subprocess.run([exe, fin, fout], stderr=subprocess.PIPE)
        dt = time.perf_counter() - t0
        if r.returncode != 0:
            raise ValueError(r.stderr.decode(errors="replace").strip() or "latmbr_cpu_baseline: exit status %d" % r.returncode)
        with open(fout, "rb") as f:
            return unpack(f.read(), n, K), dt


def same_answer(a, b):
    """Bit for bit, every output of every pair."""
    bits = lambda x: np.asarray(x, np.float32).reshape(-1).view(np.int32)
    for ra, rb in zip(a, b):
        for x, y in zip(ra, rb):
            if not (np.array_equal(x["words"], y["words"]) and x["iterations"] == y["iterations"] and
                    np.float64(x["bayes_risk"]).view(np.int64) == np.float64(y["bayes_risk"]).view(np.int64) and
                    len(x["sausage_stats"]) == len(y["sausage_stats"])):
                return False
            for bx, by in zip(x["sausage_stats"], y["sausage_stats"]):
                if [w for w, _ in bx] != [w for w, _ in by] or not np.array_equal(bits([p for _, p in bx]), bits([p for _, p in by])):
                    return False
            for k in ("sausage_times", "one_best_times", "one_best_confidences"):
                if not np.array_equal(bits(x[k]), bits(y[k])):
                    return False
    return True


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_path = os.path.join(ROOT, "profiles", "lattice_mbr_bench.json")
    if "--out" in sys.argv:
        out_path = sys.argv[sys.argv.index("--out") + 1]
        args = [a for a in args if a != out_path]
    n_take = int(args[0]) if args else 16
    copies = int(args[1]) if len(args) > 1 else 2
    exe = cpu_baseline()
    api = importlib.import_module(PKG + ".api")
    api.select_gpu(0)
    from tools.lattice_prune_rate import decoded_compact_lattices
    clats, frames = decoded_compact_lattices(api, n_take)
    clats = clats * copies
    n = len(clats)
    csrs = [api.compact_lattice_mbr_prepare(c) for c in clats]
    out = dict(lattices=n, distinct_lattices=n // copies, frames=frames * copies, states=sum(L["n_states"] for L in csrs),
               arcs=sum(len(L["arc_label"]) for L in csrs))

    def timed(fn_, reps=3, getter=api.compact_lattice_mbr_last_timings):
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
        points = [api.score_point(inv_acoustic_scale=float(7 + i if K > 1 else 10)) for i in range(K)]
        leg = dict(points=K, inv_acoustic_scales=[7 + i if K > 1 else 10 for i in range(K)])
        bp_ms, bp, _ = timed(lambda: api.compact_lattice_best_paths_raw(csrs, points), getter=api.compact_lattice_best_paths_last_timings)
        labels = [np.asarray(L["arc_label"], np.int32) for L in csrs]
        hyps = [[labels[i][bp[1][i][p]][labels[i][bp[1][i][p]] != 0] for p in range(K)] for i in range(n)]
        a_ms, raw, split = timed(lambda: api.compact_lattice_mbr_raw(csrs, points, hyps, True))
        leg["a_mbr_raw_call"] = dict(wall_ms=a_ms, lattices_per_s=per_s(a_ms), **split)
        leg["mean_iterations"] = float(np.mean([r["iterations"] for row in raw for r in row]))
        leg["mean_hypothesis_words"] = float(np.mean([len(r["words"]) for row in raw for r in row]))
        b_ms, res, _ = timed(lambda: api.compact_lattice_mbr(clats, points), reps=2)
        t0 = time.perf_counter()
        [api.compact_lattice_mbr_prepare(c) for c in clats]
        prep_ms = (time.perf_counter() - t0) * 1e3
        rest_ms = b_ms - prep_ms - bp_ms - a_ms
        leg["b_python_call"] = dict(wall_ms=b_ms, lattices_per_s=per_s(b_ms), prepare_ms=prep_ms, best_paths_ms=bp_ms, raw_call_ms=a_ms,
                                    rest_ms=rest_ms)
        cpu, c_s = run_cpu(exe, pack(csrs, points, hyps, True))
        leg["c_cpu_one_thread"] = dict(wall_ms=c_s * 1e3, lattices_per_s=per_s(c_s * 1e3), agrees=same_answer(cpu, raw))
        parts = dict(prepare=prep_ms, best_paths=bp_ms, host_prep=split["host_prep_ms"], upload=split["upload_ms"], kernel=split["kernel_ms"],
                     download=split["download_ms"], host_loop=split["host_loop_ms"], python_packing=a_ms - split["call_ms"], rest=rest_ms)
        leg["dominant"] = max(parts, key=parts.get)
        out["points_%d" % K] = leg
    text = json.dumps(out, indent=1)
    print(text)
    with open(out_path, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
