#!/usr/bin/env python3
"""Tree statistics accumulation alone (the inner loop of acc-tree-stats), two routes over a generated set shaped like a
recipe's: --frames (200000) frames of D = --dim (40) features; about a fifth of the frames on five context-independent
silence events (one phone, five pdf-classes), the rest drawn with a 1 / (rank + 10) law from --events (40000) triphone events
(three phones of 40, three pdf-classes), so that tens of thousands of events are met, most of them a handful of times:
 (a) the library: the upload of the features, then api.tree_acc_stats from zero (add = 0) and running on (add = 1, which
     also uploads the sums), timed after a warming pass over --passes (15) passes: medians with minimum and maximum of the
     whole call, of its host plan (host clock: tree_last_timings) and of its kernel alone between device events; and one
     api.TreeStats.accumulate over the frames' event tuples, which adds the compaction of the events in Python, and one
     over per-utterance event tables and frame indices (codes=), the form the tool uses;
 (b) tools/tree_stats_cpu_baseline.cc (g++ -O2 -ffp-contract=off, one thread, a process of its own; its own clock around
     the accumulation, file reading excluded): a std::map of events, the same arithmetic.  Its statistics must equal the
     library's bit for bit, or the tool stops.
  python tools/tree_stats_rate.py [--frames=200000] [--dim=40] [--events=40000] [--passes=15] [--cpu=1] [--out=FILE]
Prints one JSON object and writes it to profiles/tree_stats_rate.json (or --out).  No threshold is set on any figure; the
expectation recorded against is only that the whole library call beats the one-thread baseline on the same machine
(library_call_beats_baseline)."""
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
SEED = 2468


def cpu_baseline(out_dir=None, extra_flags=()):
    """tools/tree_stats_cpu_baseline.cc as a program (built when missing or older than its source); returns its path."""
    src = os.path.join(ROOT, "tools", "tree_stats_cpu_baseline.cc")
    exe = os.path.join(out_dir or os.path.join(ROOT, PKG, "build"), "tree_stats_cpu_baseline")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    if not os.path.exists(exe) or os.path.getmtime(exe) < os.path.getmtime(src):
        subprocess.check_call(["g++", "-O2", "-std=c++14", "-ffp-contract=off"] + list(extra_flags) + [src, "-o", exe])
    return exe


def run_cpu(exe, feats, frame_event, events, work_dir):
    """-> ([(event, count, stats [2, D])] in the program's map order, ms of the accumulation); the layouts are in the source."""
    inp, outp = os.path.join(work_dir, "tree_in.bin"), os.path.join(work_dir, "tree_out.bin")
    T, D = feats.shape
    offsets = np.cumsum([0] + [len(e) for e in events]).astype("<i4")
    pairs = np.asarray([v for e in events for kv in e for v in kv], "<i4")
    with open(inp, "wb") as f:
        f.write(struct.pack("<4i", T, D, len(events), int(offsets[-1])))
        for x, dt in ((feats, "<f4"), (frame_event, "<i4"), (offsets, "<i4"), (pairs, "<i4")):
            f.write(np.ascontiguousarray(x, dt).tobytes())
    p = subprocess.run([exe, inp, outp], capture_output=True, text=True)
    if p.returncode != 0:
        raise ValueError("tree_stats_cpu_baseline: " + p.stderr.strip())
    buf = open(outp, "rb").read()
    n, pos, out = struct.unpack_from("<q", buf, 0)[0], 8, []
    for _ in range(n):
        k = struct.unpack_from("<i", buf, pos)[0]
        ev = np.frombuffer(buf, "<i4", 2 * k, pos + 4).reshape(k, 2)
        pos += 4 + 8 * k
        count = struct.unpack_from("<d", buf, pos)[0]
        out.append((tuple((int(a), int(b)) for a, b in ev), count, np.frombuffer(buf, "<f8", 2 * D, pos + 8).reshape(2, D).copy()))
        pos += 8 + 16 * D
    assert pos == len(buf)
    return out, float(p.stdout.split()[1])


def make_set(T, D, n_events, seed=SEED):
    """-> (feats [T, D] float32, frame_event [T] int32, events: the event tuples by id)."""
    rng = np.random.default_rng(seed)
    events = [((-1, pc), (1, 1)) for pc in range(5)]
    seen = set()
    while len(events) < 5 + n_events:
        a, b, c, pc = (int(v) for v in np.append(rng.integers(2, 42, 3), rng.integers(0, 3)))
        if (a, b, c, pc) not in seen:
            seen.add((a, b, c, pc))
            events.append(((-1, pc), (0, a), (1, b), (2, c)))
    law = 1.0 / (np.arange(n_events) + 10.0)
    fe = np.where(rng.random(T) < 0.2, rng.integers(0, 5, T), 5 + rng.choice(n_events, T, p=law / law.sum())).astype(np.int32)
    feats = rng.standard_normal((T, D), dtype=np.float32) * np.float32(3.0) + np.float32(0.5)
    return np.ascontiguousarray(feats, np.float32), fe, events


def main(argv):
    opt = dict(frames="200000", dim="40", events="40000", passes="15", cpu="1", out=os.path.join(ROOT, "profiles", "tree_stats_rate.json"))
    for a in argv:
        k, _, v = a.lstrip("-").partition("=")
        opt[k] = v
    import torch
    api = importlib.import_module(PKG + ".api")
    api.select_gpu(0)
    T, D = int(opt["frames"]), int(opt["dim"])
    feats, fe, events = make_set(T, D, int(opt["events"]))
    E = len(events)
    runs = np.bincount(fe, minlength=E)

    def device(add, count, stats):
        t0 = time.perf_counter()
        x = torch.from_numpy(feats).cuda()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        api.tree_acc_stats(x, fe, count, stats, add=add)
        t2 = time.perf_counter()
        t = api.tree_last_timings()
        t.update(upload_ms=(t1 - t0) * 1e3, wall_ms=(t2 - t0) * 1e3)
        return t

    result = dict(frames=T, dim=D, events_possible=E, tile=api.tree_tile(), max_dim=api.tree_max_dim(), passes=int(opt["passes"]),
                  feature_megabytes=feats.nbytes / 1e6, statistics_megabytes=E * 2 * D * 8 / 1e6)
    count, stats = np.zeros(E), np.zeros((E, 2, D))
    for name, add in (("from_zero", False), ("running_on", True)):
        device(add, count.copy(), stats.copy())                   # warm: allocations, code load
        passes = []
        for _ in range(int(opt["passes"])):
            c, s = (count.copy(), stats.copy()) if add else (np.empty(E), np.empty((E, 2, D)))
            passes.append(device(add, c, s))
            if not add:
                count, stats = c, s                                # the sums of one pass from zero: what the baseline is held to
        keys = [k for k in passes[0] if k.endswith("_ms")]
        result[name] = dict(ms={k: float(np.median([p[k] for p in passes])) for k in keys},
                            ms_min_max={k: [float(min(p[k] for p in passes)), float(max(p[k] for p in passes))] for k in keys})
    t = passes[0]
    result.update(events_met=int(t["events"]), work_items=int(t["work_items"]), longest_event_frames=int(t["longest"]),
                  longest_event_share=float(t["longest"]) / T, silence_frames_share=float(runs[:5].sum()) / T,
                  median_frames_per_event_met=float(np.median(runs[runs > 0])))
    # the running accumulator over event tuples: the compaction in Python and one library call
    tuples = [events[k] for k in fe.tolist()]
    x = torch.from_numpy(feats).cuda()
    t0 = time.perf_counter()
    ts = api.TreeStats(D, 0.01)
    ts.accumulate(x, tuples)
    result["accumulator_wall_ms"] = (time.perf_counter() - t0) * 1e3
    result["accumulator_library_call_ms"] = float(api.tree_last_timings()["call_ms"])
    items = list(ts.items())
    # the same through a table of events and per-frame indices, as tools/acc_tree_stats.py passes them: utterances of 500
    # frames, each with the table of the events it meets
    tables, codes = [], []
    for u in range(0, T, 500):
        ids, inverse = np.unique(fe[u:u + 500], return_inverse=True)
        codes.append(inverse + sum(map(len, tables)))
        tables.append([events[k] for k in ids.tolist()])
    table, code = [ev for t in tables for ev in t], np.concatenate(codes)
    t0 = time.perf_counter()
    ts2 = api.TreeStats(D, 0.01)
    ts2.accumulate(x, table, codes=code)
    result["accumulator_codes_wall_ms"] = (time.perf_counter() - t0) * 1e3
    result["accumulator_codes_table_entries"] = len(table)
    for (ev, g), (ev2, g2) in zip(items, ts2.items()):
        if ev != ev2 or g["count"] != g2["count"] or not (g["stats"].view(np.int64) == g2["stats"].view(np.int64)).all():
            raise SystemExit("tree_stats_rate: the two accumulator routes differ")
    if int(opt["cpu"]):
        with tempfile.TemporaryDirectory() as d:
            cpu, ms = run_cpu(cpu_baseline(), feats, fe, events, d)
        same = len(cpu) == len(items) == int((runs > 0).sum())
        for (ev, c, s), (ev2, g) in zip(cpu, items):
            same = same and ev == ev2 and c == g["count"] and bool((s.view(np.int64) == np.ascontiguousarray(g["stats"]).view(np.int64)).all())
        by_id = {ev: i for i, ev in enumerate(events)}
        for ev, c, s in cpu:
            i = by_id[ev]
            same = same and c == count[i] and bool((s.view(np.int64) == stats[i].view(np.int64)).all())
        if not same:
            raise SystemExit("tree_stats_rate: the baseline's statistics differ from the library's")
        call = result["from_zero"]["ms"]["call_ms"]
        result.update(cpu_accumulate_ms=ms, bit_equal_to_baseline=True, speedup_call_from_zero=ms / call,
                      speedup_call_running_on=ms / result["running_on"]["ms"]["call_ms"],
                      speedup_kernel=ms / result["from_zero"]["ms"]["kernels_ms"],
                      speedup_upload_and_call=ms / result["from_zero"]["ms"]["wall_ms"],
                      library_call_beats_baseline=bool(call < ms))
    os.makedirs(os.path.dirname(opt["out"]), exist_ok=True)
    with open(opt["out"], "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
