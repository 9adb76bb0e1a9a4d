#!/usr/bin/env python3
"""The word-alignment stage alone: kh_compact_lattice_align_words on the determinized CompactLattices of a structured decode
(those of tools/lattice_prune_rate.py).  python tools/lattice_align_rate.py [n_utterances [copies]] [--out FILE]

The bench set's model has no word-position phones: transition-id 2k + 1 is taken as the one final transition of phone k + 1,
2k + 2 as its self-loop, and every phone as a singleton word; where the lattice's word labels do not line up with that the
aligner forces words out and flags the lattice, which is work of the same kind.  The set is used as it is.
 (a) the C call, split as kh_compact_lattice_align_words_last_timings splits it (call_ms = the whole C call by the host's
     clock; wall_ms includes the Python packing around it);
 (b) tools/latalign_cpu_baseline.cc (g++ -O2, one thread, a process of its own; its own clock around the alignment, file
     reading excluded) over the same arrays, and whether it agrees with the library in every output bit for bit.
Prints one JSON object with lattices per second for each and their ratio, and writes it to
profiles/lattice_align_bench.json (or --out).  No threshold is set on any of these."""
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
ORDER = ("lat_state_offsets", "lat_start", "arc_offsets", "arc_label", "arc_nextstate", "arc_graph", "arc_acoustic",
         "arc_string_offsets", "arc_strings", "final_graph", "final_acoustic", "final_string_offsets", "final_strings", "tid_phone",
         "tid_is_final", "tid_is_self_loop", "phone_type")


def cpu_baseline(out_dir=None, extra_flags=()):
    """tools/latalign_cpu_baseline.cc as a program (built when missing or older than its source); returns its path."""
    src = os.path.join(ROOT, "tools", "latalign_cpu_baseline.cc")
    exe = os.path.join(out_dir or os.path.join(ROOT, PKG, "build"), "latalign_cpu_baseline")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    if not os.path.exists(exe) or os.path.getmtime(exe) < os.path.getmtime(src):
        subprocess.check_call(["g++", "-O2", "-std=c++14", "-ffp-contract=off"] + list(extra_flags) + [src, "-o", exe])
    return exe


def pack(csrs, tmodel, wbinfo, max_states=0):
    """The batch as the baseline reads it (api.compact_lattice_align_words_pack's arrays, each behind its int64 count)."""
    api = importlib.import_module(PKG + ".api")
    A = api.compact_lattice_align_words_pack(csrs, tmodel, wbinfo, max_states)
    parts = [A[k] for k in ORDER] + [np.asarray([A["reorder"], A["silence_label"], A["partial_word_label"]], np.int32), A["max_states"]]
    le = lambda x: np.ascontiguousarray(x).astype(x.dtype.newbyteorder("<")).tobytes()
    return b"".join(le(np.asarray([x.size], np.int64)) + le(x) for x in parts), len(csrs)


def unpack(data, n):
    """The baseline's output file -> api.compact_lattice_align_words_raw's list of dicts."""
    at = 0

    def take(dt, count):
        nonlocal at
        x = np.frombuffer(data, np.dtype(dt).newbyteorder("<"), count, at)
        at += x.nbytes
        return x.astype(dt)

    out = []
    for _ in range(n):
        status, nt, ns, na, nw = (int(x) for x in take(np.int32, 5))
        fg, fa = take(np.float32, ns), take(np.float32, ns)
        src, dst, lab = take(np.int32, na), take(np.int32, na), take(np.int32, na)
        g, a, ln = take(np.float32, na), take(np.float32, na), take(np.int32, na)
        strs = take(np.int32, nw)
        ends = np.cumsum(ln)
        arcs = [(int(src[k]), int(dst[k]), int(lab[k]), g[k], a[k], tuple(strs[int(ends[k]) - int(ln[k]):int(ends[k])].tolist()))
                for k in range(na)]
        out.append(dict(status=status, n_tuples=nt, n_states=ns, final=np.stack([fg, fa], axis=1), arcs=arcs))
    if at != len(data):
        raise ValueError("latalign_cpu_baseline: %d bytes of output, %d read" % (len(data), at))
    return out


def run_cpu(exe, packed, work_dir=None, repeat=1):
    """The baseline, as a process, on pack()'s bytes.  Returns (unpack()'s result, milliseconds of its best pass).  Raises
    ValueError with the program's message when it refuses its input."""
    data, n = packed
    with tempfile.TemporaryDirectory(dir=work_dir) as d:
        fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        with open(fin, "wb") as f:
            f.write(data)
        r = subprocess.run([exe, fin, fout, str(repeat)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        if r.returncode != 0:
            raise ValueError(r.stderr.decode(errors="replace").strip() or "latalign_cpu_baseline: exit status %d" % r.returncode)
        with open(fout, "rb") as f:
            return unpack(f.read(), n), float(r.stdout.decode().strip())


def same_answer(a, b):
    """Bit for bit, every output of every lattice."""
    bits = lambda x: np.asarray(x, np.float32).reshape(-1).view(np.int32)
    for x, y in zip(a, b):
        if (x["status"], x["n_tuples"], x["n_states"], len(x["arcs"])) != (y["status"], y["n_tuples"], y["n_states"], len(y["arcs"])):
            return False
        if not np.array_equal(bits(x["final"]), bits(y["final"])):
            return False
        for p, q in zip(x["arcs"], y["arcs"]):
            if p[:3] != q[:3] or p[5] != q[5] or not np.array_equal(bits(p[3:5]), bits(q[3:5])):
                return False
    return True


def bench_model(n_pdfs=600):
    tids = 2 * n_pdfs
    phone = np.zeros(tids + 1, np.int32)
    phone[1:] = 1 + (np.arange(tids) // 2)
    fin = np.zeros(tids + 1, bool)
    fin[1::2] = True
    loop = np.zeros(tids + 1, bool)
    loop[2::2] = True
    types = np.full(n_pdfs + 1, 3, np.int32)
    types[0] = 0
    return (dict(tid2phone=phone, tid_is_final=fin, tid_is_self_loop=loop),
            dict(phone_to_type=types, reorder=False, silence_label=0, partial_word_label=0))


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_path = os.path.join(ROOT, "profiles", "lattice_align_bench.json")
    if "--out" in sys.argv:
        out_path = sys.argv[sys.argv.index("--out") + 1]
        args = [a for a in args if a != out_path]
    n_take = int(args[0]) if args else 16
    copies = int(args[1]) if len(args) > 1 else 4
    exe = cpu_baseline()
    api = importlib.import_module(PKG + ".api")
    api.select_gpu(0)
    from tools.lattice_prune_rate import decoded_compact_lattices
    clats, frames = decoded_compact_lattices(api, n_take)
    clats = clats * copies
    n = len(clats)
    tm, wb = bench_model()
    csrs = [api.compact_lattice_align_csr(c) for c in clats]
    out = dict(lattices=n, distinct_lattices=n // copies, frames=frames * copies, states=sum(int(L["n_states"]) for L in csrs),
               arcs=sum(len(L["arc_label"]) for L in csrs))
    best = None
    for _ in range(3):
        t0 = time.perf_counter()
        raw = api.compact_lattice_align_words_raw(csrs, tm, wb)
        dt = (time.perf_counter() - t0) * 1e3
        if best is None or dt < best[0]:
            best = (dt, raw, api.compact_lattice_align_words_last_timings())
    a_ms, raw, split = best
    out["statuses"] = np.bincount([r["status"] for r in raw], minlength=5).tolist()
    out["out_states"] = sum(r["n_states"] for r in raw)
    out["a_device_call"] = dict(wall_ms=a_ms, lattices_per_s=n / (split["call_ms"] * 1e-3), **split)
    cpu, c_ms = run_cpu(exe, pack(csrs, tm, wb), repeat=3)
    out["b_cpu_one_thread"] = dict(ms=c_ms, lattices_per_s=n / (c_ms * 1e-3), agrees=same_answer(cpu, raw))
    out["device_over_cpu"] = c_ms / split["call_ms"]
    text = json.dumps(out, indent=1)
    print(text)
    with open(out_path, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
