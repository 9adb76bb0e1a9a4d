"""CPU: tools/gmm_rescore_cpu_baseline.cc - the one-thread yardstick of tools/gmm_rescore_rate.py - gives the restatement's
costs when the restatement is fed the oracle's GMM scores, up to the difference between two CPU scorers (the baseline sums a
Gaussian's two dot products in its own order): 1e-4 relative to the cost's magnitude per transition-id, a sanity bound on a
yardstick, not a claim about the product."""
import importlib
import os
import sys

import numpy as np

import gmm_cases as G
import latalign_cases as A
import rescore_cases as C
import rescore_restatement as R
from conftest import ROOT, pkg

sys.path.insert(0, ROOT)


def test_baseline_agrees_with_the_restatement_on_the_oracles_scores(oracle, tmp_path):
    rate = importlib.import_module("tools.gmm_rescore_rate")
    api = pkg("api")
    exe = rate.cpu_baseline(str(tmp_path))
    off, g, mi, iv, dim, rng = G.build("edge_small_d13", oracle)
    clats = [C.lengths_clat(5, 3), C.long_final_clat(), A.generate(11007, 6), C.negative_zero_clat(), C.plain_clat(7)]
    utt = [C.utt_len_of(c) for c in clats]
    rows = np.concatenate([[0], np.cumsum([u + k % 2 for k, u in enumerate(utt)])]).astype(np.int32)
    rows[-1] -= 2                                              # the last lattice is one frame short: left as it is
    feats = G.frames(rng, int(rows[-1]), dim)
    t2p = C.tid2pdf(len(off) - 1)
    csrs = [api.compact_lattice_align_csr(c) for c in clats]
    res, ms = rate.run_cpu(exe, rate.pack(csrs, rows, t2p, feats, dict(gconsts=g, means_invvars=mi, inv_vars=iv, pdf_offsets=off)))
    assert ms >= 0.0
    scores = oracle.am_gmm_loglikes(feats, g, mi, iv, off, prune=-1.0)
    n_arcs = sum(len(c["arc_src"]) for c in clats)
    a0 = s0 = 0
    for i, c in enumerate(clats):
        status, arc_a, final_a = R.rescore_compact_lattice_internal(c, scores[rows[i]:rows[i + 1]], t2p)
        assert status == (R.FEATURES_TOO_SHORT if i == len(clats) - 1 else R.OK)
        got_a, got_f = res[a0:a0 + len(arc_a)], res[n_arcs + s0:n_arcs + s0 + len(final_a)]
        lens = np.asarray([len(x) for x in c["arc_string"]])
        assert np.all(np.abs(got_a - arc_a) <= 1e-4 * lens * np.maximum(1.0, np.abs(arc_a))), i
        assert np.array_equal(got_a[lens == 0].view(np.int32), np.asarray(c["arc_a"], np.float32)[lens == 0].view(np.int32))
        fin = np.isfinite(final_a)
        flens = np.asarray([len(x) for x in c["final_string"]])
        assert np.array_equal(np.isfinite(got_f), fin)
        assert np.all(np.abs(got_f[fin] - final_a[fin]) <= 1e-4 * np.maximum(flens[fin], 1) * np.maximum(1.0, np.abs(final_a[fin]))), i
        if status == R.OK:
            assert np.any(got_a != np.asarray(c["arc_a"], np.float32))
        a0 += len(arc_a)
        s0 += len(final_a)
    assert os.path.exists(exe)
