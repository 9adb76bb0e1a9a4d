"""CPU: bench.py --dump-outputs.  dump_outputs() writes what the timed step hands its caller (best paths, lattice sizes,
seeded samples of the scores and the raw lattices) as finite float32 / float64 .npy files within 64 MB, the same files for
the same decoder state; --steps below 1 is refused (ms_per_step is the elapsed time over --steps)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import bench  # noqa: E402


class FakeDecoder:
    """The decoder calls dump_outputs() makes, on fixed data: 40 utterances."""

    def __init__(self, off):
        self.off = off
        self.n = len(off) - 1

    def get_best_paths(self):
        rng = np.random.default_rng(1)
        nw = rng.integers(0, 5, self.n)
        wo = np.concatenate([[0], np.cumsum(nw)]).astype(np.int64)
        return dict(alignment=rng.integers(1, 12000, int(self.off[-1])).astype(np.int32), ali_off=self.off.astype(np.int64),
                    words=rng.integers(1, 200000, int(wo[-1])).astype(np.int32), words_off=wo,
                    graph_cost=rng.standard_normal(self.n).astype(np.float32),
                    acoustic_cost=rng.standard_normal(self.n).astype(np.float32))

    def stats_batch(self, counters=True):
        s = np.zeros(self.n, dtype=[("num_tokens", np.int32), ("num_links", np.int32)])
        s["num_tokens"], s["num_links"] = np.arange(self.n) + 3, 2 * np.arange(self.n) + 5
        return None, s

    def get_raw_lattice(self, u):
        n, m = u + 3, 2 * u + 5
        i = lambda k, hi: np.random.default_rng(1000 * u + k).integers(0, hi, m if k > 2 else n).astype(np.int32)
        f = lambda k, cnt: np.random.default_rng(1000 * u + k).standard_normal(cnt).astype(np.float32)
        final = f(2, n)
        final[np.random.default_rng(u).random(n) < 0.7] = np.inf       # +inf: not a final state (kh_decoder_get_raw_lattice)
        return dict(state_frame=i(0, 50), state_hclg=i(1, 10 ** 6), state_final=final, arc_src=i(3, n), arc_dst=i(4, n),
                    arc_il=i(5, 12000), arc_ol=i(6, 200000), arc_g=f(7, m), arc_a=f(8, m))


def _dump(tmp, poison=None):
    lens = np.random.default_rng(0).integers(10, 60, 40)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    scores = np.random.default_rng(2).standard_normal((int(off[-1]), 36)).astype(np.float32)
    if poison is not None:
        scores[:, 5] = poison
    loglikes = torch.from_numpy(scores)[:, :33]
    dec = FakeDecoder(off)
    nfiles, nbytes = bench.dump_outputs(str(tmp), dec, loglikes, off)
    files = {f[:-4]: np.load(os.path.join(str(tmp), f)) for f in sorted(os.listdir(str(tmp)))}
    return dec, loglikes, off, nfiles, nbytes, files


def test_dump_outputs_writes_what_the_step_returns(tmp_path):
    dec, loglikes, off, nfiles, nbytes, files = _dump(tmp_path / "a")
    assert nfiles == len(files) and nbytes <= 64 << 20
    assert all(a.dtype in (np.float32, np.float64) and np.isfinite(a).all() for a in files.values())
    bp = dec.get_best_paths()
    assert np.array_equal(files["best_path_utterances"], np.arange(40))
    assert np.array_equal(files["best_path_alignment"], bp["alignment"].astype(np.float64))
    assert np.array_equal(files["best_path_words"], bp["words"].astype(np.float64))
    assert np.array_equal(files["best_path_words_offsets"], bp["words_off"].astype(np.float64))
    assert np.array_equal(files["best_path_graph_cost"], bp["graph_cost"])
    assert np.array_equal(files["lattice_num_links"], 2 * np.arange(40) + 5.0)
    rows = files["loglikes_sample_rows"].astype(np.int64)
    assert np.array_equal(files["loglikes_sample"], loglikes.numpy()[rows])
    so, ao = files["raw_lattice_state_offsets"].astype(np.int64), files["raw_lattice_arc_offsets"].astype(np.int64)
    fo = files["raw_lattice_final_offsets"].astype(np.int64)
    assert fo[-1] > 0
    for k, u in enumerate(files["raw_lattice_utterances"].astype(np.int64)):
        L = dec.get_raw_lattice(int(u))
        assert np.array_equal(files["raw_lattice_arc_il"][ao[k]:ao[k + 1]], L["arc_il"].astype(np.float64))
        assert np.array_equal(files["raw_lattice_state_hclg"][so[k]:so[k + 1]], L["state_hclg"].astype(np.float64))
        final = np.full(so[k + 1] - so[k], np.inf, np.float32)      # the final weights, rebuilt from the final states
        final[files["raw_lattice_final_states"][fo[k]:fo[k + 1]].astype(np.int64)] = files["raw_lattice_final_cost"][fo[k]:fo[k + 1]]
        assert np.array_equal(final, L["state_final"])
    # the same state gives the same files
    files_b = _dump(tmp_path / "b")[-1]
    assert files.keys() == files_b.keys() and all(np.array_equal(files[k], files_b[k]) for k in files)


@pytest.mark.parametrize("poison", [np.nan, -np.inf])
def test_dump_outputs_refuses_non_finite_values(tmp_path, poison):
    with pytest.raises(ValueError, match="loglikes_sample"):
        _dump(tmp_path / "c", poison)
    assert not os.path.exists(tmp_path / "c") or not os.listdir(tmp_path / "c")


def test_steps_below_one_are_refused():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0", "--no-gpu-dryrun"],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode != 0 and b"--steps" in p.stderr
