"""Models, features and lists for the Gaussian-selection tests (tests/test_gpu_gselect.py, tests/test_gpu_global_acc.py)."""
import numpy as np

F32 = np.float32


def model(seed, G, D, same=()):
    """A random DiagGmm as dict(gconsts, means_invvars, inv_vars) float32.  same: (a, b) pairs - Gaussian b becomes a copy of a."""
    rng = np.random.default_rng(seed)
    iv = rng.uniform(0.5, 2.0, (G, D)).astype(F32)
    mi = (rng.standard_normal((G, D)) * iv).astype(F32)
    m = dict(gconsts=rng.uniform(-8, -4, G).astype(F32), means_invvars=mi, inv_vars=iv)
    for a, b in same:
        for k in m:
            m[k][b] = m[k][a]
    return m


def features(seed, T, D, stride=None):
    """[T, D] float32; with stride > D the rows of a wider array whose other columns hold NaN (they must never be read)."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((T, D)).astype(F32)
    if stride is None:
        return x, x
    wide = np.full((T, stride), np.nan, F32)
    wide[:, :D] = x
    return x, wide


def device_model(api, m):
    return api.AmDiagGmm(m["gconsts"], m["means_invvars"], m["inv_vars"], np.asarray([0, len(m["gconsts"])], np.int32))


def device_features(x, wide):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(wide)).cuda()
    return t if wide is x else t[:, :x.shape[1]]


def lists(seed, T, G, lengths, kind):
    """A list per frame, its length cycling through `lengths` (capped at G): kind "contiguous" (a run from a random start),
    "scattered" (ascending, with gaps) or "unsorted" (a random order)."""
    rng = np.random.default_rng(seed)
    out = []
    for t in range(T):
        n = min(int(lengths[t % len(lengths)]), G)
        if kind == "contiguous":
            s = int(rng.integers(0, G - n + 1))
            out.append(np.arange(s, s + n, dtype=np.int32))
        else:
            v = rng.choice(G, n, replace=False).astype(np.int32)
            out.append(np.sort(v) if kind == "scattered" else v)
    return out
