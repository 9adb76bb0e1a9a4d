"""The reference's own answers, stored.  Tests that pin the restatement to the reference's compiled CPU code
(oracle/_ref, buildable only where the reference's sources are) call it through a Reference: where the library is
built the call goes to it, elsewhere the answer it gave to the same inputs is read back from
tests/golden/reference_calls/<test>.npz.  A call is looked up by its name and its place among the test's calls of that
name, and its inputs must match the recorded ones: bit for bit (SHA-256), or - where another CPU's BLAS rounded the test's
own arithmetic differently - in shape, type and sums to 1e-6.  A test whose inputs changed finds no stored answer and
fails instead of comparing against another input's output.

Rewriting the records (where oracle/_ref is built):
    KH_RECORD_REFERENCE=1 python -m pytest -m "not gpu" tests
"""
import hashlib
import json
import os
import re

import numpy as np

RECORDS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_calls")


def _feed(h, obj):
    if isinstance(obj, np.ndarray):
        a = np.ascontiguousarray(obj)
        h.update(b"a" + a.dtype.str.encode() + repr(a.shape).encode())
        h.update(a.tobytes())
    elif isinstance(obj, np.generic):
        _feed(h, np.asarray(obj))
    elif isinstance(obj, dict):
        h.update(b"d%d" % len(obj))
        for k in sorted(obj, key=str):
            _feed(h, str(k))
            _feed(h, obj[k])
    elif isinstance(obj, (list, tuple)):
        h.update(b"l%d" % len(obj))
        for x in obj:
            _feed(h, x)
    elif isinstance(obj, bytes):
        h.update(b"b%d:" % len(obj) + obj)
    elif obj is None or isinstance(obj, (bool, int, float, str)):
        h.update(("%s:%r;" % (type(obj).__name__, obj)).encode())
    else:
        raise TypeError("cannot key a reference call on %r" % type(obj))


def _summary(obj, out):
    """Per leaf of the inputs: arrays by dtype, shape and float64 sums; other values exactly (floats to 1e-12)."""
    if isinstance(obj, (np.ndarray, np.generic)):
        a = np.asarray(obj)
        x = a.astype(np.float64) if a.dtype.kind in "biuf" else np.zeros(0)
        out.append(["a", a.dtype.str, list(a.shape), float(x.sum()), float(np.abs(x).sum())])
    elif isinstance(obj, dict):
        for k in sorted(obj, key=str):
            out.append(["k", str(k)])
            _summary(obj[k], out)
    elif isinstance(obj, (list, tuple)):
        out.append(["n", len(obj)])
        for x in obj:
            _summary(x, out)
    elif isinstance(obj, float):
        out.append(["f", obj])
    elif isinstance(obj, bytes):
        out.append(["x", hashlib.sha256(obj).hexdigest()])
    else:
        out.append(["x", repr(obj)])
    return out


def _close(got, want):
    if len(got) != len(want):
        return False
    for g, w in zip(got, want):
        if g[0] != w[0]:
            return False
        if g[0] == "a":
            if g[1:3] != w[1:3] or abs(g[3] - w[3]) > 1e-6 * (w[4] + 1e-30) or abs(g[4] - w[4]) > 1e-6 * (w[4] + 1e-30):
                return False
        elif g[0] == "f":
            if abs(g[1] - w[1]) > 1e-12 * max(1.0, abs(w[1])):
                return False
        elif g != w:
            return False
    return True


def _pack(obj, prefix, arrays):
    if isinstance(obj, np.ndarray):
        arrays[prefix] = obj
        return "a"
    if isinstance(obj, np.generic):
        arrays[prefix] = np.asarray(obj)
        return "g"
    if isinstance(obj, dict):
        return ["d", {k: _pack(v, "%s.%s" % (prefix, k), arrays) for k, v in obj.items()}]
    if isinstance(obj, (list, tuple)):
        return ["t" if isinstance(obj, tuple) else "l", [_pack(x, "%s.%d" % (prefix, i), arrays) for i, x in enumerate(obj)]]
    if isinstance(obj, bytes):
        return ["b", obj.decode("latin-1")]
    if obj is None or isinstance(obj, (bool, int, float, str)):
        return ["s", obj]
    raise TypeError("cannot store a reference answer of type %r" % type(obj))


def _unpack(spec, prefix, arrays):
    if spec == "a":
        return arrays[prefix]
    if spec == "g":
        return arrays[prefix][()]
    tag, body = spec
    if tag == "d":
        return {k: _unpack(v, "%s.%s" % (prefix, k), arrays) for k, v in body.items()}
    if tag in ("t", "l"):
        xs = [_unpack(v, "%s.%d" % (prefix, i), arrays) for i, v in enumerate(body)]
        return tuple(xs) if tag == "t" else xs
    if tag == "b":
        return body.encode("latin-1")
    return body


def record_path(nodeid):
    name = nodeid.split("/")[-1].replace(".py::", ".")
    return os.path.join(RECORDS, re.sub(r"[^A-Za-z0-9_.\-\[\]]", "_", name) + ".npz")


class Reference:
    """live: the compiled reference (binding.OracleLib("ref")) or None.  Methods of OracleLib are called as
    attributes (ref.softmax_per_row(X)); any other function of the reference goes through call(name, fn, *args)."""

    def __init__(self, nodeid, live, record=False):
        self.live = live
        self.path = record_path(nodeid)
        self.record = bool(record and live is not None)
        self._new = {}
        self._count = {}
        self._stored = None
        if live is None:
            if not os.path.exists(self.path):
                raise FileNotFoundError("no recorded reference answers for %s (%s)" % (nodeid, self.path))
            z = np.load(self.path)
            self._arrays = {k: z[k] for k in z.files}
            self._stored = json.loads(str(self._arrays.pop("__calls__")))

    @property
    def kind(self):
        return "ref"

    def call(self, name, fn, *args, **kwargs):
        k = self._count.get(name, 0)
        self._count[name] = k + 1
        key = "%s.%d" % (name, k)
        h = hashlib.sha256(name.encode())
        _feed(h, list(args))
        _feed(h, dict(kwargs))
        inputs = dict(sha256=h.hexdigest(), summary=_summary([list(args), dict(kwargs)], []))
        if self.live is not None:
            out = fn(*args, **kwargs)
            if self.record:
                self._new[key] = (inputs, out)
            return out
        rec = self._stored.get(key)
        if rec is None or not (rec["sha256"] == inputs["sha256"] or _close(inputs["summary"], rec["summary"])):
            raise KeyError("no recorded reference answer for call %d of %s on these inputs (%s): re-record where oracle/_ref "
                           "is built" % (k, name, self.path))
        return _unpack(rec["out"], key, self._arrays)

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)
        live = self.live
        return lambda *a, **kw: self.call(name, getattr(live, name) if live is not None else None, *a, **kw)

    def save(self):
        if not self.record:
            return
        arrays, specs = {}, {}
        for key, (inputs, out) in self._new.items():
            specs[key] = dict(inputs, out=_pack(out, key, arrays))
        arrays["__calls__"] = np.asarray(json.dumps(specs, sort_keys=True))
        os.makedirs(RECORDS, exist_ok=True)
        np.savez_compressed(self.path, **arrays)
