"""acc-lda restated line by line in numpy: the binary's loop (bin/acc-lda.cc:69-122) over LdaEstimate::Init, Accumulate, Write
and Read (transform/lda-estimate.cc:26-30, 45-55, 180-260) and RandPrune (base/kaldi-math.h:169-175; imported from
tests/mllt_restatement.py with its generator).  float32 where the reference is float, float64 where it is double.
oracle/_ref does not build transform/, so this file is the yardstick of the LDA tests.

An accumulator is dict(zero [C], first [C, D], second [Q] float64, dim, num_classes): second is total_second_acc_ as
SpMatrix packs it, (r, c), r >= c, at r (r + 1) / 2 + c.  LdaEstimate lda; before Init is dim 0 with 0 classes.

The packed rank-one update SpMatrix<double>::AddVec2(alpha, v) is cblas_dspr(CblasRowMajor, CblasLower, ...), which is the
column-major upper form of the netlib routine:
    for j: temp = alpha * x[j]; for i <= j: ap[k] += x[i] * temp        (k runs over column j: j (j + 1) / 2 + i)
- a product and an addition, each rounded once.  Row r of the row-major lower packing is column j = r of that form, so
second[r (r + 1) / 2 + c] += x[c] * (alpha * x[r]).  Vector::AddVec(alpha, v) is cblas_daxpy: y[i] += alpha * x[i].

The text and binary layouts of Write are restated here too (io-funcs, kaldi-vector.cc, kaldi-matrix.cc, packed-matrix.cc),
on their own, so that kaldi_io.write_lda_accs is held to bytes it did not make.

As a program it runs the binary's loop on a pickled job, in a process of its own whose generator nobody has seeded:
  python tests/lda_restatement.py <job.pkl> <rand-prune> <out.pkl>"""
import io
import pickle
import struct
import sys

import numpy as np

import mllt_restatement as M

F32, F64 = np.float32, np.float64


def empty():
    """LdaEstimate lda;"""
    return dict(zero=np.zeros(0, F64), first=np.zeros((0, 0), F64), second=np.zeros(0, F64), dim=0, num_classes=0)


def init(acc, num_classes, dimension):
    """lda-estimate.cc:26-30."""
    acc.update(zero=np.zeros(num_classes, F64), first=np.zeros((num_classes, dimension), F64),
               second=np.zeros(dimension * (dimension + 1) // 2, F64), dim=int(dimension), num_classes=int(num_classes))
    return acc


def dspr(ap, alpha, x):
    """The netlib packed rank-one update, column by column (see the head of this file)."""
    alpha = F64(alpha)
    for j in range(len(x)):
        temp = alpha * x[j]
        k = j * (j + 1) // 2
        ap[k:k + j + 1] += x[:j + 1] * temp


def accumulate(acc, data, class_id, weight):
    """lda-estimate.cc:45-55."""
    assert 0 <= class_id < acc["num_classes"] and len(data) == acc["dim"]
    data_d = np.asarray(data, F32).astype(F64)                           # Vector<double> data_d(data)
    weight = F32(weight)                                                 # BaseFloat weight
    acc["zero"][class_id] += F64(weight)                                 # zero_acc_(class_id) += weight
    acc["first"][class_id] += F64(weight) * data_d                       # first_acc_.Row(class_id).AddVec(weight, data_d)
    dspr(acc["second"], weight, data_d)                                  # total_second_acc_.AddVec2(weight, data_d)


def acc_lda(num_pdfs, tid2pdf, utts, prune, log=None, trace=None):
    """acc-lda.cc:67-117.  utts: [(features [T, D], posterior over transition-ids, or None when the utterance has none)].
    trace: a list that takes (weight, what RandPrune made of it) per entry.  -> (acc, num_done, num_fail)."""
    lda = empty()
    num_done = num_fail = 0
    for feats, post in utts:
        if post is None:                                                 # "No posteriors for utterance"
            num_fail += 1
            continue
        if lda["dim"] == 0:
            init(lda, num_pdfs, feats.shape[1])
        if feats.shape[0] != len(post):                                  # "Posterior vs. feats size mismatch"
            num_fail += 1
            continue
        if lda["dim"] != 0 and lda["dim"] != feats.shape[1]:             # "Feature dimension mismatch"
            num_fail += 1
            continue
        pdf_post = M.convert_posterior_to_pdfs(tid2pdf, post)
        for i in range(feats.shape[0]):
            for pdf_id, w in pdf_post[i]:
                weight = M.rand_prune(F32(w), F32(prune), log)
                if trace is not None:
                    trace.append((F32(w), weight))
                if weight != 0.0:
                    accumulate(lda, feats[i], pdf_id, weight)
        num_done += 1
    return lda, num_done, num_fail


def mangled(acc):
    """Write's tmp_sec_acc (lda-estimate.cc:251-255), double."""
    tmp = np.array(acc["second"], F64)
    for c in range(acc["num_classes"]):
        if acc["zero"][c] != 0:
            dspr(tmp, -1.0 / acc["zero"][c], acc["first"][c])
    return tmp


# ---- the layouts of Write
def _g(x):
    x = float(x)
    if x != x:
        return "nan"
    if x in (float("inf"), float("-inf")):
        return "inf" if x > 0 else "-inf"
    return "%.7g" % x                                                    # the stream's precision is 7


def _token(f, tok):
    f.write(tok.encode() + b" ")


def _int32(f, binary, v):
    f.write(b"\x04" + struct.pack("<i", v) if binary else b"%d " % v)


def _float_vector(f, binary, v):
    if binary:
        f.write(b"FV \x04" + struct.pack("<i", len(v)) + v.astype("<f4").tobytes())
    else:
        f.write(b" [ " + b"".join((_g(x) + " ").encode() for x in v) + b"]\n")


def _float_matrix(f, binary, m):
    if binary:
        f.write(b"FM \x04" + struct.pack("<i", m.shape[0]) + b"\x04" + struct.pack("<i", m.shape[1]) + m.astype("<f4").tobytes())
    elif m.shape[0] == 0 or m.shape[1] == 0:
        f.write(b" [ ]\n")
    else:
        f.write(b" [")
        for row in m:
            f.write(b"\n  " + b"".join((_g(x) + " ").encode() for x in row))
        f.write(b"]\n")


def _float_packed(f, binary, p, n):
    if binary:
        f.write(b"FP \x04" + struct.pack("<i", n) + p.astype("<f4").tobytes())
    elif n == 0:
        f.write(b"[ ]\n")
    else:
        f.write(b"[\n")
        for r in range(n):
            f.write(b"".join((_g(x) + " ").encode() for x in p[r * (r + 1) // 2:r * (r + 1) // 2 + r + 1]))
            f.write(b"]\n" if r == n - 1 else b"\n")


def write(acc, binary):
    """lda-estimate.cc:237-260 -> bytes (without the "\\0B" of the Output)."""
    f = io.BytesIO()
    _token(f, "<LDAACCS>")
    _token(f, "<VECSIZE>")
    _int32(f, binary, acc["dim"])
    _token(f, "<NUMCLASSES>")
    _int32(f, binary, acc["num_classes"])
    _token(f, "<ZERO_ACCS>")
    _float_vector(f, binary, acc["zero"].astype(F32))                    # Vector<BaseFloat> zero_acc_bf(zero_acc_)
    _token(f, "<FIRST_ACCS>")
    _float_matrix(f, binary, acc["first"].astype(F32))                   # Matrix<BaseFloat> first_acc_bf(first_acc_)
    _token(f, "<SECOND_ACCS>")
    with np.errstate(over="ignore", invalid="ignore"):
        _float_packed(f, binary, mangled(acc).astype(F32), acc["dim"])   # SpMatrix<BaseFloat> tmp_sec_acc_bf(tmp_sec_acc)
    _token(f, "</LDAACCS>")
    return f.getvalue()


def read_values(zero_bf, first_bf, sec_bf, lda=None):
    """lda-estimate.cc:180-235 after the parsing: the FLOAT values of a file's three sections, in the order Write writes
    them, into lda (add = true; None: a fresh accumulator, add = false)."""
    nc, dim = first_bf.shape if first_bf.size else (len(zero_bf), int(round((np.sqrt(8 * len(sec_bf) + 1) - 1) / 2)))
    if lda is None or (lda["num_classes"] == 0 and lda["dim"] == 0):
        lda = init(empty() if lda is None else lda, nc, dim)
    elif (lda["num_classes"], lda["dim"]) != (nc, dim):
        raise ValueError("LdaEstimate::Read, dimension or classes count mismatch, %d, %d,  vs. %d, %d" % (lda["num_classes"], lda["dim"], nc, dim))
    tmp_zero = np.asarray(zero_bf, F32).astype(F64)
    tmp_first = np.asarray(first_bf, F32).astype(F64).reshape(nc, dim)
    tmp_sec = np.asarray(sec_bf, F32).astype(F64)
    lda["zero"] += tmp_zero                                              # zero_acc_.AddVec(1.0, tmp_zero_acc)
    lda["first"] += tmp_first                                            # first_acc_.AddMat(1.0, tmp_first_acc)
    for c in range(nc):
        if tmp_zero[c] != 0:
            dspr(tmp_sec, 1.0 / tmp_zero[c], tmp_first[c])
    lda["second"] += tmp_sec                                             # total_second_acc_.AddSp(1.0, tmp_sec_acc)
    return lda


def read_of_write(acc, lda=None):
    """Read(Write(acc)) without the bytes: the float casts of Write, then read_values."""
    with np.errstate(over="ignore", invalid="ignore"):
        return read_values(acc["zero"].astype(F32), acc["first"].astype(F32), mangled(acc).astype(F32), lda)


def main(argv):
    with open(argv[0], "rb") as f:
        job = pickle.load(f)
    log, trace = [], []
    acc, done, fail = acc_lda(job["num_pdfs"], job["tid2pdf"], job["utts"], float(argv[1]), log, trace)
    with open(argv[2], "wb") as f:
        pickle.dump(dict(acc=acc, done=done, fail=fail, log=log, trace=np.asarray(trace, F32).reshape(-1, 2), draws=M.DRAWS[0]), f)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
