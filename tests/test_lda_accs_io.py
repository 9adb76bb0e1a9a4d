"""CPU: kaldi_io.write_lda_accs / read_lda_accs / add_lda_accs against LdaEstimate::Write and Read (transform/lda-estimate.cc:
180-260): a file spelled out byte by byte, equal bytes with the restatement's Write on random accumulators, add with its
mismatch message, the section orders Read's loop accepts, and a file with nothing accumulated.
Fails without write_lda_accs."""
import io

import numpy as np
import pytest

import lda_restatement as L
from conftest import pkg

# C = 2, D = 2.  zero = [2, 4], first = [[2, 4], [4, 8]], second = [[10, 14], [14, 30]].  Write mangles in double:
#   class 0: alpha = -1 / 2, first first^T = [[4, 8], [8, 16]]  -> minus [[2, 4], [4, 8]]
#   class 1: alpha = -1 / 4, first first^T = [[16, 32], [32, 64]] -> minus [[4, 8], [8, 16]]
# every product and sum a small integer, hence exact: the file's matrix is [[4, 2], [2, 6]], packed 4, 2, 6.
SMALL = dict(zero=np.array([2.0, 4.0]), first=np.array([[2.0, 4.0], [4.0, 8.0]]), second=np.array([10.0, 14.0, 30.0]), dim=2, num_classes=2)
F2, F4, F6, F8 = b"\x00\x00\x00\x40", b"\x00\x00\x80\x40", b"\x00\x00\xc0\x40", b"\x00\x00\x00\x41"
I2 = b"\x04\x02\x00\x00\x00"                                                # an int32 in binary: its size, then the value
SMALL_BINARY = (b"<LDAACCS> <VECSIZE> " + I2 + b"<NUMCLASSES> " + I2
                + b"<ZERO_ACCS> FV " + I2 + F2 + F4
                + b"<FIRST_ACCS> FM " + I2 + I2 + F2 + F4 + F4 + F8
                + b"<SECOND_ACCS> FP " + I2 + F4 + F2 + F6
                + b"</LDAACCS> ")
SMALL_TEXT = (b"<LDAACCS> <VECSIZE> 2 <NUMCLASSES> 2 <ZERO_ACCS>  [ 2 4 ]\n"
              b"<FIRST_ACCS>  [\n  2 4 \n  4 8 ]\n"
              b"<SECOND_ACCS> [\n4 \n2 6 ]\n"
              b"</LDAACCS> ")


def written(kio, acc, binary):
    f = io.BytesIO()
    kio.write_lda_accs(f, acc, binary)
    return f.getvalue()


def same(a, b):
    return (a["dim"], a["num_classes"]) == (b["dim"], b["num_classes"]) and all(
        np.asarray(a[k]).shape == np.asarray(b[k]).shape and np.array_equal(a[k], b[k]) for k in ("zero", "first", "second"))


def random_acc(seed, nc, dim):
    rng = np.random.default_rng(seed)
    acc = L.init(L.empty(), nc, dim)
    for i in range(40 + 3 * dim):
        L.accumulate(acc, (rng.standard_normal(dim) * 2 + 0.5).astype(np.float32), int(rng.integers(0, nc)), rng.random() + 0.25)
    return acc


@pytest.mark.parametrize("binary,data", [(True, SMALL_BINARY), (False, SMALL_TEXT)])
def test_small_file_byte_by_byte(binary, data):
    kio = pkg("kaldi_io")
    assert written(kio, SMALL, binary) == data == L.write(SMALL, binary)
    got = kio.read_lda_accs(io.BytesIO(data), binary)
    assert same(got, SMALL) and got["second"].dtype == np.float64          # demangled from the floats: exact here
    assert same(L.read_of_write(SMALL), SMALL)


@pytest.mark.parametrize("nc,dim", [(1, 1), (3, 4), (5, 13), (7, 40)])
def test_write_equals_the_restatements_write(nc, dim):
    kio = pkg("kaldi_io")
    acc = random_acc(10 * nc + dim, nc, dim)
    if nc > 2:
        acc["zero"][1], acc["first"][1] = 0.0, 0.0                         # "if (zero_acc_(c) != 0)"
    for binary in (True, False):
        data = written(kio, acc, binary)
        assert data == L.write(acc, binary)
        got = kio.read_lda_accs(io.BytesIO(data), binary)
        if binary:                                                         # Read(Write(acc)) is the restatement's, bit for bit
            assert same(got, L.read_of_write(acc))
        else:                                                              # the text holds 7 digits
            assert np.allclose(got["second"], acc["second"], rtol=1e-5, atol=1e-5 * np.abs(acc["second"]).max())


def test_add_and_its_mismatch():
    kio = pkg("kaldi_io")
    a, b = random_acc(1, 3, 4), random_acc(2, 3, 4)
    fa, fb = written(kio, a, True), written(kio, b, False)
    lda = kio.read_lda_accs(io.BytesIO(fa), True, add_into=kio.empty_lda_accs())         # an empty accumulator takes the sizes
    out = kio.read_lda_accs(io.BytesIO(fb), False, add_into=lda)
    assert out is lda
    want = L.read_of_write(a)
    ra = {k: np.array(want[k]) for k in ("zero", "first", "second")}
    tb = kio.read_lda_accs(io.BytesIO(fb), False)
    assert all(np.array_equal(lda[k], ra[k] + tb[k]) for k in ra)
    other = written(kio, random_acc(3, 4, 4), True)
    with pytest.raises(ValueError, match="LdaEstimate::Read, dimension or classes count mismatch, 3, 4,  vs. 4, 4"):
        kio.read_lda_accs(io.BytesIO(other), True, add_into=lda)
    with pytest.raises(ValueError, match="dimension or classes count mismatch, 3, 4,  vs. 3, 5"):
        kio.add_lda_accs(lda, random_acc(4, 3, 5))
    assert same(kio.add_lda_accs(kio.empty_lda_accs(), a), a)


def test_section_orders():
    """Read's loop takes the sections by their tokens: the rows before the counts is fine, a section may be absent (zeros),
    an unknown token is an error; <SECOND_ACCS> is demangled with the counts and rows read BEFORE it."""
    kio = pkg("kaldi_io")
    head = b"<LDAACCS> <VECSIZE> " + I2 + b"<NUMCLASSES> " + I2
    zero = b"<ZERO_ACCS> FV " + I2 + F2 + F4
    first = b"<FIRST_ACCS> FM " + I2 + I2 + F2 + F4 + F4 + F8
    second = b"<SECOND_ACCS> FP " + I2 + F4 + F2 + F6
    assert same(kio.read_lda_accs(io.BytesIO(head + first + zero + second + b"</LDAACCS> "), True), SMALL)
    got = kio.read_lda_accs(io.BytesIO(head + zero + b"</LDAACCS> "), True)
    assert got["zero"].tolist() == [2.0, 4.0] and not got["first"].any() and not got["second"].any() and got["first"].shape == (2, 2)
    with pytest.raises(ValueError, match="<SECOND_ACCS> before the counts and rows"):
        kio.read_lda_accs(io.BytesIO(head + second + zero + first + b"</LDAACCS> "), True)
    with pytest.raises(ValueError, match="Unexpected token '<THIRD_ACCS>' in file"):
        kio.read_lda_accs(io.BytesIO(head + zero + b"<THIRD_ACCS> "), True)
    with pytest.raises(ValueError):
        kio.read_lda_accs(io.BytesIO(b"<LDAACCS> <NUMCLASSES> " + I2), True)


@pytest.mark.parametrize("binary", [True, False])
def test_nothing_accumulated(binary):
    """LdaEstimate lda; lda.Write(...): dim 0 and 0 classes, empty sections."""
    kio = pkg("kaldi_io")
    data = written(kio, kio.empty_lda_accs(), binary)
    assert data == L.write(L.empty(), binary)
    if binary:
        zero4 = b"\x04\x00\x00\x00\x00"
        assert data == (b"<LDAACCS> <VECSIZE> " + zero4 + b"<NUMCLASSES> " + zero4 + b"<ZERO_ACCS> FV " + zero4 + b"<FIRST_ACCS> FM " + zero4 + zero4
                        + b"<SECOND_ACCS> FP " + zero4 + b"</LDAACCS> ")
    else:
        assert data == b"<LDAACCS> <VECSIZE> 0 <NUMCLASSES> 0 <ZERO_ACCS>  [ ]\n<FIRST_ACCS>  [ ]\n<SECOND_ACCS> [ ]\n</LDAACCS> "
    got = kio.read_lda_accs(io.BytesIO(data), binary)
    assert got["dim"] == 0 and got["num_classes"] == 0 and got["zero"].shape == (0,) and got["first"].shape == (0, 0) and got["second"].shape == (0,)
    # an accumulator Init'ed and never added to: the sizes, zeros
    z = L.init(L.empty(), 3, 2)
    back = kio.read_lda_accs(io.BytesIO(written(kio, z, binary)), binary)
    assert same(back, z)
