"""CPU: kaldi_io.write_gmm_accs / read_gmm_accs, the .acc file between gmm-acc-stats-* and gmm-est.  The bytes are spelled
out from the reference's Write lines: Vector<double>::Write of the transition accumulators, then AccumAmDiagGmm::Write
(gmm/mle-am-diag-gmm.cc:153-166) over AccumDiagGmm::Write (gmm/mle-diag-gmm.cc:77-103) with WriteBasicType
(base/io-funcs-inl.h:32-50: a size byte, negative for an unsigned type, then the value) and WriteToken (the token and a
space)."""
import io
import struct

import numpy as np
import pytest

from conftest import pkg


def one_pdf(flags=7):
    return dict(occ=np.array([1.5]), mean_acc=np.array([[1.25, 4.0]]) if flags & 1 else None,
                var_acc=np.array([[1.125, 12.0]]) if flags & 2 else None, pdf_offsets=np.array([0, 1], np.int32), dim=2, flags=flags,
                total_like=-3.5, total_frames=1.5, transition_accs=np.array([0.0, 2.0]))


def i32(v):
    return b"\x04" + struct.pack("<i", v)


def expected_binary(flags=7, tail=True):
    b = b"DV " + i32(2) + struct.pack("<2d", 0.0, 2.0)                               # transition_accs.Write
    b += b"<NUMPDFS> " + i32(1)                                                      # mle-am-diag-gmm.cc:155-156
    b += b"<GMMACCS> " + b"<VECSIZE> " + i32(2) + b"<NUMCOMPONENTS> " + i32(1)       # mle-diag-gmm.cc:78-82
    b += b"<FLAGS> " + b"\xfe" + struct.pack("<H", flags)                            # :83-84, GmmFlagsType = uint16: size byte -2
    b += b"<OCCUPANCY> " + b"FV " + i32(1) + struct.pack("<f", 1.5)                  # :96-97, converted to BaseFloat
    b += b"<MEANACCS> " + (b"FM " + i32(1) + i32(2) + struct.pack("<2f", 1.25, 4.0) if flags & 1 else b"FM " + i32(0) + i32(0))
    b += b"<DIAGVARACCS> " + (b"FM " + i32(1) + i32(2) + struct.pack("<2f", 1.125, 12.0) if flags & 2 else b"FM " + i32(0) + i32(0))
    b += b"</GMMACCS> "
    if tail:
        b += b"<total_like> " + b"\x08" + struct.pack("<d", -3.5) + b"<total_frames> " + b"\x08" + struct.pack("<d", 1.5)   # :161-165
    return b


def write(acc, binary, **kw):
    f = io.BytesIO()
    pkg("kaldi_io").write_gmm_accs(f, acc, binary, **kw)
    return f.getvalue()


def read(data, binary, **kw):
    return pkg("kaldi_io").read_gmm_accs(io.BytesIO(data), binary, **kw)


def same(a, b):
    for k in ("occ", "mean_acc", "var_acc", "transition_accs"):
        assert (a[k] is None) == (b[k] is None) and (a[k] is None or (np.array_equal(a[k], b[k]) and a[k].dtype == np.float64)), k
    return (a["flags"], a["dim"], a["total_like"], a["total_frames"], a["pdf_offsets"].tolist()) == \
        (b["flags"], b["dim"], b["total_like"], b["total_frames"], b["pdf_offsets"].tolist())


@pytest.mark.parametrize("flags", [15, 7, 5, 4])
def test_binary_bytes_and_round_trip(flags):
    acc = one_pdf(flags)
    data = write(acc, True)
    assert data == expected_binary(flags)
    assert same(read(data, True), acc)


def test_bytes_of_the_binaries_default_flags():
    """gmm-acc-stats-ali and -twofeats Init with kGmmAll = 0x0F, gmm-acc-stats with StringToGmmFlags("mvwt") = 0x0F;
    AugmentGmmFlags (model-common.cc:52-62) only adds bits, Resize stores the result (mle-diag-gmm.cc:110) and Write emits it
    (:84): every pdf's block holds <FLAGS> fe 0f 00, in text 15."""
    data = write(one_pdf(15), True)
    assert b"<NUMCOMPONENTS> \x04\x01\x00\x00\x00<FLAGS> \xfe\x0f\x00<OCCUPANCY> FV \x04\x01\x00\x00\x00\x00\x00\xc0\x3f<MEANACCS> FM " in data
    assert data == expected_binary(15) and read(data, True)["flags"] == 15
    text = write(one_pdf(15), False)
    assert b"<NUMCOMPONENTS> 1 <FLAGS> 15 <OCCUPANCY>  [ 1.5 ]\n" in text and read(text, False)["flags"] == 15


def test_text_bytes_and_round_trip():
    data = write(one_pdf(), False)
    assert data == (b" [ 0 2 ]\n<NUMPDFS> 1 <GMMACCS> <VECSIZE> 2 <NUMCOMPONENTS> 1 <FLAGS> 7 <OCCUPANCY>  [ 1.5 ]\n"
                    b"<MEANACCS>  [\n  1.25 4 ]\n<DIAGVARACCS>  [\n  1.125 12 ]\n</GMMACCS> <total_like> -3.5 <total_frames> 1.5 ")
    assert same(read(data, False), one_pdf())
    for flags in (5, 4):
        assert same(read(write(one_pdf(flags), False), False), one_pdf(flags))


def test_values_are_floats_in_the_file():
    acc = one_pdf()
    acc["occ"] = np.array([1.0 + 2.0 ** -30])
    acc["mean_acc"] = np.array([[0.1, 1e10 + 1]])
    got = read(write(acc, True), True)
    assert got["occ"][0] == 1.0 and got["mean_acc"][0, 0] == float(np.float32(0.1)) and got["mean_acc"][0, 1] == float(np.float32(1e10 + 1))
    assert got["total_like"] == -3.5                                     # the totals stay double
    acc["total_like"] = -1.0 / 3.0
    assert read(write(acc, True), True)["total_like"] == -1.0 / 3.0


def test_several_pdfs_round_trip():
    rng = np.random.default_rng(3)
    off = np.array([0, 2, 3, 7], np.int32)
    acc = dict(occ=rng.random(7).astype(np.float32).astype(np.float64), mean_acc=rng.standard_normal((7, 3)).astype(np.float32).astype(np.float64),
               var_acc=rng.random((7, 3)).astype(np.float32).astype(np.float64), pdf_offsets=off, dim=3, flags=7, total_like=-12.25,
               total_frames=4.0, transition_accs=np.arange(5.0))
    assert same(read(write(acc, True), True), acc)
    text = read(write(acc, False), False)                              # text: 7 significant digits
    assert text["pdf_offsets"].tolist() == off.tolist() and np.allclose(text["mean_acc"], acc["mean_acc"], rtol=1e-6)
    assert np.array_equal(text["transition_accs"], np.arange(5.0))


def test_file_without_the_totals():
    """Older accumulators end after the last </GMMACCS> (mle-am-diag-gmm.cc:140-150)."""
    for binary in (True, False):
        data = write(one_pdf(), binary, tail=False)
        if binary:
            assert data == expected_binary(tail=False)
        got = read(data, binary)
        assert got["total_like"] == 0.0 and got["total_frames"] == 0.0 and got["occ"][0] == 1.5


def test_add_into():
    a = read(write(one_pdf(), True), True)
    out = read(write(one_pdf(), True), True, add_into=a)
    assert out is a and a["occ"][0] == 3.0 and a["var_acc"].tolist() == [[2.25, 24.0]] and a["total_like"] == -7.0
    assert a["transition_accs"].tolist() == [0.0, 4.0] and a["total_frames"] == 3.0
    two = dict(one_pdf(), occ=np.array([1.0, 2.0]), mean_acc=np.zeros((2, 2)), var_acc=np.zeros((2, 2)), pdf_offsets=np.array([0, 1, 2], np.int32))
    with pytest.raises(ValueError, match=r"Adding accumulators but num-pdfs do not match: 1 vs\. 2"):
        read(write(two, True), True, add_into=a)
    wide = dict(one_pdf(), mean_acc=np.zeros((1, 3)), var_acc=np.zeros((1, 3)), dim=3)
    with pytest.raises(ValueError, match=r"MlEstimatediagGmm::Read, dimension or flags mismatch, 1, 2, mvw vs\. 1, 3, 7 \(mixing accs from different models\?"):
        read(write(wide, True), True, add_into=a)
    with pytest.raises(ValueError, match=r"dimension or flags mismatch, 1, 2, mvw vs\. 1, 2, 5"):
        read(write(one_pdf(5), True), True, add_into=a)
    with pytest.raises(ValueError, match=r"dimension or flags mismatch, 1, 2, mvw vs\. 1, 2, 15"):
        read(write(one_pdf(15), True), True, add_into=a)                 # the t bit counts, as in the reference
    b15 = read(write(one_pdf(15), True), True)
    with pytest.raises(ValueError, match=r"dimension or flags mismatch, 1, 2, mvwt vs\. 1, 2, 7"):
        read(write(one_pdf(7), True), True, add_into=b15)
    assert read(write(one_pdf(15), True), True, add_into=b15)["occ"][0] == 3.0 and b15["flags"] == 15
    comps = dict(one_pdf(), occ=np.zeros(2), mean_acc=np.zeros((2, 2)), var_acc=np.zeros((2, 2)), pdf_offsets=np.array([0, 2], np.int32))
    with pytest.raises(ValueError, match=r"dimension or flags mismatch, 1, 2, mvw vs\. 2, 2, 7"):
        read(write(comps, True), True, add_into=a)
    assert a["occ"][0] == 3.0                                            # a failed add leaves the accumulator as it was


def test_wrong_flags_type_is_refused():
    data = expected_binary().replace(b"<FLAGS> \xfe\x07\x00", b"<FLAGS> \x04\x07\x00\x00\x00")
    with pytest.raises(ValueError, match="GmmFlagsType"):
        read(data, True)
