"""No GPU: the .macc file (kaldi_io.write_mllt_accs / read_mllt_accs / add_mllt_accs) against MlltAccs::Write / Read
(transform/mllt.cc:34-63) over PackedMatrix<double>::Write / Read: the bytes of a binary file for D = 2 spelled out, the
line structure of the text form, write / read / add round trips, and the size-mismatch message of Read(add = true)."""
import io
import struct

import numpy as np
import pytest

from conftest import pkg


def acc2():
    # G_0 = [[1.5, .], [-2, 0.25]], G_1 = [[3, .], [0, -7]] as packed rows
    return dict(beta=12.5, G=np.array([[1.5, -2.0, 0.25], [3.0, 0.0, -7.0]]), dim=2)


def dumps(acc, binary):
    f = io.BytesIO()
    pkg("kaldi_io").write_mllt_accs(f, acc, binary)
    return f.getvalue()


def test_binary_bytes_for_dim_2():
    want = (b"<MlltAccs> " + b"\x08" + struct.pack("<d", 12.5) + b"\x04" + struct.pack("<i", 2) + b"<G> "
            + b"DP " + b"\x04" + struct.pack("<i", 2) + struct.pack("<3d", 1.5, -2.0, 0.25)
            + b"DP " + b"\x04" + struct.pack("<i", 2) + struct.pack("<3d", 3.0, 0.0, -7.0)
            + b"</MlltAccs> ")
    assert dumps(acc2(), True) == want


def test_text_line_structure():
    text = dumps(acc2(), False)
    assert text == (b"<MlltAccs> \n12.5 2 <G> \n[\n1.5 \n-2 0.25 ]\n[\n3 \n0 -7 ]\n</MlltAccs> \n")


@pytest.mark.parametrize("binary", [True, False])
def test_round_trips_and_add(binary):
    kio = pkg("kaldi_io")
    rng = np.random.default_rng(5)
    dim = 5
    acc = dict(beta=1234.5, G=np.round(rng.standard_normal((dim, dim * (dim + 1) // 2)) * 64) / 64, dim=dim)   # exact in 7 digits
    data = dumps(acc, binary)
    got = kio.read_mllt_accs(io.BytesIO(data), binary)
    assert got["dim"] == dim and got["beta"] == acc["beta"] and got["G"].dtype == np.float64 and np.array_equal(got["G"], acc["G"])
    assert dumps(got, binary) == data
    # Read(add = true): into an accumulator of the same size, and into the empty one of a default-constructed MlltAccs
    into = kio.read_mllt_accs(io.BytesIO(data), binary)
    out = kio.read_mllt_accs(io.BytesIO(data), binary, add_into=into)
    assert out is into and out["beta"] == 2 * acc["beta"] and np.array_equal(out["G"], 2 * acc["G"])
    empty = dict(beta=0.0, G=np.zeros((0, 0)), dim=0)
    out = kio.read_mllt_accs(io.BytesIO(data), binary, add_into=empty)
    assert out["dim"] == dim and out["beta"] == acc["beta"] and np.array_equal(out["G"], acc["G"])


def test_through_the_object_holder(tmp_path):
    """As the tool writes it (the binary header in front) and read_kaldi_object reads it."""
    kio = pkg("kaldi_io")
    path = tmp_path / "x.macc"
    path.write_bytes(b"\0B" + dumps(acc2(), True))
    got = kio.read_kaldi_object(str(path), kio.read_mllt_accs)
    assert got["beta"] == 12.5 and np.array_equal(got["G"], acc2()["G"])
    path.write_bytes(dumps(acc2(), False))
    assert np.array_equal(kio.read_kaldi_object(str(path), kio.read_mllt_accs)["G"], acc2()["G"])


def test_adding_different_sizes_is_refused():
    kio, capi = pkg("kaldi_io"), pkg("capi")
    other = dict(beta=1.0, G=np.ones((3, 6)), dim=3)
    with pytest.raises(ValueError, match="MlltAccs::Read, summing accs of different size."):
        kio.read_mllt_accs(io.BytesIO(dumps(other, True)), True, add_into=acc2())
    with pytest.raises(ValueError, match="MlltAccs::Read, summing accs of different size."):
        kio.add_mllt_accs(acc2(), other)
    api = pkg("api")
    with pytest.raises(capi.KhError, match="MlltAccs::Read, summing accs of different size."):
        api.add_mllt_stats(acc2(), other)
    out = api.add_mllt_stats(acc2(), acc2())
    assert out["beta"] == 25.0 and np.array_equal(out["G"], 2 * acc2()["G"])
