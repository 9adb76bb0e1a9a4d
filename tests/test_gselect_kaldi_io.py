"""No GPU: the files of the diagonal-UBM recipe in kaldi_io - the table of vector<vector<int32>> that gmm-gselect writes
(BasicVectorVectorHolder<int32>, util/kaldi-holder-inl.h:296-420) and the stand-alone AccumDiagGmm file of
gmm-global-acc-stats (gmm/mle-diag-gmm.cc:33-103)."""
import io
import struct

import numpy as np
import pytest

from conftest import pkg

KIO = pkg("kaldi_io")
KIND = "int32_vector_vector"


def _i32(v):
    return b"\x04" + struct.pack("<i", v)          # WriteBasicType<int32>, binary: the size byte, then the value


CASES = {
    "plain": [[1, 2, 3], [4, 5], [6]],
    "empty inner": [[7], [], [8, -9], []],
    "only empty inner": [[]],
    "empty outer": [],
}


def _write(obj, binary):
    f = io.BytesIO()
    KIO._write_object(f, binary, KIND, obj)
    return f.getvalue()


def test_bytes_of_a_hand_case():
    """Written out from the holder's code: binary - the outer size, then per inner vector its size and its elements, each a
    basic type; text - every element followed by a space, every inner vector terminated by "; ", one newline at the end."""
    obj = [[1, 2, 3], [], [-4]]
    assert _write(obj, True) == _i32(3) + _i32(3) + _i32(1) + _i32(2) + _i32(3) + _i32(0) + _i32(1) + _i32(-4)
    assert _write(obj, False) == b"1 2 3 ; ; -4 ; \n"
    assert _write([], True) == _i32(0) and _write([], False) == b"\n"
    assert _write([[]], False) == b"; \n"


@pytest.mark.parametrize("binary", [True, False], ids=["binary", "text"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_round_trip(name, binary):
    obj = CASES[name]
    got = KIO._read_object(KIO.Stream(io.BytesIO(_write(obj, binary))), binary, KIND)
    assert len(got) == len(obj)
    for a, b in zip(got, obj):
        assert a.dtype == np.int32 and a.tolist() == b


def test_text_reader_takes_what_the_holder_takes():
    """Any white space between items, a semicolon right after a number; a newline before the semicolon is refused."""
    rd = lambda b: KIO._read_object(KIO.Stream(io.BytesIO(b)), False, KIND)
    assert [v.tolist() for v in rd(b" 1  2;3 ;\t; \nrest")] == [[1, 2], [3], []]
    with pytest.raises(ValueError, match="No semicolon before newline"):
        rd(b"1 2 \n")
    with pytest.raises(ValueError, match="Unexpected EOF"):
        rd(b"1 2 ; ")


@pytest.mark.parametrize("binary", [True, False], ids=["binary", "text"])
def test_table_round_trip(tmp_path, binary):
    path = str(tmp_path / "gselect.ark")
    with KIO.TableWriter(path, kind=KIND, binary=binary) as w:
        for k, name in enumerate(sorted(CASES)):
            w.write("utt%d" % k, CASES[name])
    got = list(KIO.read_ark(path, KIND))
    assert [k for k, _ in got] == ["utt%d" % k for k in range(len(CASES))]
    for (_, g), name in zip(got, sorted(CASES)):
        assert [v.tolist() for v in g] == CASES[name]


def _acc(rng, G, D, flags):
    return dict(occ=rng.uniform(0, 5, G), mean_acc=rng.standard_normal((G, D)) if flags & 1 else None,
                var_acc=rng.uniform(0, 3, (G, D)) if flags & 2 else None, dim=D, flags=flags)


@pytest.mark.parametrize("binary", [True, False], ids=["binary", "text"])
@pytest.mark.parametrize("flags", [4, 5, 7])
def test_global_accs_are_the_gmmaccs_block_of_the_am_file(binary, flags):
    """write_global_gmm_accs' bytes are the <GMMACCS> ... </GMMACCS> block write_gmm_accs writes for a one-pdf model; read
    back, the floats of the file widened to double."""
    rng = np.random.default_rng(flags)
    acc = _acc(rng, 5, 3, flags)
    f = io.BytesIO()
    KIO.write_global_gmm_accs(f, acc, binary)
    am = io.BytesIO()
    KIO.write_gmm_accs(am, dict(acc, pdf_offsets=np.asarray([0, 5], np.int32), total_like=0.0, total_frames=0.0), binary, tail=False)
    whole = am.getvalue()
    a, b = whole.index(b"<GMMACCS>"), whole.index(b"</GMMACCS>") + len(b"</GMMACCS> ")
    assert f.getvalue() == whole[a:b] and whole[b:] == b""
    back = KIO.read_global_gmm_accs(io.BytesIO(f.getvalue()), binary)
    assert back["dim"] == 3 and back["flags"] == flags
    for k in ("occ", "mean_acc", "var_acc"):
        if acc[k] is None:
            assert back[k] is None
        elif binary:
            assert back[k].dtype == np.float64 and np.array_equal(back[k], acc[k].astype(np.float32).astype(np.float64))
        else:
            assert np.allclose(back[k], acc[k], rtol=1e-5, atol=1e-6)      # the text form holds 6 significant digits


def test_add_and_the_mismatch_message():
    rng = np.random.default_rng(0)
    a, b = _acc(rng, 4, 2, 7), _acc(rng, 4, 2, 7)
    fa, fb = io.BytesIO(), io.BytesIO()
    KIO.write_global_gmm_accs(fa, a)
    KIO.write_global_gmm_accs(fb, b)
    tot = KIO.read_global_gmm_accs(io.BytesIO(fa.getvalue()), add_into=dict(occ=np.zeros(0), mean_acc=None, var_acc=None, dim=0, flags=0))
    tot = KIO.read_global_gmm_accs(io.BytesIO(fb.getvalue()), add_into=tot)
    for k in ("occ", "mean_acc", "var_acc"):
        assert np.array_equal(tot[k], a[k].astype(np.float32).astype(np.float64) + b[k].astype(np.float32).astype(np.float64))
    other = io.BytesIO()
    KIO.write_global_gmm_accs(other, _acc(rng, 3, 2, 5))
    with pytest.raises(ValueError) as e:
        KIO.read_global_gmm_accs(io.BytesIO(other.getvalue()), add_into=tot)
    assert str(e.value) == ("MlEstimatediagGmm::Read, dimension or flags mismatch, 4, 2, mvw vs. 3, 2, 5 "
                            "(mixing accs from different models?")
