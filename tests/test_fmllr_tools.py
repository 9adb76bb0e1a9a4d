"""CPU: the host-only programs of tools/fmllr_tools.py (ali-to-post, weight-silence-post, compose-transforms), the refusals of
the others that come before any device call, and kaldi_io's GaussPost holder (hmm/posterior.cc:141-200) with its fixtures
under tests/golden/kaldi_io/ (written by kaldi_io.write_gauss_post)."""
import importlib
import io
import os
import sys

import numpy as np
import pytest

import fmllr_cases as C
import fmllr_restatement as R
from conftest import GOLDEN, ROOT, pkg

sys.path.insert(0, os.path.join(ROOT, "tools"))


def tool(name):
    return importlib.import_module(name.replace("-", "_"))


GPOST = [[(3, np.array([0.25, 0.5], np.float32))], [], [(0, np.array([1.0], np.float32)), (2, np.array([0.125, -0.5, 1e-8], np.float32))]]


def same_gpost(a, b):
    assert len(a) == len(b)
    for fa, fb in zip(a, b):
        assert [p for p, _ in fa] == [p for p, _ in fb]
        for (_, va), (_, vb) in zip(fa, fb):
            assert va.dtype == np.float32 and np.array_equal(va, vb)


@pytest.mark.parametrize("binary", [True, False])
def test_gauss_post_round_trip_and_fixture(binary):
    kio = pkg("kaldi_io")
    buf = io.BytesIO()
    kio.write_gauss_post(buf, GPOST, binary)
    same_gpost(kio.read_gauss_post(kio.Stream(io.BytesIO(buf.getvalue())), binary), GPOST)
    path = os.path.join(GOLDEN, "kaldi_io", "gpost.bin" if binary else "gpost.txt")
    assert open(path, "rb").read() == buf.getvalue()
    if not binary:
        assert buf.getvalue() == b"3 1 3  [ 0.25 0.5 ]\n0 2 0  [ 1 ]\n2  [ 0.125 -0.5 1e-08 ]\n\n"


def test_gauss_post_table(tmp_path):
    cli, kio = pkg("kaldi_cli"), pkg("kaldi_io")
    for spec in ("ark:", "ark,t:"):
        w = cli.TableWriter(spec + str(tmp_path / "g.ark"), "gauss_post")
        w.write("u1", GPOST)
        w.write("u2", [])
        assert w.close()
        got = dict(cli.SequentialTableReader("ark:" + str(tmp_path / "g.ark"), "gauss_post"))
        same_gpost(got["u1"], GPOST)
        assert got["u2"] == []
    with pytest.raises(ValueError, match="negative size"):
        kio.read_gauss_post(kio.Stream(io.BytesIO(b"-1 ")), False)


def test_ali_to_post_and_weight_silence_post(tmp_path, monkeypatch, capfd, oracle):
    cli, kio = pkg("kaldi_cli"), pkg("kaldi_io")
    monkeypatch.chdir(tmp_path)
    am = C.model(C.E2E_SIZES, C.E2E_DIM, 31, oracle)
    C.e2e_model_files(kio, am, "final.mdl")
    alis = {"a": np.array([1, 2, 3, 4, 12], np.int32), "b": np.array([5], np.int32)}
    w = cli.TableWriter("ark:ali.ark", "int32_vector")
    for k, v in alis.items():
        w.write(k, v)
    w.close()
    assert tool("ali-to-post").main(["ark:ali.ark", "ark,t:post.txt"]) == 0
    assert "LOG (ali-to-post:main()) Converted 2 alignments." in capfd.readouterr().err
    assert open("post.txt").read() == "a [ 1 1 ] [ 2 1 ] [ 3 1 ] [ 4 1 ] [ 12 1 ] \nb [ 5 1 ] \n"
    assert tool("weight-silence-post").main(["0.0", "1:2", "final.mdl", "ark:post.txt", "ark,t:nosil.txt"]) == 0
    assert "LOG (weight-silence-post:main()) Done 2 posteriors." in capfd.readouterr().err
    assert open("nosil.txt").read() == "a [ ] [ ] [ ] [ ] [ 12 1 ] \nb [ 5 1 ] \n"
    assert tool("weight-silence-post").main(["--distribute=true", "0.5", "2", "final.mdl", "ark:post.txt", "ark,t:d.txt"]) == 0
    assert open("d.txt").read() == "a [ 1 1 ] [ 2 1 ] [ 3 0.5 ] [ 4 0.5 ] [ 12 1 ] \nb [ 5 1 ] \n"
    capfd.readouterr()
    assert tool("weight-silence-post").main(["x", "1", "final.mdl", "ark:post.txt", "ark:o"]) == 255
    assert 'Invalid silence-weight parameter: expected float, got "x"' in capfd.readouterr().err
    assert tool("ali-to-post").main(["ark:ali.ark"]) == 1            # usage
    open("empty.ark", "wb").close()
    assert tool("ali-to-post").main(["ark:empty.ark", "ark:o.ark"]) == 1


def test_compose_transforms_tool(tmp_path, monkeypatch, capfd, rng):
    cli, kio = pkg("kaldi_cli"), pkg("kaldi_io")
    monkeypatch.chdir(tmp_path)
    A = {k: rng.standard_normal((13, 14)).astype(np.float32) for k in ("u1", "u2", "u3")}
    B = {k: rng.standard_normal((13, 14)).astype(np.float32) for k in ("u1", "u3")}
    for name, tab in (("a.ark", A), ("b.ark", B)):
        w = cli.TableWriter("ark:" + name, "matrix")
        for k, m in tab.items():
            w.write(k, m)
        w.close()
    assert tool("compose-transforms").main(["--b-is-affine=true", "ark:a.ark", "ark:b.ark", "ark:c.ark"]) == 0
    assert "WARNING (compose-transforms:main()) Second table does not have key u2" in capfd.readouterr().err
    got = dict(kio.read_ark("c.ark"))
    assert sorted(got) == ["u1", "u3"]
    for k in got:
        assert got[k].shape == (13, 14) and np.abs(got[k] - R.compose_transforms(A[k], B[k], True)).max() < 1e-4
    # a global A, a table B; then all files
    with open("lda.mat", "wb") as f:
        f.write(b"\0B")
        kio.write_matrix(f, rng.standard_normal((9, 13)).astype(np.float32), True)
    lda = cli.read_kaldi_object("lda.mat", kio.read_matrix)
    assert tool("compose-transforms").main(["lda.mat", "ark:b.ark", "ark:c2.ark"]) == 0
    got = dict(kio.read_ark("c2.ark"))
    assert np.abs(got["u3"] - lda.astype(np.float64) @ B["u3"]).max() < 1e-4
    assert tool("compose-transforms").main(["--binary=false", "lda.mat", "lda.mat", "c3.mat"]) == 255       # 13 columns against 9 rows
    assert "ComposeTransforms: mismatched dimensions, a has 13 columns and b has 9 rows." in capfd.readouterr().err
    assert tool("compose-transforms").main(["lda.mat", "ark:b.ark", "c4.mat"]) == 255
    assert "Formats of the input and output" in capfd.readouterr().err


def test_rand_prune_is_refused(tmp_path, monkeypatch, capfd, oracle):
    kio = pkg("kaldi_io")
    monkeypatch.chdir(tmp_path)
    C.e2e_model_files(kio, C.model(C.E2E_SIZES, C.E2E_DIM, 31, oracle), "final.mdl")
    assert tool("gmm-post-to-gpost").main(["--rand-prune=0.5", "final.mdl", "ark:f.ark", "ark:p.ark", "ark:g.ark"]) == 255
    assert "RandPrune's random stream is not reproduced" in capfd.readouterr().err
    assert tool("gmm-est-fmllr").main(["--fmllr-update-type=fulll", "final.mdl", "ark:f.ark", "ark:p.ark", "ark:t.ark"]) == 255
    assert "Unknown fMLLR update type fulll" in capfd.readouterr().err
