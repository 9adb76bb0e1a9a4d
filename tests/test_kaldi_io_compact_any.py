"""CPU: the holder kind "compact_lattice_converted" (CompactLatticeHolder::Read, lat/kaldi-lattice.cc:310-392) on binary
and text tables of both forms: a CompactLattice table comes back as read_compact_lattice reads it, a Lattice table as
lattice_to_compact_lattice of read_lattice."""
import io

import numpy as np
import pytest

import latalign_cases as A
import rescore_restatement as R
from conftest import pkg


def tables(tmp_path, binary):
    cli, kio = pkg("kaldi_cli"), pkg("kaldi_io")
    clats = [("utt_%d" % i, A.generate(11100 + i, 4 + i % 3)) for i in range(4)]
    lats = [(k, kio.compact_lattice_to_lattice(c)) for k, c in clats]
    for _, L in lats:
        L["state_frame"] = np.zeros(L["num_states"], np.int32)      # (write_lattice takes the decoder's raw-lattice dict)
    flag = "" if binary else ",t"
    cpath, lpath = tmp_path / ("c%d.ark" % binary), tmp_path / ("l%d.ark" % binary)
    w = cli.TableWriter("ark%s:%s" % (flag, cpath), "compact_lattice")
    for k, c in clats:
        w.write(k, c)
    w.close()
    w = cli.TableWriter("ark%s:%s" % (flag, lpath), "lattice")
    for k, L in lats:
        w.write(k, L)
    w.close()
    return cpath, lpath, [k for k, _ in clats]


@pytest.mark.parametrize("binary", [True, False])
def test_compact_table_comes_back_as_it_is(tmp_path, binary):
    cli = pkg("kaldi_cli")
    cpath, _, keys = tables(tmp_path, binary)
    got = list(cli.SequentialTableReader("ark:%s" % cpath, "compact_lattice_converted"))
    want = list(cli.SequentialTableReader("ark:%s" % cpath, "compact_lattice"))
    assert [k for k, _ in got] == keys == [k for k, _ in want]
    for (_, g), (_, w) in zip(got, want):
        R.same_clat(g, w)


@pytest.mark.parametrize("binary", [True, False])
def test_lattice_table_comes_back_converted(tmp_path, binary):
    cli, kio = pkg("kaldi_cli"), pkg("kaldi_io")
    _, lpath, keys = tables(tmp_path, binary)
    got = list(cli.SequentialTableReader("ark:%s" % lpath, "compact_lattice_converted"))
    raw = list(cli.SequentialTableReader("ark:%s" % lpath, "lattice"))
    assert [k for k, _ in got] == keys
    for (_, g), (_, L) in zip(got, raw):
        R.same_clat(g, kio.lattice_to_compact_lattice(L))
        R.same_clat(g, R.convert_lattice(L))
        assert int(g["n_states"]) < int(L["num_states"]) and max(len(x) for x in g["arc_string"]) > 1
        assert all(len(x) == 0 for x in g["final_string"])
    # the existing kinds are as they were: a Lattice table is no CompactLattice table
    with pytest.raises(Exception):
        list(cli.SequentialTableReader("ark:%s" % lpath, "compact_lattice"))


def test_random_access_and_the_function_itself(tmp_path):
    cli, kio = pkg("kaldi_cli"), pkg("kaldi_io")
    _, lpath, keys = tables(tmp_path, True)
    r = cli.RandomAccessTableReader("ark:%s" % lpath, "compact_lattice_converted")
    assert r.has_key(keys[2]) and not r.has_key("nope")
    L = dict(cli.SequentialTableReader("ark:%s" % lpath, "lattice"))[keys[2]]
    R.same_clat(r.value(keys[2]), kio.lattice_to_compact_lattice(L))
    buf = io.BytesIO()
    kio.write_lattice(buf, dict(L, state_frame=np.zeros(L["num_states"], np.int32)), True)
    R.same_clat(kio.read_compact_lattice_converted(io.BytesIO(buf.getvalue()), True), kio.lattice_to_compact_lattice(L))
    assert np.array_equal(kio.read_compact_lattice_converted(io.BytesIO(buf.getvalue()), True)["arc_src"],
                          kio.lattice_to_compact_lattice(L)["arc_src"])
