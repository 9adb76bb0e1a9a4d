"""CPU: the command-line surface of every command in bin/ - usage, --help, an unknown option and, for the tools that shard by
JOB, an output without JOB - byte for byte what tests/golden/cli_surface.json recorded from the commit it names
(tests/golden/make_cli_surface.py started the shims there).  Replayed in-process through each module's main(argv): every
case ends before a file is opened or a device is touched."""
import importlib
import json
import os
import re

import pytest

from conftest import GOLDEN, ROOT

with open(os.path.join(GOLDEN, "cli_surface.json")) as _f:
    SURFACE = json.load(_f)
CASES = [(command, name) for command, cases in sorted(SURFACE["commands"].items()) for name in sorted(cases)]


def test_every_command_of_bin_is_recorded():
    assert sorted(SURFACE["commands"]) == sorted(os.listdir(os.path.join(ROOT, "bin")))
    assert re.fullmatch(r"[0-9a-f]{40}", SURFACE["parent"])
    for command, cases in SURFACE["commands"].items():
        assert {"no_args", "help", "bad_option"} <= set(cases), command
        assert (cases["no_args"]["status"], cases["help"]["status"], cases["bad_option"]["status"]) == (1, 0, 255), command
    assert sorted(c for c, cases in SURFACE["commands"].items() if "no_job" in cases) == [
        "acc-lda", "gmm-acc-mllt", "gmm-latgen-faster", "gmm-rescore-lattice", "nnet-latgen-faster"]


def _module_of(command):
    """The module the shim runs: `exec python "$here/../tools/<module>.py" "$@"`."""
    with open(os.path.join(ROOT, "bin", command)) as f:
        (name,) = set(re.findall(r"/tools/(\w+)\.py", f.read()))
    return importlib.import_module("tools." + name)


@pytest.mark.parametrize("command,name", CASES, ids=["%s-%s" % c for c in CASES])
def test_surface(command, name, capfd, monkeypatch):
    want = SURFACE["commands"][command][name]
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        monkeypatch.delenv(k, raising=False)
    main = _module_of(command).main
    capfd.readouterr()
    try:
        status = main(list(want["argv"]))
    except SystemExit as e:                 # ParseOptions.read leaves through sys.exit(0) on --help
        status = e.code
    got = capfd.readouterr()
    assert (status, got.out, got.err) == (want["status"], want["stdout"], want["stderr"])
