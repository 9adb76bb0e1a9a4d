"""CPU: the command-line surface of tools/acc_tree_stats.py and tools/sum_tree_stats.py - no arguments, --help, an unknown
option, the argument counts - in process through each module's main(argv), as tests/test_cli_surface.py replays the commands
of bin/ (these two have no shim there yet; the JOB refusal is in tests/test_gpu_acc_tree_stats_tool.py).  Every case ends before a file is
opened or a device is touched.  The usage texts and option lists are the reference binaries' (bin/acc-tree-stats.cc:38-60,
bin/sum-tree-stats.cc:30-39) plus the [MI355X] options."""
import importlib

import pytest

ACC_USAGE = ("Accumulate statistics for phonetic-context tree building.\n"
             "Usage:  acc-tree-stats [options] model-in features-rspecifier alignments-rspecifier [tree-accs-out]\n"
             "e.g.: \n"
             " acc-tree-stats 1.mdl scp:train.scp ark:1.ali 1.tacc\n")
SUM_USAGE = ("Sum statistics for phonetic-context tree building.\n"
             "Usage:  sum-tree-stats [options] tree-accs-out tree-accs-in1 tree-accs-in2 ...\n"
             "e.g.: \n"
             " sum-tree-stats treeacc 1.treeacc 2.treeacc 3.treeacc\n")
ACC_OPTIONS = ["--batch-frames", "--binary", "--central-position", "--ci-phones", "--context-width", "--gpu", "--phone-map", "--rank",
               "--var-floor", "--world"]
REFERENCE_DEFAULTS = ["Write output in binary mode (bool, default = true)", "Variance floor for tree clustering. (float, default = 0.01)",
                      "Context window size. (int, default = 3)", "Central context-window position (zero-based) (int, default = 1)",
                      'File name containing old->new phone mapping (each line is: old-integer-id new-integer-id) (string, default = "")',
                      "Colon-separated list of integer indices of context-independent phones (after mapping, if --phone-map option is "
                      'used). (string, default = "")']
LAUNCHER_ENV = ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")


def run(module, argv, capfd, monkeypatch):
    for k in LAUNCHER_ENV:
        monkeypatch.delenv(k, raising=False)
    main = importlib.import_module("tools." + module).main
    capfd.readouterr()
    try:
        status = main(list(argv))
    except SystemExit as e:                 # ParseOptions.read leaves through sys.exit(0) on --help
        status = e.code
    got = capfd.readouterr()
    return status, got.out, got.err


def options_of(err):
    """The names of the "Options:" block of a printed usage, in the order printed."""
    block = err.split("\nOptions:\n", 1)[1].split("\nStandard options:\n", 1)[0]
    return [line.split()[0] for line in block.splitlines() if line.startswith("  --")]


@pytest.mark.parametrize("module,prog,usage,options,n_args", [("acc_tree_stats", "acc-tree-stats", ACC_USAGE, ACC_OPTIONS, 4),
                                                              ("sum_tree_stats", "sum-tree-stats", SUM_USAGE, ["--binary"], 2)])
def test_usage_help_and_unknown_option(module, prog, usage, options, n_args, capfd, monkeypatch):
    status, out, err = run(module, [], capfd, monkeypatch)
    assert status == 1 and out == "" and err.startswith(prog + " \n\n" + usage + "\nOptions:\n") and options_of(err) == options
    assert "Command line was" not in err
    status, out, help_err = run(module, ["--help"], capfd, monkeypatch)
    assert status == 0 and out == "" and help_err == err[len(prog + " \n"):]         # the same usage, before the arguments are echoed
    args = ["arg%d" % i for i in range(1, n_args + 1)]
    status, out, bad = run(module, ["--no-such-option=1"] + args, capfd, monkeypatch)
    assert status == 255 and out == ""
    assert bad == help_err + "Command line was: %s --no-such-option=1 %s \nERROR (%s) Invalid option --no-such-option=1\n" % (prog, " ".join(args), prog)
    if module == "acc_tree_stats":
        for text in REFERENCE_DEFAULTS:
            assert text in err, text


def test_argument_counts(capfd, monkeypatch):
    for argv in (["a", "b"], ["a", "b", "c", "d", "e"]):                       # three or four arguments
        status, out, err = run("acc_tree_stats", argv, capfd, monkeypatch)
        assert status == 1 and ACC_USAGE in err
    status, out, err = run("sum_tree_stats", ["out"], capfd, monkeypatch)       # at least two
    assert status == 1 and SUM_USAGE in err
