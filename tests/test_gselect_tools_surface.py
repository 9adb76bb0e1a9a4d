"""CPU: the command-line surface of tools/gmm_gselect.py, tools/gmm_global_acc_stats.py and tools/gmm_global_sum_accs.py -
no arguments, --help, an unknown option, the argument counts - in process through each module's main(argv), as
tests/test_tree_tools_surface.py does for the tree tools (these three have no shim under bin/ yet; the JOB refusal is in
tests/test_gpu_gselect_tools.py).  Every case ends before a file is opened or a device is touched.  The usage texts, the option
texts and the defaults are the reference binaries' (gmmbin/gmm-gselect.cc:32-52, gmm-global-acc-stats.cc:33-49,
gmm-global-sum-accs.cc:28-35) plus the [MI355X] options."""
import importlib

import pytest

GSELECT_USAGE = ("Precompute Gaussian indices for pruning\n"
                 " (e.g. in training UBMs, SGMMs, tied-mixture systems)\n"
                 " For each frame, gives a list of the n best Gaussian indices,\n"
                 " sorted from best to worst.\n"
                 "See also: gmm-global-get-post, fgmm-global-gselect-to-post,\n"
                 "copy-gselect, fgmm-gselect\n"
                 "Usage: gmm-gselect [options] <model-in> <feature-rspecifier> <gselect-wspecifier>\n"
                 "The --gselect option (which takes an rspecifier) limits selection to a subset\n"
                 "of indices:\n"
                 "e.g.: gmm-gselect \"--gselect=ark:gunzip -c bigger.gselect.gz|\" --n=20 1.gmm \"ark:feature-command |\" "
                 "\"ark,t:|gzip -c >gselect.1.gz\"\n")
ACC_USAGE = ("Accumulate stats for training a diagonal-covariance GMM.\n"
             "Usage:  gmm-global-acc-stats [options] <model-in> <feature-rspecifier> <stats-out>\n"
             "e.g.: gmm-global-acc-stats 1.mdl scp:train.scp 1.acc\n")
SUM_USAGE = ("Sum multiple accumulated stats files for diagonal-covariance GMM training.\n"
             "Usage: gmm-global-sum-accs [options] stats-out stats-in1 stats-in2 ...\n")
TOOLS = {
    "gmm_gselect": ("gmm-gselect", GSELECT_USAGE, ["--batch-frames", "--gpu", "--gselect", "--n", "--rank", "--world", "--write-likes"], 3,
                    ["Number of Gaussians to keep per frame\n (int, default = 50)",
                     'rspecifier for likelihoods per utterance (string, default = "")',
                     'rspecifier for gselect objects to limit the search to (string, default = "")']),
    "gmm_global_acc_stats": ("gmm-global-acc-stats", ACC_USAGE,
                             ["--batch-frames", "--binary", "--gpu", "--gselect", "--rank", "--update-flags", "--weights", "--world"], 3,
                             ["Write output in binary mode (bool, default = true)",
                              'Which GMM parameters will be updated: subset of mvw. (string, default = "mvw")',
                              'rspecifier for gselect objects to limit the #Gaussians accessed on each frame. (string, default = "")',
                              "rspecifier for a vector of floats for each utterance, that's a per-frame weight. (string, default = \"\")"]),
    "gmm_global_sum_accs": ("gmm-global-sum-accs", SUM_USAGE, ["--binary", "--gpu", "--rank", "--world"], 2,
                            ["Write output in binary mode (bool, default = true)"]),
}
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


@pytest.mark.parametrize("module", sorted(TOOLS))
def test_usage_help_and_unknown_option(module, capfd, monkeypatch):
    prog, usage, options, n_args, texts = TOOLS[module]
    status, out, err = run(module, [], capfd, monkeypatch)
    assert status == 1 and out == "" and err.startswith(prog + " \n\n" + usage + "\nOptions:\n") and options_of(err) == options
    assert "Command line was" not in err
    status, out, help_err = run(module, ["--help"], capfd, monkeypatch)
    assert status == 0 and out == "" and help_err == err[len(prog + " \n"):]         # the same usage, before the arguments are echoed
    args = ["arg%d" % i for i in range(1, n_args + 1)]
    status, out, bad = run(module, ["--no-such-option=1"] + args, capfd, monkeypatch)
    assert status == 255 and out == ""
    assert bad == help_err + "Command line was: %s --no-such-option=1 %s \nERROR (%s) Invalid option --no-such-option=1\n" % (prog, " ".join(args), prog)
    for text in texts:
        assert text in err, text


def test_argument_counts(capfd, monkeypatch):
    for module, usage in (("gmm_gselect", GSELECT_USAGE), ("gmm_global_acc_stats", ACC_USAGE)):
        for argv in (["a", "b"], ["a", "b", "c", "d"]):                           # exactly three
            status, out, err = run(module, argv, capfd, monkeypatch)
            assert status == 1 and usage in err
    status, out, err = run("gmm_global_sum_accs", ["out"], capfd, monkeypatch)      # at least two
    assert status == 1 and SUM_USAGE in err
