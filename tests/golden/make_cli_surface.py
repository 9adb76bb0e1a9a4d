"""Record the command-line surface of every command in bin/: what each prints and returns before it reads a file.

Run it on a checkout of the commit whose surface is to be kept (the parent of a change to the tools' shared code):

    git worktree add ../parent <commit>
    python tests/golden/make_cli_surface.py --tree ../parent --parent <commit>

It writes tests/golden/cli_surface.json next to this script.  For every command in <tree>/bin it starts the shim itself and
stores stdout, stderr and the exit status of

    no_args     no arguments: the usage, status 1
    help        --help: the usage, status 0
    bad_option  --no-such-option=1 in front of a valid number of arguments: the usage with "Command line was", the
                "Invalid option" error, status 255
    no_job      (the tools that take --world / --rank) --world=2 --rank=1 with an output that lacks JOB: the tool's own
                message, status 255

All of them end in an orderly exit before a model is read or a device is touched.  tests/test_cli_surface.py replays them on
the tree under test and compares byte for byte.  Without --parent the commit named in the existing file is kept, so that a
run on a tree with the same surface reproduces the file exactly."""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "cli_surface.json")

# a valid number of positional arguments per command (they are never opened)
NARGS = {
    "acc-lda": 4, "ali-to-post": 2, "compose-transforms": 3, "gmm-acc-mllt": 4, "gmm-acc-stats": 4, "gmm-acc-stats-ali": 4,
    "gmm-acc-stats-twofeats": 5, "gmm-align-compiled": 4, "gmm-est-fmllr": 4, "gmm-est-fmllr-gpost": 4, "gmm-latgen-faster": 4,
    "gmm-post-to-gpost": 4, "gmm-rescore-lattice": 4, "gmm-sum-accs": 2, "lattice-add-penalty": 2, "lattice-align-words": 4,
    "lattice-best-path": 2, "lattice-depth": 1, "lattice-determinize-pruned": 2, "lattice-mbr-decode": 2, "lattice-oracle": 3,
    "lattice-prune": 2, "lattice-scale": 2, "lattice-to-ctm-conf": 2, "lattice-to-post": 2, "nnet-align-compiled": 4,
    "nnet-latgen-faster": 4, "online2-wav-nnet2-latgen-faster": 5, "sum-lda-accs": 2, "transform-feats": 3,
    "weight-silence-post": 5,
}
# the commands that shard by JOB: their arguments with an output that lacks it
NO_JOB = {
    "acc-lda": ["final.mdl", "ark:feats.JOB.ark", "ark:post.JOB.ark", "lda.acc"],
    "gmm-acc-mllt": ["final.mdl", "ark:feats.JOB.ark", "ark:post.JOB.ark", "1.macc"],
    "gmm-rescore-lattice": ["final.mdl", "ark:lat.tmp.JOB.ark", "ark:feats.JOB.ark", "ark:lat.ark"],
    "nnet-latgen-faster": ["final.mdl", "HCLG.fst", "ark:feats.JOB.ark", "ark:lat.ark"],
    "gmm-latgen-faster": ["final.mdl", "HCLG.fst", "ark:feats.JOB.ark", "ark:lat.ark"],
}
LAUNCHER_ENV = ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")


def cases(command):
    out = {"no_args": [], "help": ["--help"],
           "bad_option": ["--no-such-option=1"] + ["arg%d" % i for i in range(1, NARGS[command] + 1)]}
    if command in NO_JOB:
        out["no_job"] = ["--world=2", "--rank=1"] + NO_JOB[command]
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--tree", default=ROOT, help="the checkout whose bin/ is run (default: this one)")
    ap.add_argument("--parent", default=None, help="the commit the tree is a checkout of, stored in the file")
    args = ap.parse_args()
    parent = args.parent
    if parent is None:
        with open(OUT) as f:
            parent = json.load(f)["parent"]
    bindir = os.path.join(os.path.abspath(args.tree), "bin")
    commands = sorted(os.listdir(bindir))
    if set(commands) != set(NARGS):
        sys.exit("bin/ and NARGS differ: %s" % sorted(set(commands) ^ set(NARGS)))
    env = {k: v for k, v in os.environ.items() if k not in LAUNCHER_ENV}
    env["PYTHON"] = sys.executable
    surface = {}
    for command in commands:
        surface[command] = {}
        for name, argv in cases(command).items():
            r = subprocess.run([os.path.join(bindir, command)] + argv, env=env, stdin=subprocess.DEVNULL, capture_output=True, timeout=300)
            surface[command][name] = dict(argv=argv, status=r.returncode, stdout=r.stdout.decode(), stderr=r.stderr.decode())
            print("%-34s %-10s %3d" % (command, name, r.returncode))
    with open(OUT, "w") as f:
        json.dump(dict(parent=parent, commands=surface), f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
