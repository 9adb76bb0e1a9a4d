#!/usr/bin/env python3
"""gmm-global-sum-accs: gmmbin/gmm-global-sum-accs.cc's command line, host only (no device is touched), so that

  gmm-global-est ... "gmm-global-sum-accs - $dir/$x.*.acc|" ...

of steps/online/nnet2/train_diag_ubm.sh reads this project's statistics files.  (There is no bin/ shim for it yet:
tests/test_cli_surface.py pins bin/ to the recorded tests/golden/cli_surface.json.)  The files' floats are added into doubles in
argument order, as AccumDiagGmm::Read(..., add = true) does (gmm/mle-diag-gmm.cc:33-75), files of another size, dimension or
flags are the binary's "dimension or flags mismatch" error, and the sum is written as floats; "-" is standard output.
--world / --rank: rank r is the recipe's JOB r + 1 and every JOB in the arguments becomes r + 1; the output must then carry
JOB in its name."""
import importlib
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
kt = importlib.import_module("old-kaldi-git_amd.kaldi_tool")

PROG = "gmm-global-sum-accs"
USAGE = ("Sum multiple accumulated stats files for diagonal-covariance GMM training.\n"
         "Usage: gmm-global-sum-accs [options] stats-out stats-in1 stats-in2 ...\n")


def main(argv=None):
    return kt.run_tool(PROG, run, argv, kt.KALDI)


def run(cli, argv):
    def register(po):
        po.register("binary", True, "Write output in binary mode")
        kt.register_gpu(po, "[MI355X] accepted for uniformity with the other tools; this one does not use a device")
        kt.register_ranks(po)
    argv, rank, world, raw_pos = kt.rank_substitute(argv)
    po = kt.parse(cli, PROG, USAGE, argv, register, lambda n: n >= 2)
    if po is None:
        return 1
    if world > 1 and "JOB" not in raw_pos[0]:
        raise cli.KaldiError("--world=%d: the output needs JOB in its name, or the ranks overwrite each other" % world)
    kio = importlib.import_module("old-kaldi-git_amd.kaldi_io")
    import numpy as np
    acc = dict(occ=np.zeros(0), mean_acc=None, var_acc=None, dim=0, flags=0)
    for i in range(2, po.num_args() + 1):
        acc = cli.read_kaldi_object(po.get_arg(i), lambda s, b: kio.read_global_gmm_accs(s, b, add_into=acc))
    cli.write_kaldi_object(po.get_arg(1), po["binary"], lambda f: kio.write_global_gmm_accs(f, acc, po["binary"]))
    cli.log("Written stats to " + po.get_arg(1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
