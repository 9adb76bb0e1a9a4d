"""CPU: bench.py's legs.  A plain run does only what the headline needs; --full adds every other leg, and the --no-*
options drop single legs of a --full run."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402

LEGS = ("no_cpu_baseline", "no_strong", "no_secondary", "no_extra_legs", "no_end_to_end")


def test_a_plain_run_skips_every_other_leg():
    for argv in ([], ["--steps", "5", "--warmup", "2"], ["--no-secondary", "--dump-outputs", "d"]):
        args = bench.parse_args(argv)
        assert not args.full and all(getattr(args, leg) for leg in LEGS), argv


def test_full_runs_every_leg_unless_dropped():
    args = bench.parse_args(["--full"])
    assert args.full and not any(getattr(args, leg) for leg in LEGS)
    args = bench.parse_args(["--full", "--no-secondary", "--no-extra-legs"])
    assert args.no_secondary and args.no_extra_legs and not (args.no_cpu_baseline or args.no_strong or args.no_end_to_end)
