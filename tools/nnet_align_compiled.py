#!/usr/bin/env python3
"""nnet2bin/nnet-align-compiled.cc's command line over the library; see tools/align_compiled.py."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import align_compiled  # noqa: E402


def main(argv=None):
    return align_compiled.main(argv, kind="nnet2")


if __name__ == "__main__":
    sys.exit(main())
