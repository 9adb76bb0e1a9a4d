#!/usr/bin/env python3
"""featbin/compose-transforms.cc's command line over the library; see tools/fmllr_tools.py."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fmllr_tools  # noqa: E402


def main(argv=None):
    return fmllr_tools.main(argv, prog="compose-transforms")


if __name__ == "__main__":
    sys.exit(main())
