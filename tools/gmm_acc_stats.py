#!/usr/bin/env python3
"""gmmbin/gmm-acc-stats.cc's command line over the library; see tools/gmm_acc_tools.py."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gmm_acc_tools  # noqa: E402


def main(argv=None):
    return gmm_acc_tools.main(argv, prog="gmm-acc-stats")


if __name__ == "__main__":
    sys.exit(main())
