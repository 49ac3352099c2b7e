#!/usr/bin/env python3
"""Generate tests/golden/cib_pins.npz from the UNMODIFIED reference's hmvec/tinker.py: NlnMsub, the subhalo mass function
the CIB model integrates, on 12 subhalo and 9 host masses, ratios above 1 included.  Data only.

Runs only where the reference checkout exists.  The module is loaded from its file, so nothing else of the reference is
imported.

Usage:  python tools/make_cib_pins.py"""
import importlib.util
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
from make_golden import REF  # noqa: E402


def main():
    path = os.path.join(REF, "hmvec", "tinker.py")
    if not os.path.isfile(path):
        sys.exit("the reference checkout is absent")
    spec = importlib.util.spec_from_file_location("reference_tinker", path)
    rt = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rt)
    Msubs, Mhosts = np.geomspace(1e10, 1e15, 12), np.geomspace(1e11, 1e16, 9)
    out = os.path.join(REPO, "tests", "golden", "cib_pins.npz")
    np.savez(out, Msubs=Msubs, Mhosts=Mhosts, NlnMsub=rt.NlnMsub(Msubs, Mhosts))
    print("wrote", out)


if __name__ == "__main__":
    main()
