#!/usr/bin/env python3
"""Generate tests/golden/lensing_2h.npz from the UNMODIFIED reference's HaloModel.kappa_2h_profiles
(hmvec/hmvec.py:598-625).

Runs only where the reference checkout exists (never on the GPU box).  The reference is made importable exactly as
tools/make_golden.py does it (stand-in camb whose background is this repo's AnalyticBackground, the np.loadtxt
redirect for tinker.py's data file); with accuracy='low' P(k) comes from the reference's own Eisenstein-Hu code.

The reference's kappa_2h_profiles only runs for one lens redshift and one mass, so every case
here is a model with nz = 1 evaluated at nM = 1.  Each case stores its inputs (grids, lens and source redshift,
theta, mass, ell cut) next to what the reference computed from them, under the prefix ``c<i>_``.

Usage:  python tools/make_lensing_golden.py [--out tests/golden]
"""
import argparse
import json
import os
import sys
import warnings

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(REPO, "tools"))
sys.path.insert(0, REPO)

from make_golden import REF, install_loadtxt_redirect, install_standin_camb  # noqa: E402

ARCMIN = np.pi / 180.0 / 60.0


def cases():
    ks = np.geomspace(1e-4, 100, 200)
    ms = np.geomspace(2e10, 1e17, 40)
    thetas = np.geomspace(0.5, 30.0, 12) * ARCMIN
    # a k grid that is not log-uniform: a coarse log grid with a dense linear stretch spliced in
    ks_odd = np.unique(np.concatenate([np.geomspace(1e-4, 100, 120), np.linspace(0.05, 2.0, 90)]))
    out = []
    for z in (0.3, 0.6, 1.2):
        for zsource in (1100.0, 2.5):
            out.append(dict(z=z, zsource=zsource, ks=ks, ms=ms, thetas=thetas, M=3e14, lmin=100.0, lmax=10000.0))
    out.append(dict(z=0.6, zsource=1100.0, ks=ks, ms=ms, thetas=thetas, M=1e13, lmin=400.0, lmax=3000.0))
    out.append(dict(z=0.45, zsource=2.5, ks=ks_odd, ms=ms, thetas=thetas, M=2e15, lmin=100.0, lmax=10000.0))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden"))
    args = ap.parse_args()
    if not os.path.isdir(REF):
        sys.exit("reference checkout not present; goldens can only be generated in the build container")
    warnings.filterwarnings("ignore")
    install_standin_camb()
    install_loadtxt_redirect()
    sys.path.insert(0, REF)
    import hmvec as hm  # the unmodified reference

    d = {}
    for i, c in enumerate(cases()):
        zs = np.array([c["z"]])
        h = hm.HaloModel(zs, c["ks"], ms=c["ms"], accuracy="low")
        k2h = h.kappa_2h_profiles(c["thetas"], np.array([c["M"]]), zsource=c["zsource"], lmin=c["lmin"],
                                  lmax=c["lmax"], verbose=False)
        p = f"c{i}_"
        d[p + "zs"], d[p + "ks"], d[p + "ms"], d[p + "thetas"] = zs, c["ks"], c["ms"], c["thetas"]
        d[p + "Ms"] = np.array([c["M"]])
        d[p + "scalars"] = np.array([c["zsource"], c["lmin"], c["lmax"]])     # zsource, lmin, lmax
        # what the reference's expression consumed (hmvec/hmvec.py:600-611), for the CPU restatement of the definition
        d[p + "in_Pzk"] = h.Pzk
        d[p + "in_bh"] = h.bh
        d[p + "in_sigmac"] = np.atleast_1d(h.sigma_crit(zs, c["zsource"]))
        d[p + "in_rhomz"] = np.atleast_1d(h.rho_matter_z(zs))
        d[p + "in_chi"] = np.atleast_1d(h.comoving_radial_distance(zs))
        d[p + "in_DA"] = np.atleast_1d(h.angular_diameter_distance(zs))
        d[p + "kappa_2h"] = np.asarray(k2h)
        print(f"case {i}: z={c['z']} zsource={c['zsource']} nk={c['ks'].size} ell cut=({c['lmin']}, {c['lmax']}) "
              f"-> shape {k2h.shape}")
    d["meta_json"] = np.array(json.dumps(dict(ncases=len(cases()), accuracy="low")))
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, "lensing_2h.npz")
    np.savez_compressed(path, **d)
    print(f"wrote {path}  ({os.path.getsize(path)/1024:.0f} KiB)")


if __name__ == "__main__":
    main()
