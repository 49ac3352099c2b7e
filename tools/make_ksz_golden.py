#!/usr/bin/env python3
"""Generate tests/golden/ksz.npz from the UNMODIFIED reference's hmvec/ksz.py.

Runs only where the reference checkout exists (never on the GPU box).  The reference is made importable exactly as
tools/make_golden.py does it (stand-in camb whose background is this repo's AnalyticBackground and whose
get_matter_power_interpolator serves tests/helpers/pk_table.py, the np.loadtxt redirect for tinker.py's data file),
plus what ksz.py needs of an environment without CLASS and with a current scipy:
  * interp2d: make_golden.py's bilinear shim, made callable (the kSZ C_ell calls iP(z, k) one point at a time);
  * kSZ's default engine is 'class' (no classy here): the module functions build kSZ with engine='camb';
  * Cosmology.get_growth_rate_f (NotImplementedError for CAMB in the reference) and the stand-in background's
    redshift_at_comoving_radial_distance come from this package (hmvec_amd.cosmology.heath_growth_rate_f, z_of_chi),
    so both sides see the same inputs;
  * the stale pksz.pars.ombh2 / .YHe / .TCMB of the C_ell functions: a kSZ passed as pksz_in gets a ``pars`` holding
    the model's ombh2, YHe and T_CMB (in K);
  * get_ksz_auto_squeezed(params=None) writes into the reference's default_params: they are restored after the call.
The internal P_q_perp and P_qr tables are read back from the debug files the reference writes with
save_debug_files=True (in a temporary directory; %.18e round-trips float64).

Usage:  python tools/make_ksz_golden.py [--out tests/golden]
"""
import argparse
import json
import os
import sys
import tempfile
import types
import warnings

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(REPO, "tools"))
sys.path.insert(0, REPO)

from make_golden import REF, install_loadtxt_redirect, install_standin_camb  # noqa: E402
from hmvec_amd.cosmology import heath_growth_rate_f, z_of_chi  # noqa: E402

MS = np.geomspace(1e7, 1e16, 200)
ZS = np.array([0.35, 0.6, 0.9])
VOL = 2.0                                   # Gpc^3
NGALS = np.array([2e-4, 1.5e-4, 1e-4])      # Mpc^-3, reachable on MS
GRID = dict(kL_max=0.1, num_kL_bins=30, kS_min=0.1, kS_max=10.0, num_kS_bins=101, num_mu_bins=24)
NK_AUTO, NMU_AUTO, KMAX_AUTO = 60, 32, 100.0
ELLS = np.array([300.0, 1000.0, 2500.0, 4000.0, 6000.0, 400000.0])   # the last: ell/30 above chi(z_max)
SIGZ = 0.02


def cls_total():
    """A smooth C_ell^tot [muK^2] with lmax = 6000: chi* k_S crosses lmax inside the k_S range (inf branch)."""
    ls = np.arange(6001.0)
    return 2.0e3 / (ls + 10.0) ** 2 + 1e-5 * np.exp((ls / 2500.0) ** 2)


def install_ksz_shims(rk):
    import scipy.interpolate as si
    from scipy.interpolate import RectBivariateSpline

    class interp2d:  # noqa: N801  (bilinear; FITPACK clamps points outside the table)
        def __init__(self, x, y, z, bounds_error=False):
            self._s = RectBivariateSpline(np.asarray(x), np.asarray(y), np.asarray(z).T, kx=1, ky=1, s=0)
            tx, ty, c = self._s.tck
            self.tck = (tx, ty, c, 1, 1)

        def __call__(self, x, y):
            return np.atleast_1d(self._s(x, y, grid=True)).ravel()

    si.interp2d = interp2d
    rk.interp2d = interp2d
    camb = sys.modules["camb"]
    real_bg = camb.get_background

    def get_background(p):
        bg = real_bg(p)
        bg.redshift_at_comoving_radial_distance = types.MethodType(z_of_chi, bg)
        return bg

    camb.get_background = get_background
    import hmvec.cosmology as rc
    rc.Cosmology.get_growth_rate_f = lambda self, zs: heath_growth_rate_f(self, zs)
    d = list(rk.kSZ.__init__.__defaults__)
    d[-1] = "camb"                                  # engine
    rk.kSZ.__init__.__defaults__ = tuple(d)


def attach_pars(k):
    k.pars = types.SimpleNamespace(ombh2=k.ombh2, YHe=k.YHe, TCMB=k.p["T_CMB"] / 1e6)
    return k


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
    import hmvec.ksz as rk  # the unmodified reference
    install_ksz_shims(rk)

    d = {}
    # (a) / (b): kSZ on three redshifts without and with photo-z
    for tag, sigz in (("a", None), ("b", SIGZ)):
        k = rk.kSZ(ZS, VOL * np.ones(3), NGALS, ms=MS, sigz=sigz, **GRID)
        p = tag + "_"
        Cls = cls_total()
        d[p + "Nvv"] = np.array([k.Nvv(i, Cls) for i in range(ZS.size)])
        d[p + "vrec"] = np.array([np.asarray(v) for v in k.vrec])
        d[p + "bgs"] = np.array(k.bgs, dtype=np.float64)
        d[p + "kstars"] = np.array(k.kstars)
        d[p + "chistars"] = np.array(k.chistars)
        d[p + "adotf"] = np.array([a[0] for a in k.adotf])
        d[p + "fs"] = np.array([f[0] for f in k.fs])
        d[p + "mu"], d[p + "kLs"], d[p + "kS"] = k.mu, k.kLs, k.kS
        # what Nvv's k_S integral consumed, unbiased (W is re-applied in the CPU restatement)
        d[p + "in_Pgg"] = k.get_power("g", "g")
        d[p + "in_Pge"] = k.get_power("g", "e")
        d[p + "in_Hphoto"] = np.asarray(k.Hphotozs)
        if sigz is None:
            edges = np.geomspace(0.1, 10.0, 6)
            d[p + "Pge_err"] = np.array([k.Pge_err(i, edges, cls_total()) for i in range(ZS.size)])
            d[p + "Pge_err_edges"] = edges
        snr, _ = rk.get_ksz_snr(VOL, ZS[1], NGALS[1], cls_total(), ms=MS, sigz=sigz, **GRID)
        d[p + "snr"] = np.array([snr]).ravel()
        print(f"case {tag}: Nvv {d[p + 'Nvv'].shape} snr {d[p + 'snr']}")

    # (c) / (d): C_ell^kSZ, Ma-Fry and squeezed, on a kSZ passed in (the reference's own skip_hod=True model cannot
    # be built: kSZ.__init__ asks for the 'g' spectra unconditionally)
    kmin = rk.get_kmin(VOL)
    pk = attach_pars(rk.kSZ(ZS, VOL * np.ones(3), NGALS, kL_max=KMAX_AUTO, num_kL_bins=NK_AUTO, kS_min=kmin,
                            kS_max=KMAX_AUTO, num_kS_bins=NK_AUTO, num_mu_bins=NMU_AUTO, ms=MS))
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        os.mkdir("debug_files")
        try:
            _, cl_mf = rk.get_ksz_auto_signal_mafry(ELLS, VOL, ZS, NGALS[0], None, pksz_in=pk, save_debug_files=True)
            d["c_pqperp"] = np.loadtxt("debug_files/pqperp.dat").reshape(NK_AUTO, ZS.size)
            d["c_Pee"] = np.loadtxt("debug_files/pee.dat")
            d["c_Pmm"] = np.loadtxt("debug_files/pmm.dat")
            saved = dict(rk.default_params)
            _, cl_sq, spec = rk.get_ksz_auto_squeezed(ELLS, VOL, ZS, NGALS, np.ones(3), pksz_in=pk,
                                                      save_debug_files=True)
            # (with params=None the reference writes hod_bisection_search_min_log10mthresh = 1 into its module's
            # default_params, which would change the HOD bisection of every later kSZ: put it back)
            rk.default_params.clear()
            rk.default_params.update(saved)
            d["d_pqr"] = np.loadtxt("debug_files/pqr.dat").reshape(NK_AUTO, ZS.size)
        finally:
            os.chdir(cwd)
    d["c_cl"], d["d_cl"] = cl_mf, cl_sq
    d["c_ks"], d["c_mus"], d["c_kLs"] = pk.kS, pk.mu, pk.kLs
    d["c_adotf"] = np.array([a[0] for a in pk.adotf])
    chi_max = pk.comoving_radial_distance(ZS[-1])
    chi_int = np.array([np.geomspace(e / 30.0, chi_max, 100) for e in ELLS])
    d["c_chi_nodes"] = chi_int
    d["c_z_nodes"] = np.asarray(pk.redshift_at_comoving_radial_distance(chi_int))
    d["c_ne0"] = np.array([rk.ne0_shaw(pk.ombh2, pk.YHe)])
    print(f"case c/d: cl_mafry {cl_mf} cl_squeezed {cl_sq}")

    # (e): the kSZ template cross-spectrum
    cl_t, fk, _ = rk.get_ksz_template_signal_snapshot(ELLS[:5], VOL, ZS[1], NGALS[1], 1.7, ms=MS, **GRID)
    d["e_cl"] = np.asarray(cl_t)
    print(f"case e: {cl_t}")

    d["zs"], d["ngals"], d["ms"], d["ells"], d["Cls"] = ZS, NGALS, MS, ELLS, cls_total()
    d["meta_json"] = np.array(json.dumps(dict(vol=VOL, sigz=SIGZ, grid=GRID, nk_auto=NK_AUTO, nmu_auto=NMU_AUTO,
                                              kmax_auto=KMAX_AUTO, accuracy="medium", bg_template=1.7)))
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, "ksz.npz")
    np.savez_compressed(path, **d)
    print(f"wrote {path}  ({os.path.getsize(path)/1024:.0f} KiB)")


if __name__ == "__main__":
    main()
