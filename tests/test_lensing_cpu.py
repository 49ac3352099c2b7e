"""CPU checks of the cluster-lensing definitions, no GPU needed.

The two-halo convergence is restated here in numpy, per lens redshift, from the inputs stored with
tests/golden/lensing_2h.npz (tools/make_lensing_golden.py), and must reproduce what the unmodified reference's
kappa_2h_profiles computed from them: this pins the written definition to the reference independently of the kernels.
"""
import numpy as np
import pytest
from scipy.special import j0

from conftest import load_golden

_trapz = getattr(np, "trapezoid", None) or np.trapz


def kappa_2h_definition(ks, ms, Pzk, bh, chi, DA, rhomz, sigmac, z, thetas, Ms, lmin, lmax):
    """DESIGN.md section 10, kappa_2h: (nz, ntheta, nM)."""
    out = np.empty((len(z), len(thetas), len(Ms)))
    for iz in range(len(z)):
        ells = ks * chi[iz]
        sel = (ells > lmin) & (ells < lmax)
        ell = ells[sel]
        pre = rhomz[iz] / (1 + z[iz]) ** 3 / sigmac[iz] / DA[iz] ** 2
        b = np.interp(Ms, ms, bh[iz])
        for it, th in enumerate(thetas):
            I = _trapz(pre * Pzk[iz, sel] * j0(ell * th) * ell / 2 / np.pi, ell) if ell.size >= 2 else 0.0
            out[iz, it] = b * I
    return out


def _cases(g):
    return [k[:-len("zs")] for k in g if k.endswith("_zs")]


def test_kappa_2h_definition_reproduces_reference():
    g = load_golden("lensing_2h")
    cases = _cases(g)
    assert len(cases) == g["meta"]["ncases"] >= 8
    for p in cases:
        zsource, lmin, lmax = g[p + "scalars"]
        mine = kappa_2h_definition(g[p + "ks"], g[p + "ms"], g[p + "in_Pzk"], g[p + "in_bh"], g[p + "in_chi"],
                                   g[p + "in_DA"], g[p + "in_rhomz"], g[p + "in_sigmac"], g[p + "zs"],
                                   g[p + "thetas"], g[p + "Ms"], lmin, lmax)[0]
        ref = g[p + "kappa_2h"]
        assert ref.shape == (g[p + "thetas"].size, 1)
        scale = np.max(np.abs(ref))
        assert np.all(np.abs(mine - ref) <= 1e-12 * np.abs(ref) + 1e-14 * scale), p


def test_golden_covers_the_issue_cases():
    g = load_golden("lensing_2h")
    cases = _cases(g)
    zl = {float(g[p + "zs"][0]) for p in cases}
    zsrc = {float(g[p + "scalars"][0]) for p in cases}
    cuts = {tuple(g[p + "scalars"][1:]) for p in cases}
    assert len(zl) >= 3 and len(zsrc) >= 2 and len(cuts) >= 2
    arcmin = np.pi / 180 / 60
    th = g[cases[0] + "thetas"]
    assert np.isclose(th[0], 0.5 * arcmin) and np.isclose(th[-1], 30 * arcmin)
    uniform = [np.allclose(np.diff(np.log(g[p + "ks"])), np.diff(np.log(g[p + "ks"]))[0]) for p in cases]
    assert not all(uniform)


@pytest.mark.parametrize("kw", [
    dict(rs=[0.0], delta_c=[1e4], rho_crit=[1e11], rbins=[0.1]),
    dict(rs=[0.2], delta_c=[-1.0], rho_crit=[1e11], rbins=[0.1]),
    dict(rs=[0.2], delta_c=[1e4], rho_crit=[1e11], rbins=[0.0, 0.1]),
    dict(rs=[0.2, 0.3], delta_c=[1e4], rho_crit=[1e11, 1e11], rbins=[0.1]),
    dict(rs=[0.2], delta_c=[1e4], rho_crit=[1e11], rbins=[0.1], offsets=[-0.1]),
    dict(rs=[0.2, 0.3], delta_c=[1e4, 1e4], rho_crit=[1e11, 1e11], rbins=np.ones((3, 2))),
])
def test_sigma_nfw_rejects_bad_inputs_before_any_launch(kw):
    from hmvec_amd.lensing import sigma_nfw
    with pytest.raises(ValueError):
        sigma_nfw(**kw)


def test_kappa_2h_integral_rejects_bad_inputs_before_any_launch():
    from hmvec_amd.lensing import kappa_2h_integral
    ks, ms = np.geomspace(1e-3, 10, 20), np.geomspace(1e12, 1e15, 5)
    base = dict(ks=ks, chi=[1000.0], pre=[1.0], Pzk=np.ones((1, 20)), thetas=[1e-3], lmin=100, lmax=1e4, ms=ms,
                bh=np.ones((1, 5)), Ms=[1e13])
    for bad in (dict(Ms=[1e16]), dict(Ms=[1e11]), dict(thetas=[0.0]), dict(ks=ks[::-1]), dict(Pzk=np.ones((2, 20))),
                dict(bh=np.ones((1, 4)))):
        with pytest.raises(ValueError):
            kappa_2h_integral(**{**base, **bad})


def test_abi_declares_the_lensing_entry_points():
    from hmvec_amd import _native as nat
    assert nat.ABI_VERSION == 10
    for name in ("hmg_lensing_sigma_nfw", "hmg_lensing_sigma_nfw_off", "hmg_lensing_kappa_2h"):
        assert name in nat.SIGNATURES
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hmgrid.h")).read()
    assert "#define HMG_ABI_VERSION 10" in hdr
    for name in ("hmg_lensing_sigma_nfw(", "hmg_lensing_sigma_nfw_off(", "hmg_lensing_kappa_2h("):
        assert name in hdr
