"""GPU checks of the excess-surface-density and tangential-shear profiles (HaloModel.delta_sigma_1h_profiles,
gamma_t_1h_profiles, gamma_t_2h_profiles, delta_sigma_2h_profiles, sigma_2h_profiles; hmvec_amd.lensing.delta_sigma_nfw
and gamma_t_2h_integral; definitions in DESIGN.md section 12).

The reference has no Delta Sigma, so there is no reference fixture: the centred profile is pinned against 50-digit
mpmath of the Wright & Brainerd closed forms, the miscentred one against a host integration of the already validated
miscentred Sigma, the device J2 against mpmath, and the two-halo terms against a numpy restatement on the inputs stored
with tests/golden/lensing_2h.npz.
"""
import os
import sys

import mpmath as mp
import numpy as np
import pytest
from scipy.special import jv

from conftest import load_golden

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
from lensing_model import model  # noqa: E402

pytestmark = pytest.mark.gpu

ARCMIN = np.pi / 180 / 60
_trapz = getattr(np, "trapezoid", None) or np.trapz


def mp_delta_sigma_shape(x):
    """(Sigmabar(<x) - Sigma(x)) / A from the Wright & Brainerd (2000) closed forms, eqs. 11 and 13-15."""
    with mp.workdps(50):
        x = mp.mpf(float(x))
        if x == 1:
            return float(2 * (1 + mp.log(mp.mpf(1) / 2)) - mp.mpf(1) / 3)
        if x < 1:
            h = 2 / mp.sqrt(1 - x * x) * mp.atanh(mp.sqrt((1 - x) / (1 + x)))
        else:
            h = 2 / mp.sqrt(x * x - 1) * mp.atan(mp.sqrt((x - 1) / (1 + x)))
        return float(2 * (h + mp.log(x / 2)) / (x * x) - (1 - h) / (x * x - 1))


# ---------------------------------------------------------------- 1. centred Delta Sigma vs mpmath
def test_centred_delta_sigma_matches_mpmath():
    from hmvec_amd.lensing import delta_sigma_nfw
    x = np.concatenate([np.geomspace(1e-6, 1e4, 301), 1 + np.array([-1e-4, -1e-8, -1e-12, 1e-12, 1e-8, 1e-4]),
                        [1.0, 0.8181, 0.8182, 1.2222, 1.2223]])
    rng = np.random.default_rng(5)
    n = x.size
    rs = rng.uniform(0.05, 0.8, n)
    dc = 10 ** rng.uniform(3, 5, n)
    rhoc = 10 ** rng.uniform(10.8, 11.8, n)
    R = x * rs
    got = delta_sigma_nfw(rs, dc, rhoc, R[:, None])[:, 0]
    xd = R / rs                                         # the device's x
    ref = 2 * rs * dc * rhoc * np.array([mp_delta_sigma_shape(v) for v in xd])
    assert np.max(np.abs(got / ref - 1)) <= 1e-12


def test_centred_delta_sigma_shared_radii_and_shape():
    from hmvec_amd.lensing import delta_sigma_nfw, sigma_nfw
    rs, dc, rhoc = np.array([0.2, 0.4]), np.array([1e4, 3e4]), np.array([1.2e11, 1.3e11])
    R = np.geomspace(0.01, 5, 7)
    a = delta_sigma_nfw(rs, dc, rhoc, R)
    b = delta_sigma_nfw(rs, dc, rhoc, np.tile(R, (2, 1)))
    assert a.shape == (2, 7) and np.array_equal(a, b)
    assert np.all(a > 0) and not np.array_equal(a, sigma_nfw(rs, dc, rhoc, R))


# ---------------------------------------------------------------- 2. miscentred Delta Sigma vs a host integral of Sigma_off
def test_miscentred_delta_sigma_vs_integral_of_sigma_off():
    from hmvec_amd.lensing import delta_sigma_nfw, sigma_nfw
    so_rs = np.geomspace(0.05, 5, 6)
    nR = 12
    rs = np.array([0.1, 0.25, 0.4, 0.2, 0.5, 0.3])
    dc = np.array([2e4, 8e3, 5e3, 1.5e4, 3e3, 1e4])
    rhoc = np.full(6, 1.3e11)
    so = so_rs * rs
    R = so[:, None] * np.geomspace(0.05, 50, nR)[None, :]
    got = delta_sigma_nfw(rs, dc, rhoc, R, offsets=so)

    # (2 / R^2) int_0^R R' Sigma_off(R') dR': 48-point Gauss-Legendre on 9 segments of [0, R] split at
    # R * geomspace(1e-3, 1, 9); Sigma_off at the nodes and at R itself in one call (one row per (halo, R))
    u, w = np.polynomial.legendre.leggauss(48)
    br = np.concatenate([[0.0], np.geomspace(1e-3, 1, 9)])
    lo, hi = br[:-1, None], br[1:, None]
    t = (0.5 * (hi - lo) * (u + 1) + lo).ravel()                  # nodes and weights on [0, 1]
    wt = (0.5 * (hi - lo) * w).ravel()
    Rf = R.ravel()
    hidx = np.repeat(np.arange(6), nR)
    S = sigma_nfw(rs[hidx], dc[hidx], rhoc[hidx], np.concatenate([Rf[:, None] * t, Rf[:, None]], axis=1),
                  offsets=so[hidx])
    ref = (2 * np.sum(wt * t * S[:, :-1], axis=1) - S[:, -1]).reshape(6, nR)
    tol = 1e-6 * np.abs(ref) + 1e-9 * np.max(np.abs(ref), axis=1, keepdims=True)
    assert np.all(np.abs(got - ref) <= tol), float(np.max(np.abs(got - ref) / tol))


# ---------------------------------------------------------------- 3. miscentred limits, zero offsets, determinism
def test_miscentred_approaches_centred():
    from hmvec_amd.lensing import delta_sigma_nfw
    rs, dc, rhoc = 0.3, 1e4, 1.3e11
    R = rs * np.geomspace(0.1, 10, 9)
    cen = delta_sigma_nfw([rs], [dc], [rhoc], R)[0]
    errs = []
    for s in (1e-2, 1e-3, 1e-4):                       # sigma_off -> 0
        off = delta_sigma_nfw([rs], [dc], [rhoc], R, offsets=[s * rs])[0]
        errs.append(np.max(np.abs(off / cen - 1)))
    assert errs[0] > errs[1] > errs[2] and errs[2] <= 1e-5, errs
    so = 0.1 * rs                                       # R >> sigma_off
    R = so * np.array([5.0, 50.0, 500.0])
    off = delta_sigma_nfw([rs], [dc], [rhoc], R, offsets=[so])[0]
    rel = np.abs(off / delta_sigma_nfw([rs], [dc], [rhoc], R)[0] - 1)
    assert rel[0] > rel[1] > rel[2] and rel[1] <= 1e-3 and rel[2] <= 1e-4, rel


def test_zero_offsets_take_the_centred_route_bit_for_bit():
    from hmvec_amd.lensing import delta_sigma_nfw
    rs = np.array([0.2, 0.3])
    args = (rs, [1e4, 2e4], [1e11, 1e11], [0.1, 0.5])
    mixed = delta_sigma_nfw(*args, offsets=[0.0, 0.1])
    centred = delta_sigma_nfw(*args)
    assert np.array_equal(mixed[0], centred[0]) and not np.array_equal(mixed[1], centred[1])
    assert np.array_equal(delta_sigma_nfw(*args, offsets=[0.0, 0.0]), centred)
    h = model([0.4])
    th = np.geomspace(0.5, 30, 16) * ARCMIN
    Ms, cs = np.array([1e13, 3e14, 2e15]), np.array([7.0, 5.0, 3.5])
    a = h.delta_sigma_1h_profiles(th, Ms, cs)
    assert a.shape == (3, 16)
    assert np.array_equal(a, h.delta_sigma_1h_profiles(th, Ms, cs, sig_theta=0.0))


def test_miscentred_delta_sigma_is_bit_identical_on_repeat():
    from hmvec_amd.lensing import delta_sigma_nfw
    rng = np.random.default_rng(3)
    n = 500
    rs = rng.uniform(0.1, 0.5, n)
    args = (rs, 10 ** rng.uniform(3, 5, n), np.full(n, 1.2e11), np.geomspace(0.01, 5, 24))
    off = rs * rng.uniform(0.05, 3, n)
    a = delta_sigma_nfw(*args, offsets=off)
    b = delta_sigma_nfw(*args, offsets=off)
    assert np.all(np.isfinite(a)) and np.array_equal(a, b)


# ---------------------------------------------------------------- 4. the device J2
def test_device_j2_matches_mpmath():
    """Two k nodes, P = (1, 0), chi = 1, b = 1, pre = 1: out = (l1 - l0) l0 J2(l0 theta) / 4 pi = J2(theta) / 4 pi."""
    from hmvec_amd.lensing import gamma_t_2h_integral
    x = np.concatenate([np.geomspace(1e-3, 1e4, 1500), np.linspace(1.9, 2.1, 81), [2.0, np.nextafter(2.0, 0)]])
    out = gamma_t_2h_integral([1.0, 2.0], [1.0], [1.0], [[1.0, 0.0]], x, 0.5, 3.0, [1.0, 2.0], [[1.0, 1.0]],
                              [1.5])[0, :, 0]
    c = 0.25 / np.pi
    ref = np.array([float(mp.besselj(2, v)) for v in x])
    amp = np.minimum(1.0, np.sqrt(2 / (np.pi * x)))
    # a few ulp absolute; at large x the argument reduction x - 3pi/4 adds x's own rounding, amp * ulp(x)
    tol = c * 4 * (np.spacing(1.0) + amp * np.spacing(x)) + np.spacing(np.abs(c * ref))
    assert np.all(np.abs(out - c * ref) <= tol), float(np.max(np.abs(out - c * ref) / tol))
    small = x < 5                                      # the series keeps J2 ~ x^2/8 in relative terms
    assert np.max(np.abs(out[small] / (c * ref[small]) - 1)) <= 8e-15


# ---------------------------------------------------------------- 5. two-halo terms vs a numpy restatement
def two_halo_definition(g, p, order, with_sigmac):
    ks, ms = g[p + "ks"], g[p + "ms"]
    zsource, lmin, lmax = (float(v) for v in g[p + "scalars"])
    z, th, Ms = g[p + "zs"], g[p + "thetas"], g[p + "Ms"]
    out = np.empty((len(z), len(th), len(Ms)))
    for iz in range(len(z)):
        ells = ks * g[p + "in_chi"][iz]
        sel = (ells > lmin) & (ells < lmax)
        ell = ells[sel]
        pre = g[p + "in_rhomz"][iz] / (1 + z[iz]) ** 3 / g[p + "in_DA"][iz] ** 2
        if with_sigmac:
            pre = pre / g[p + "in_sigmac"][iz]
        b = np.interp(Ms, ms, g[p + "in_bh"][iz])
        for it, t in enumerate(th):
            I = _trapz(pre * g[p + "in_Pzk"][iz, sel] * jv(order, ell * t) * ell / 2 / np.pi, ell) if ell.size >= 2 \
                else 0.0
            out[iz, it] = b * I
    return out[0]


def test_two_halo_gamma_t_and_delta_sigma_match_restatement():
    g = load_golden("lensing_2h")
    cases = sorted(k[:-len("zs")] for k in g if k.endswith("_zs"))
    assert len(cases) >= 8
    for p in cases:
        zsource, lmin, lmax = (float(v) for v in g[p + "scalars"])
        h = model(g[p + "zs"], g[p + "ks"], g[p + "ms"])
        gt = h.gamma_t_2h_profiles(g[p + "thetas"], g[p + "Ms"], zsource, lmin=lmin, lmax=lmax, verbose=False)
        ds = h.delta_sigma_2h_profiles(g[p + "thetas"], g[p + "Ms"], lmin=lmin, lmax=lmax, verbose=False)
        for got, ref in ((gt, two_halo_definition(g, p, 2, True)), (ds, two_halo_definition(g, p, 2, False))):
            assert got.shape == ref.shape == (g[p + "thetas"].size, 1)
            tol = 1e-9 * np.abs(ref) + 1e-12 * np.max(np.abs(ref))
            assert np.all(np.abs(got - ref) <= tol), (p, float(np.max(np.abs(got - ref) / tol)))


def test_sigma_2h_is_sigma_crit_times_kappa_2h():
    h = model([0.5])
    th = np.geomspace(0.5, 30, 12) * ARCMIN
    Ms = np.array([1e13, 3e14])
    K = h.kappa_2h_profiles(th, Ms, 1.5, verbose=False)
    S = h.sigma_2h_profiles(th, Ms, verbose=False)
    G = h.gamma_t_2h_profiles(th, Ms, 1.5, verbose=False)
    D = h.delta_sigma_2h_profiles(th, Ms, verbose=False)
    sc = float(np.atleast_1d(h.sigma_crit(np.array([0.5]), 1.5))[0])
    assert S.shape == K.shape == G.shape == D.shape == (12, 2)
    assert np.allclose(S, sc * K, rtol=1e-14, atol=0)
    assert np.allclose(D, sc * G, rtol=1e-14, atol=0)


def test_two_halo_verbose_prints_bias(capsys):
    h = model([0.5])
    h.delta_sigma_2h_profiles(np.array([1.0, 2.0]) * ARCMIN, [3e14])
    out = capsys.readouterr().out.splitlines()
    assert out[0].startswith("bias ") and not any(l.startswith("sigmacr") for l in out)
    h.gamma_t_2h_profiles(np.array([1.0, 2.0]) * ARCMIN, [3e14], 1100.0)
    out = capsys.readouterr().out.splitlines()
    assert out[0].startswith("bias ") and out[-1].startswith("sigmacr ")


# ---------------------------------------------------------------- 6. batching
def test_multi_z_batch_equals_single_z_models():
    zs = np.array([0.2, 0.45, 0.8, 1.3])
    th = np.geomspace(0.5, 30, 10) * ARCMIN
    Ms, cs = np.array([5e13, 3e14]), np.array([6.0, 4.0])
    hz = model(zs)
    D = hz.delta_sigma_1h_profiles(th, Ms, cs)
    Do = hz.delta_sigma_1h_profiles(th, Ms, cs, sig_theta=0.5 * ARCMIN)
    G1 = hz.gamma_t_1h_profiles(th, Ms, cs, 1100.0)
    two = {name: getattr(hz, name)(th, Ms, *args, verbose=False) for name, args in
           (("gamma_t_2h_profiles", (1100.0,)), ("delta_sigma_2h_profiles", ()), ("sigma_2h_profiles", ()))}
    assert D.shape == Do.shape == G1.shape == (4, 2, 10)
    for i, z in enumerate(zs):
        h1 = model([z])
        assert np.array_equal(D[i], h1.delta_sigma_1h_profiles(th, Ms, cs))
        assert np.array_equal(Do[i], h1.delta_sigma_1h_profiles(th, Ms, cs, sig_theta=0.5 * ARCMIN))
        assert np.array_equal(G1[i], h1.gamma_t_1h_profiles(th, Ms, cs, 1100.0))
        for name, args in (("gamma_t_2h_profiles", (1100.0,)), ("delta_sigma_2h_profiles", ()),
                           ("sigma_2h_profiles", ())):
            one = getattr(h1, name)(th, Ms, *args, verbose=False)
            assert two[name].shape == (4, 10, 2) and one.shape == (10, 2)
            assert np.max(np.abs(two[name][i] - one)) <= 1e-14 * np.max(np.abs(one)), name


def test_gamma_t_1h_is_delta_sigma_over_sigma_crit():
    h = model([0.5])
    th = np.geomspace(1, 20, 5) * ARCMIN
    D = h.delta_sigma_1h_profiles(th, [2e14], [5.0], rho="critical", delta=500, sig_theta=0.3 * ARCMIN)
    G = h.gamma_t_1h_profiles(th, [2e14], [5.0], 2.0, rho="critical", delta=500, sig_theta=0.3 * ARCMIN)
    assert np.allclose(G, D / h.sigma_crit(np.array([0.5]), 2.0), rtol=1e-15, atol=0)


# ---------------------------------------------------------------- 7. validation (the C ABI's: tests/test_gpu_lensing.py)
def test_methods_reject_bad_inputs():
    h = model([0.5])
    th = np.array([1.0, 2.0]) * ARCMIN
    for bad in (dict(thetas=np.array([0.0, 1e-3])), dict(Ms=[-1e14]), dict(concs=[0.0]), dict(sig_theta=-1e-4),
                dict(Ms=[1e14, 2e14])):
        kw = dict(thetas=th, Ms=[1e14], concs=[5.0])
        kw.update(bad)
        with pytest.raises(ValueError):
            h.delta_sigma_1h_profiles(**kw)
        with pytest.raises(ValueError):
            h.gamma_t_1h_profiles(zsource=2.0, **kw)
    for Ms in ([1e9], [1e18], [0.0]):
        with pytest.raises(ValueError):
            h.gamma_t_2h_profiles(th, Ms, 2.0, verbose=False)
        with pytest.raises(ValueError):
            h.delta_sigma_2h_profiles(th, Ms, verbose=False)
        with pytest.raises(ValueError):
            h.sigma_2h_profiles(th, Ms, verbose=False)
    with pytest.raises(ValueError):
        h.gamma_t_2h_profiles(-th, [1e14], 2.0, verbose=False)
    from hmvec_amd.lensing import delta_sigma_nfw, gamma_t_2h_integral
    with pytest.raises(ValueError):
        delta_sigma_nfw([0.2, 0.3], [1e4, 1e4], [1e11, 1e11], np.ones((3, 4)))
    with pytest.raises(ValueError):
        delta_sigma_nfw([0.2, 0.3], [1e4, 1e4], [1e11], [0.1])
    with pytest.raises(ValueError):
        delta_sigma_nfw([0.2, 0.3], [1e4, 1e4], [1e11, 1e11], [0.1], offsets=[-0.1, 0.1])
    with pytest.raises(ValueError):
        gamma_t_2h_integral([1.0, 2.0], [1.0], [1.0], [[1.0, 0.0, 0.0]], [1e-3], 0.5, 3.0, [1.0, 2.0],
                            [[1.0, 1.0]], [1.5])
    with pytest.raises(ValueError):
        gamma_t_2h_integral([1.0, 2.0], [1.0], [1.0], [[1.0, 0.0]], [1e-3], 0.5, 3.0, [1.0, 2.0],
                            [[1.0, 1.0]], [3.0])

