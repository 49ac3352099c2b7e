"""GPU checks of the cluster-lensing profiles (HaloModel.sigma_1h_profiles / kappa_1h_profiles / kappa_2h_profiles,
hmvec_amd.lensing; definitions in DESIGN.md section 10).

kappa_2h is checked against the unmodified reference (tests/golden/lensing_2h.npz).  The one-halo terms have no
reference fixture (the reference delegates them to clusterlensing, which is not available): they are pinned by
independent numerical integration with scipy - the line-of-sight integral of an NFW density written here, and nquad
over the Rayleigh-averaged definition.
"""
import os
import sys

import numpy as np
import pytest
from scipy import integrate

from conftest import load_golden

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
from lensing_model import model  # noqa: E402

pytestmark = pytest.mark.gpu

ARCMIN = np.pi / 180 / 60


def rho_nfw(r, rs, dc, rhoc):
    x = r / rs
    return dc * rhoc / (x * (1 + x) ** 2)


def sigma_los(R, rs, dc, rhoc, **kw):
    """2 int_0^inf rho_NFW(sqrt(R^2 + l^2)) dl, in three pieces for quad."""
    f = lambda l: rho_nfw(np.hypot(R, l), rs, dc, rhoc)   # noqa: E731
    opts = dict(limit=400, **kw)
    return 2 * sum(integrate.quad(f, a, b, **opts)[0] for a, b in ((0, R), (R, 30 * R), (30 * R, np.inf)))


def centred_shape(x):
    """Wright & Brainerd closed form, for the continuity check only (away from x = 1)."""
    x = np.asarray(x, float)
    lo = (1 - 2 / np.sqrt(1 - x * x) * np.arctanh(np.sqrt((1 - x) / (1 + x)))) / (x * x - 1)
    hi = (1 - 2 / np.sqrt(x * x - 1) * np.arctan(np.sqrt((x - 1) / (1 + x)))) / (x * x - 1)
    return np.where(x < 1, lo, hi)


# ---------------------------------------------------------------- 1. kappa_2h vs the reference
def test_kappa_2h_matches_reference():
    g = load_golden("lensing_2h")
    cases = sorted(k[:-len("zs")] for k in g if k.endswith("_zs"))
    assert len(cases) >= 8
    for p in cases:
        zsource, lmin, lmax = (float(v) for v in g[p + "scalars"])
        h = model(g[p + "zs"], g[p + "ks"], g[p + "ms"])
        assert np.max(np.abs(h.Pzk / g[p + "in_Pzk"] - 1)) < 1e-13
        got = h.kappa_2h_profiles(g[p + "thetas"], g[p + "Ms"], zsource, lmin=lmin, lmax=lmax, verbose=False)
        ref = g[p + "kappa_2h"]
        assert got.shape == ref.shape == (g[p + "thetas"].size, 1)
        tol = 1e-9 * np.abs(ref) + 1e-12 * np.max(np.abs(ref))
        assert np.all(np.abs(got - ref) <= tol), (p, float(np.max(np.abs(got - ref) / tol)))


def test_kappa_2h_verbose_prints_the_reference_lines(capsys):
    h = model([0.5])
    h.kappa_2h_profiles(np.array([1.0, 2.0]) * ARCMIN, [3e14], 1100.0)
    out = capsys.readouterr().out.splitlines()
    assert out[0].startswith("bias ") and out[-1].startswith("sigmacr ")


# ---------------------------------------------------------------- 2. centred Sigma vs the line-of-sight integral
def test_centred_sigma_vs_line_of_sight_integral():
    from hmvec_amd.lensing import sigma_nfw
    rng = np.random.default_rng(7)
    n = 200
    rs = rng.uniform(0.05, 0.8, n)
    dc = 10 ** rng.uniform(3, 5, n)
    rhoc = 10 ** rng.uniform(10.8, 11.8, n)
    x = np.geomspace(1e-4, 1e3, n)
    rng.shuffle(x)
    R = x * rs
    got = sigma_nfw(rs, dc, rhoc, R[:, None])[:, 0]
    ref = np.array([sigma_los(R[i], rs[i], dc[i], rhoc[i], epsabs=0, epsrel=1e-12) for i in range(n)])
    assert np.max(np.abs(got / ref - 1)) <= 1e-10


def test_centred_sigma_near_x_equal_one():
    from hmvec_amd.lensing import sigma_nfw
    rs, dc, rhoc = 0.3, 5e3, 1.3e11
    eps = np.array([-1e-4, -1e-8, -1e-12, 1e-12, 1e-8, 1e-4])
    x = 1 + eps
    got = sigma_nfw([rs], [dc], [rhoc], (x * rs)[None, :])[0]
    # (scipy refuses epsrel below 50 ulp with epsabs = 0: a vanishing epsabs asks for the same relative accuracy)
    ref = np.array([sigma_los(xi * rs, rs, dc, rhoc, epsabs=1e-300, epsrel=1e-14) for xi in x])
    assert np.max(np.abs(got / ref - 1)) <= 1e-12
    A = 2 * rs * dc * rhoc
    # continuous across x = 1: the series values meet A/3 and the closed form just outside the series' range
    assert np.all(np.abs(got / (A / 3) - 1) <= 1.5 * np.abs(eps) + 1e-15)       # slope of ln f at x = 1: -1.2
    xo = np.array([0.8, 0.81, 1.22, 1.23])
    out = sigma_nfw([rs], [dc], [rhoc], (xo * rs)[None, :])[0]
    assert np.max(np.abs(out / (A * centred_shape(xo)) - 1)) <= 1e-13
    xs = np.linspace(1 - 1e-3, 1 + 1e-3, 2001)
    s = sigma_nfw([rs], [dc], [rhoc], (xs * rs)[None, :])[0]
    assert np.all(np.diff(s) < 0)                  # monotone through the switch points


# ---------------------------------------------------------------- 3. miscentred Sigma vs nquad
def test_miscentred_sigma_vs_nquad():
    from hmvec_amd.lensing import sigma_nfw
    rng = np.random.default_rng(11)
    n = 30
    rs = rng.uniform(0.1, 0.6, n)
    dc = 10 ** rng.uniform(3, 5, n)
    rhoc = np.full(n, 1.3e11)
    so = rs * np.geomspace(0.05, 5, n)
    R = rs * np.exp(rng.uniform(np.log(0.01), np.log(30), n))
    got = sigma_nfw(rs, dc, rhoc, R[:, None], offsets=so)[:, 0]
    A = 2 * rs * dc * rhoc
    for i in range(n):
        s, r, Ri = so[i], rs[i], R[i]

        def f(phi, ro):
            rr = np.sqrt((Ri - ro) ** 2 + 4 * Ri * ro * np.sin(phi / 2) ** 2)
            return ro / s ** 2 * np.exp(-ro ** 2 / (2 * s ** 2)) * A[i] * centred_shape(rr / r) / np.pi

        top = 12 * s           # the Rayleigh weight beyond: exp(-72)
        outer = dict(limit=200, epsabs=0, epsrel=1e-9, **(dict(points=[Ri]) if Ri < top else {}))
        ref = integrate.nquad(f, [[0, np.pi], [0, top]], opts=[dict(limit=200, epsabs=0, epsrel=1e-9, points=[0.0]),
                                                               outer])[0]
        assert abs(got[i] / ref - 1) <= 1e-6, (i, s / r, Ri / r, got[i] / ref - 1)


def test_zero_offset_is_the_centred_route_bit_for_bit():
    h = model([0.4])
    th = np.geomspace(0.5, 30, 16) * ARCMIN
    Ms, cs = np.array([1e13, 3e14, 2e15]), np.array([7.0, 5.0, 3.5])
    a = h.sigma_1h_profiles(th, Ms, cs)
    b = h.sigma_1h_profiles(th, Ms, cs, sig_theta=0.0)
    assert a.shape == (3, 16)
    assert np.array_equal(a, b)
    from hmvec_amd.lensing import sigma_nfw
    rs = np.array([0.2, 0.3])
    mixed = sigma_nfw(rs, [1e4, 2e4], [1e11, 1e11], [0.1, 0.5], offsets=[0.0, 0.1])
    centred = sigma_nfw(rs, [1e4, 2e4], [1e11, 1e11], [0.1, 0.5])
    assert np.array_equal(mixed[0], centred[0]) and not np.array_equal(mixed[1], centred[1])


# ---------------------------------------------------------------- 4. several lens redshifts
def test_multi_z_batch_equals_single_z_models():
    zs = np.array([0.2, 0.45, 0.8, 1.3])
    th = np.geomspace(0.5, 30, 10) * ARCMIN
    Ms, cs = np.array([5e13, 3e14]), np.array([6.0, 4.0])
    hz = model(zs)
    S = hz.sigma_1h_profiles(th, Ms, cs)
    So = hz.sigma_1h_profiles(th, Ms, cs, sig_theta=0.5 * ARCMIN)
    K1 = hz.kappa_1h_profiles(th, Ms, cs, 1100.0)
    K2 = hz.kappa_2h_profiles(th, Ms, 1100.0, verbose=False)
    assert S.shape == So.shape == K1.shape == (4, 2, 10)
    assert K2.shape == (4, 10, 2)
    for i, z in enumerate(zs):
        h1 = model([z])
        assert np.array_equal(S[i], h1.sigma_1h_profiles(th, Ms, cs))
        assert np.array_equal(So[i], h1.sigma_1h_profiles(th, Ms, cs, sig_theta=0.5 * ARCMIN))
        assert np.array_equal(K1[i], h1.kappa_1h_profiles(th, Ms, cs, 1100.0))
        k2 = h1.kappa_2h_profiles(th, Ms, 1100.0, verbose=False)
        assert k2.shape == (10, 2)
        assert np.max(np.abs(K2[i] - k2)) <= 1e-14 * np.max(np.abs(k2))


def test_kappa_1h_is_sigma_over_sigma_crit():
    h = model([0.5])
    th = np.geomspace(1, 20, 5) * ARCMIN
    S = h.sigma_1h_profiles(th, [2e14], [5.0], rho="critical", delta=500)
    K = h.kappa_1h_profiles(th, [2e14], [5.0], 2.0, rho="critical", delta=500)
    assert np.allclose(K, S / h.sigma_crit(np.array([0.5]), 2.0), rtol=1e-15, atol=0)


# ---------------------------------------------------------------- 5. determinism
def test_miscentred_kernel_is_bit_identical_on_repeat():
    from hmvec_amd.lensing import sigma_nfw
    rng = np.random.default_rng(3)
    n = 500
    rs = rng.uniform(0.1, 0.5, n)
    args = (rs, 10 ** rng.uniform(3, 5, n), np.full(n, 1.2e11), np.geomspace(0.01, 5, 24))
    off = rs * rng.uniform(0.05, 3, n)
    a = sigma_nfw(*args, offsets=off)
    b = sigma_nfw(*args, offsets=off)
    assert np.all(np.isfinite(a)) and np.array_equal(a, b)


# ---------------------------------------------------------------- 6. validation
def test_lensing_methods_reject_bad_inputs():
    h = model([0.5])
    th = np.array([1.0, 2.0]) * ARCMIN
    for bad in (dict(thetas=np.array([0.0, 1e-3])), dict(Ms=[-1e14]), dict(concs=[0.0])):
        kw = dict(thetas=th, Ms=[1e14], concs=[5.0])
        kw.update(bad)
        with pytest.raises(ValueError):
            h.sigma_1h_profiles(**kw)
        with pytest.raises(ValueError):
            h.kappa_1h_profiles(zsource=2.0, **kw)
    with pytest.raises(ValueError):
        h.sigma_1h_profiles(th, [1e14, 2e14], [5.0])
    for Ms in ([1e9], [1e18], [0.0]):
        with pytest.raises(ValueError):
            h.kappa_2h_profiles(th, Ms, 2.0, verbose=False)
    with pytest.raises(ValueError):
        h.kappa_2h_profiles(-th, [1e14], 2.0, verbose=False)


# the six entry points (this file's and tests/test_gpu_delta_sigma.py's), by the argument list they share
@pytest.mark.parametrize("entry", ["hmg_lensing_sigma_nfw", "hmg_lensing_delta_sigma_nfw"])
def test_c_abi_rejects_null_pointers_and_empty_sizes(entry):
    from hmvec_amd import _native as nat
    ctx = nat.Context(0)
    d = ctx.empty((8,))
    p = d.ptr
    with pytest.raises(nat.NativeError, match="NULL"):
        ctx.call(entry, 2, 2, 0, p, p, None, p, p)
    with pytest.raises(nat.NativeError, match="empty"):
        ctx.call(entry, 0, 2, 0, p, p, p, p, p)
    ctx.close()


@pytest.mark.parametrize("entry", ["hmg_lensing_sigma_nfw_off", "hmg_lensing_delta_sigma_nfw_off"])
def test_c_abi_miscentred_rejects_null_pointers_and_empty_sizes(entry):
    from hmvec_amd import _native as nat
    ctx = nat.Context(0)
    d = ctx.empty((8,))
    p = d.ptr
    with pytest.raises(nat.NativeError, match="NULL"):
        ctx.call(entry, 2, 2, 0, p, p, p, p, None, p)
    with pytest.raises(nat.NativeError, match="empty"):
        ctx.call(entry, 2, 0, 1, p, p, p, p, p, p)
    ctx.close()


@pytest.mark.parametrize("entry", ["hmg_lensing_kappa_2h", "hmg_lensing_gamma_t_2h"])
def test_c_abi_two_halo_rejects_null_pointers_and_empty_sizes(entry):
    from hmvec_amd import _native as nat
    ctx = nat.Context(0)
    d = ctx.empty((8,))
    p = d.ptr
    k2 = [1, 2, 2, 2, 1, p, p, p, p, p, 100.0, 1e4, p, p, p, p]
    for i, bad in ((5, None), (15, None), (0, 0), (2, 0)):
        a = list(k2)
        a[i] = bad
        with pytest.raises(nat.NativeError):
            ctx.call(entry, *a)
    a = list(k2)
    a[3] = 1
    with pytest.raises(nat.NativeError, match="two masses"):
        ctx.call(entry, *a)
    ctx.close()
