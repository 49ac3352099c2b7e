"""kSZ forecasts without a GPU: the definitions of the three kSZ kernels restated in numpy and
checked against the unmodified reference's values in tests/golden/ksz.npz (tools/make_ksz_golden.py), the host
helpers of hmvec_amd.ksz, and the two background methods kSZ needs (Cosmology.get_growth_rate_f and
redshift_at_comoving_radial_distance)."""
import os

import numpy as np
import pytest
from scipy.integrate import solve_ivp
from scipy.interpolate import interp1d

from conftest import load_golden

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_trapz = getattr(np, "trapezoid", None) or np.trapz


@pytest.fixture(scope="module")
def g():
    return load_golden("ksz")


# ------------------------------------------------------------------------------------------ the kernels' definitions
def pqperp_def(ks, mus, Pee, Pmm, adotf):
    """out[k, z] = adotf^2 (2 pi)^-2 trapz_mu trapz_k' nan_to_num(k'^2 k (k-2k'mu)(1-mu^2) / (k'^2 (k'^2+k^2-2kk'mu))
    Pmm(k') Pee(|k-k'|)), Pee linear on ks with 0 outside; also the same with |integrand| (the cancellation scale)."""
    mu, kp = np.meshgrid(mus, ks)
    out = np.zeros((ks.size, len(adotf)))
    absout = np.zeros_like(out)
    for iz in range(len(adotf)):
        pee = interp1d(ks, Pee[iz], bounds_error=False, fill_value=0.)
        for ik, k in enumerate(ks):
            with np.errstate(invalid="ignore", divide="ignore"):
                d2 = kp ** 2 + k ** 2 - 2 * k * kp * mu
                igr = kp ** 2 * (k * (k - 2 * kp * mu) * (1 - mu ** 2)) / (kp ** 2 * d2)
                igr = np.nan_to_num(igr * Pmm[iz][:, None] * pee(np.sqrt(d2)))
            pre = adotf[iz] ** 2 * (2 * np.pi) ** -2
            out[ik, iz] = pre * _trapz(_trapz(igr, ks, axis=0), mus)
            absout[ik, iz] = abs(pre) * _trapz(_trapz(np.abs(igr), ks, axis=0), mus)
    return out, absout


def cls_at(Cls, ell):
    ell = np.asarray(ell)
    inside = ell <= Cls.size - 1
    idx = np.where(inside, ell, 0).astype(int)
    c = np.where(idx < 2, 0.0, Cls[idx])
    return np.where(inside, c, np.inf)


def nvv_def(chi, F, mus, kLs, kSs, Cls, Pge, Pgg, ngg, sig=None, H=None):
    """Nvv[mu, kL] = mu^-2 2 pi chi^2 / F^2 / trapz_kS sanitize(kS (W Pge)^2 / ((W^2 Pgg + ngg) C(chi kS)))."""
    W = np.ones((mus.size, kLs.size, 1))
    if sig is not None:
        kr = mus[:, None] * kLs[None, :]
        W = np.exp(-sig ** 2 * kr ** 2 / 2 / H ** 2)[..., None]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        y = kSs * (W * Pge) ** 2 / ((W ** 2 * Pgg + ngg) * cls_at(Cls, chi * kSs))
    y[~np.isfinite(y)] = 0
    return (mus[:, None] ** -2.0 * 2 * np.pi * chi ** 2 / F ** 2) / _trapz(y, kSs, axis=-1)


def bilinear_clamped(zs, ks, P, z, k):
    z = np.clip(z, zs[0], zs[-1])
    k = np.clip(k, ks[0], ks[-1])
    i = np.clip(np.searchsorted(zs, z, side="right") - 1, 0, zs.size - 2)
    j = np.clip(np.searchsorted(ks, k, side="right") - 1, 0, ks.size - 2)
    tz = (z - zs[i]) / (zs[i + 1] - zs[i])
    tk = (k - ks[j]) / (ks[j + 1] - ks[j])
    return ((1 - tz) * (1 - tk) * P[j, i] + (1 - tz) * tk * P[j + 1, i] + tz * (1 - tk) * P[j, i + 1]
            + tz * tk * P[j + 1, i + 1])


def limber_def(ells, chi, zn, zs, ks, P, squeezed, c2, T2):
    """cl = trapz_chi P(z, ell/chi) (1+z)^4 / chi^2 * (1 or 0.5) * c2 * T2."""
    p = bilinear_clamped(zs, ks, P, zn, ells[:, None] / chi)
    v = p * (1 + zn) ** 4 / chi ** 2 * (1.0 if squeezed else 0.5) * c2 * T2
    return np.array([_trapz(v[i], chi[i]) for i in range(len(ells))])


def cl_prefactors(g):
    from hmvec_amd import ksz
    from hmvec_amd.params import default_params
    c2 = (ksz.constants['thompson_SI'] * g["c_ne0"][0] / ksz.constants['meter_to_megaparsec']) ** 2
    return c2, default_params["T_CMB"] ** 2


# ------------------------------------------------------------------------------------------ restatements vs reference
def test_pqperp_definition_matches_reference(g):
    P, Pabs = pqperp_def(g["c_ks"], g["c_mus"], g["c_Pee"], g["c_Pmm"], g["c_adotf"])
    assert np.all(np.abs(P - g["c_pqperp"]) <= 1e-12 * Pabs)


def test_nvv_definition_matches_reference(g):
    Cls = g["Cls"].copy()
    for tag, sig in (("a", None), ("b", g["meta"]["sigz"])):
        for iz in range(g["zs"].size):
            z = g["zs"][iz]
            got = nvv_def(g[tag + "_chistars"][iz], g[tag + "_kstars"][iz], g[tag + "_mu"], g[tag + "_kLs"],
                          g[tag + "_kS"], Cls, g[tag + "_in_Pge"][iz], g[tag + "_in_Pgg"][iz], 1 / g["ngals"][iz],
                          None if sig is None else sig * (1 + z), g[tag + "_in_Hphoto"][iz])
            assert np.allclose(got, g[tag + "_Nvv"][iz], rtol=1e-12, atol=0), (tag, iz)


def test_limber_definition_matches_reference(g):
    c2, T2 = cl_prefactors(g)
    for tag, P, sq in (("c", g["c_pqperp"], False), ("d", g["d_pqr"], True)):
        got = limber_def(g["ells"], g["c_chi_nodes"], g["c_z_nodes"], g["zs"], g["c_ks"], P, sq, c2, T2)
        assert np.allclose(got, g[tag + "_cl"], rtol=1e-12, atol=0), tag
    assert g["c_cl"][-1] < 0 and g["d_cl"][-1] < 0          # ell/30 above chi_max: descending nodes


def test_fixture_crosses_lmax_inside_the_ks_range(g):
    ell = g["a_chistars"][:, None] * g["a_kS"][None, :]
    assert np.any(ell > g["Cls"].size - 1) and np.any(ell < g["Cls"].size - 1)


# ------------------------------------------------------------------------------------------ host helpers
def test_scalar_helpers_match_reference(g):
    from hmvec_amd import ksz
    from hmvec_amd.params import default_params
    p = dict(default_params)
    ombh2, yhe = p["ombh2"], 0.2454
    assert ksz.Ngg(2e-4) == 1 / 2e-4
    assert ksz.get_kmin(2.0) == np.pi / (2e9) ** (1 / 3)
    assert ksz.chi(0.24, 0) == (1 - 0.24) / (1 - 0.12)
    assert np.isclose(ksz.ne0_shaw(ombh2, yhe), g["c_ne0"][0], rtol=1e-15)
    K = [ksz.ksz_radial_function(z, ombh2, yhe) for z in g["zs"]]
    assert np.allclose(K, g["a_kstars"], rtol=1e-15, atol=0)
    assert ksz.defaults == {'min_mass': 1e6, 'max_mass': 1e16, 'num_mass': 1000}
    assert ksz.constants['thompson_SI'] == 6.6524e-29


def test_get_interpolated_cls_quirks():
    from hmvec_amd import ksz
    Cls = np.arange(10.0) + 5
    out = ksz.get_interpolated_cls(Cls, 2.0, np.array([0.2, 0.6, 1.2, 2.4, 4.5, 4.6]))
    assert Cls[0] == 0 and Cls[1] == 0 and Cls[2] == 7           # the caller's array is zeroed below l = 2
    assert np.array_equal(out, [0.0, 0.0, 7.0, 9.0, 14.0, np.inf])
    x = np.array([1.0, np.inf, np.nan, -2.0])
    assert np.array_equal(ksz._sanitize(x), [1.0, 0.0, 0.0, -2.0])


def test_pge_err_core_matches_reference(g):
    from hmvec_amd import ksz
    Cls = g["Cls"].copy()
    edges = g["a_Pge_err_edges"]
    for iz in range(g["zs"].size):
        pggtot = (g["a_in_Pgg"][iz] + 1 / g["ngals"][iz])[0]     # the reference passes sPggtot[z][0]: a scalar
        got = ksz.pge_err_core(g["a_vrec"][iz], g["a_kstars"][iz], g["a_chistars"][iz], g["meta"]["vol"],
                               g["a_kS"], edges, pggtot, Cls)
        assert np.allclose(got, g["a_Pge_err"][iz], rtol=1e-12, atol=0)


def test_abi_declares_the_ksz_entry_points():
    from hmvec_amd import _native as nat
    hdr = open(os.path.join(REPO, "include", "hmgrid.h")).read()
    for name in ("hmg_ksz_pqperp", "hmg_ksz_nvv", "hmg_ksz_limber_cl"):
        assert name in nat.SIGNATURES
        assert name + "(" in hdr


def test_module_surface():
    from hmvec_amd import ksz
    for name in ("defaults", "constants", "Ngg", "get_survey_volume", "get_kmin", "chi", "ne0_shaw",
                 "ksz_radial_function", "_sanitize", "get_interpolated_cls", "pge_err_core", "kSZ",
                 "Nvv_core_integral", "get_ksz_template_signal_snapshot", "get_ksz_snr", "get_ksz_auto_signal_mafry",
                 "get_ksz_auto_squeezed", "Nvv"):
        assert hasattr(ksz, name), name
    for m in ("__init__", "Pge_err", "lPvv", "lPgg", "lPgv", "ksz_radial_function", "Wphoto", "Nvv"):
        assert m in ksz.kSZ.__dict__, m
    assert not hasattr(ksz, "Pqperp_igr_poly")
    import hmvec_amd
    assert hmvec_amd.ksz is ksz and not hasattr(hmvec_amd, "kSZ")


def test_squeezed_leaves_the_params_it_was_given(monkeypatch):
    """get_ksz_auto_squeezed widens the HOD bisection range on a copy: the caller's dict and default_params stay."""
    from hmvec_amd import ksz
    from hmvec_amd.params import default_params
    seen = {}

    class Stop(Exception):
        pass

    def fake_kSZ(*a, **kw):
        seen.update(kw["params"])
        raise Stop

    monkeypatch.setattr(ksz, "kSZ", fake_kSZ)
    mine = {"H0": 70.0}
    before = dict(default_params)
    for params in (mine, None):
        with pytest.raises(Stop):
            ksz.get_ksz_auto_squeezed(np.array([100.0]), 1.0, [0.5, 1.0], [1e-4, 1e-4], [1.0, 1.0], params=params)
        assert seen["hod_bisection_search_min_log10mthresh"] == 1
    assert mine == {"H0": 70.0} and default_params == before


# ------------------------------------------------------------------------------------------ background methods
def _cosmo(**over):
    from hmvec_amd.cosmology import Cosmology
    return Cosmology(params=over, engine="analytic", accuracy="low")


def test_growth_rate_matches_dlnD_dlna_and_the_growth_ode():
    c = _cosmo()
    zs = np.array([0.0, 0.3, 0.8, 1.5, 3.0, 6.0])
    f = c.get_growth_rate_f(zs)
    assert f.shape == zs.shape
    a = 1 / (1 + zs)
    eps = 1e-5
    fd = (np.log(c.D_growth_approx(a * np.exp(eps))) - np.log(c.D_growth_approx(a * np.exp(-eps)))) / (2 * eps)
    assert np.allclose(f, fd, rtol=1e-8, atol=0)

    # D'' + (3/a + E'/E) D' = 3/2 Omega_m D / (a^5 E^2), from D = a deep in matter domination
    om = c.omm0

    def E(a):
        return np.sqrt(om / a ** 3 + (1 - om))

    def rhs(a, y):
        D, dD = y
        dlnE = -1.5 * om / a ** 4 / E(a) ** 2
        return [dD, -(3 / a + dlnE) * dD + 1.5 * om / (a ** 5 * E(a) ** 2) * D]

    a0 = 1e-3
    sol = solve_ivp(rhs, (a0, 1.0), [a0, 1.0], rtol=1e-12, atol=1e-15, dense_output=True)
    D, dD = sol.sol(a)
    assert np.allclose(f, a * dD / D, rtol=2e-6, atol=0)
    assert c.get_growth_rate_f(0.3).shape == (1,) and c.get_growth_rate_f(0.3)[0] == f[1]


def test_growth_rate_refuses_non_lcdm():
    for over in (dict(w0=-0.9), dict(wa=0.1), dict(omk=0.01)):
        with pytest.raises(NotImplementedError):
            _cosmo(**over).get_growth_rate_f([0.5])


def test_growth_rate_prefers_the_provider():
    from hmvec_amd.background import AnalyticBackground
    from hmvec_amd.cosmology import Cosmology

    class Bg(AnalyticBackground):
        def growth_rate_f(self, zs):
            return 0.5 + 0 * np.asarray(zs)

    c = Cosmology(engine="analytic", accuracy="low", background=Bg(67.0, 0.022, 0.12))
    assert np.array_equal(c.get_growth_rate_f([0.1, 0.2]), [0.5, 0.5])


def test_redshift_at_comoving_radial_distance_round_trips():
    for over in ({}, dict(w0=-0.8, wa=0.2), dict(omk=0.05)):
        c = _cosmo(**over)
        zs = np.concatenate([[0.0], np.geomspace(1e-4, 1100.0, 300)])
        chi = c.comoving_radial_distance(zs)
        z = c.redshift_at_comoving_radial_distance(chi)
        assert np.allclose(z, zs, rtol=1e-10, atol=1e-14)
        back = c.comoving_radial_distance(z)
        assert np.all(np.abs(back - chi) <= 1e-12 * chi)
        grid = np.geomspace(10.0, 9000.0, 12).reshape(3, 4)
        zz = c.redshift_at_comoving_radial_distance(grid)
        assert zz.shape == (3, 4)
        assert np.all(np.abs(c.comoving_radial_distance(zz) - grid) <= 1e-12 * grid)
    one = c.redshift_at_comoving_radial_distance(3000.0)
    assert isinstance(one, float)
    with pytest.raises(ValueError):
        c.redshift_at_comoving_radial_distance(-1.0)


def test_redshift_at_comoving_radial_distance_prefers_the_provider():
    from hmvec_amd.background import AnalyticBackground
    from hmvec_amd.cosmology import Cosmology

    class Bg(AnalyticBackground):
        def redshift_at_comoving_radial_distance(self, chi):
            return 42.0 + 0 * chi

    c = Cosmology(engine="analytic", accuracy="low", background=Bg(67.0, 0.022, 0.12))
    assert c.redshift_at_comoving_radial_distance(np.array([1.0])) == 42.0

