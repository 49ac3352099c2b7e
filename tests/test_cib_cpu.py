"""The CIB halo model, the parts that need no GPU: NlnMsub against the reference's recorded values,
the SED break and both branches of the SED against 40-digit mpmath, the pair index, the numpy restatement's separability
without a flux cut and its loss with one, the Limber algebra, every refusal, the ABI and the exports."""
import inspect
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import cib_model as cbm  # noqa: E402

import hmvec_amd as hm  # noqa: E402
from hmvec_amd import cib, tinker  # noqa: E402
from hmvec_amd.quadrature import trapz_weights  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NUS = np.array([217.0, 353.0, 545.0, 857.0, 3000.0])
ZS = np.array([0.3, 1.2, 2.6])
CHIS = np.array([1900.0, 4400.0, 6400.0])
MS = np.geomspace(5e9, 10 ** 15.5, 70)


def test_nlnmsub_is_the_reference_formula():
    d = np.load(os.path.join(REPO, "tests", "golden", "cib_pins.npz"))
    got = tinker.NlnMsub(d["Msubs"], d["Mhosts"])
    assert got.shape == (12, 9) and np.any(d["Msubs"][:, None] > d["Mhosts"][None, :])
    assert np.allclose(got, d["NlnMsub"], rtol=4e-16, atol=0)
    assert np.all(got >= 0) and got[0, -1] > got[-1, 0]


# ---------------------------------------------------------------- the SED
def _mp():
    import mpmath as mp
    mp.mp.dps = 40
    return mp


@pytest.mark.parametrize("beta,gamma", [(1.75, 1.7), (1.5, 2.0), (2.0, 1.2), (0.0, 0.5)])
def test_sed_break_against_mpmath(beta, gamma):
    mp = _mp()
    s = 3 + mp.mpf(beta) + mp.mpf(gamma)
    want = mp.findroot(lambda x: x / (1 - mp.exp(-x)) - s, s)
    got = hm.sed_break(beta, gamma)
    assert abs(mp.mpf(got) - want) <= 4 * 2.0 ** -52 * want
    # the slope of the modified blackbody nu^(3 + beta) / expm1(x) at x0 is -gamma
    slope = 3 + mp.mpf(beta) - want * mp.exp(want) / mp.expm1(want)
    assert abs(slope + mp.mpf(gamma)) < mp.mpf(10) ** -30


def test_sed_on_both_branches_against_mpmath_and_continuity():
    mp = _mp()
    p = dict(cib.cib_defaults)
    x0 = hm.sed_break(p["beta"], p["gamma"])
    nus = np.array([100.0, 217.0, 353.0, 545.0, 857.0, 1500.0, 3000.0, 5000.0])
    zs = np.array([0.0, 0.3, 1.2, 2.6, 4.0])
    got = hm.cib_sed(nus, zs)
    assert got.shape == (8, 5)
    below = above = 0
    for i, nu in enumerate(nus):
        for j, z in enumerate(zs):
            zp1 = 1 + mp.mpf(float(z))
            T = mp.mpf(p["T0"]) * zp1 ** mp.mpf(p["alpha"])
            nu0 = mp.mpf(x0) * mp.mpf(cib.KH_GHZ) * T
            r = zp1 * mp.mpf(float(nu)) / nu0
            if r < 1:
                want = r ** (3 + mp.mpf(p["beta"])) * mp.expm1(mp.mpf(x0)) / mp.expm1(mp.mpf(x0) * r)
                below += 1
            else:
                want = r ** (-mp.mpf(p["gamma"]))
                above += 1
            # pow, expm1 and the argument's roundings: x0 r <= 7 moves expm1 by 7 EPS; a dozen EPS in all
            assert abs(mp.mpf(float(got[i, j])) - want) <= 32 * 2.0 ** -52 * want, (nu, z)
    assert below >= 10 and above >= 10
    assert np.all(got[-2, 1:] == (((1 + zs[1:]) * 3000.0) / ((x0 * cib.KH_GHZ) * (p["T0"] * (1 + zs[1:]) ** p["alpha"]))) ** -p["gamma"])
    # continuity at nu0: the two branches meet at 1 with the same logarithmic slope
    z = 1.2
    nu0 = x0 * cib.KH_GHZ * p["T0"] * (1 + z) ** p["alpha"] / (1 + z)
    eps = 1e-6
    lo, at, hi = hm.cib_sed([nu0 * (1 - eps), nu0, nu0 * (1 + eps)], [z])[:, 0]
    assert abs(at - 1.0) < 1e-14 and abs(lo - (1 + p["gamma"] * eps)) < 1e-9 and abs(hi - (1 - p["gamma"] * eps)) < 1e-9
    with pytest.raises(ValueError):
        hm.sed_break(-3.0, 0.5)
    with pytest.raises(ValueError):
        hm.cib_sed([217.0, -1.0], zs)
    with pytest.raises(ValueError):
        hm.cib_sed(nus, zs, params={"T_zero": 3.0})


def test_defaults_are_the_issue_table():
    assert cib.cib_defaults == dict(alpha=0.36, T0=24.4, beta=1.75, gamma=1.7, delta=3.6, z_p=2.0, log10_M_eff=12.6,
                                    sigma2=0.5, M_min=1e10, L0=1.0)
    assert not any("cib" in k for k in hm.default_params)
    assert cib.PARAMETERS == tuple(cib.cib_defaults)


# ---------------------------------------------------------------- pairs
def test_pair_index_and_list():
    for F in (1, 4, 5, 9, 16):
        pairs = cib.pair_list(F)
        assert len(pairs) == F * (F + 1) // 2
        for i, (f, g) in enumerate(pairs):
            assert f <= g and cib.pair_index(f, g, F) == i == cib.pair_index(g, f, F) == f * F - f * (f - 1) // 2 + (g - f)
    with pytest.raises(ValueError):
        cib.pair_index(0, 5, 5)


# ---------------------------------------------------------------- the restatement
def _setup(nsub=16):
    rng = np.random.default_rng(5)
    p = dict(cib.cib_defaults)
    x0 = hm.sed_break(p["beta"], p["gamma"])
    t, w = hm.sub_rule(nsub)
    nk = 9
    ks = np.geomspace(1e-2, 10.0, nk)
    nzm = rng.uniform(0.5, 1.5, (3, 70)) * (MS[None, :] / 1e12) ** -1.9 * np.exp(-MS[None, :] / 3e14)
    bh = rng.uniform(0.8, 1.2, (3, 70)) * (1.0 + (MS[None, :] / 1e13) ** 0.5)
    us = 1.0 / (1.0 + (ks[None, None, :] * (MS[None, :, None] / 1e12) ** (1 / 3) * 0.1) ** 2) ** 2 + 0.0 * ZS[:, None, None]
    Pzk = rng.uniform(1e2, 1e4, (3, nk))
    return p, x0, t, w, ks, nzm, bh, us, Pzk


def test_sub_rule_and_the_subhalo_integral():
    t, w = hm.sub_rule(64)
    assert t.shape == w.shape == (64,) and np.all(np.diff(t) > 0) and 0 < t[0] and t[-1] < 1 and abs(w.sum() - 1) < 1e-14
    assert hm.sub_rule is hm.quadrature.sub_rule
    for bad in (1, 0, 2.0, True, None):
        with pytest.raises(ValueError):
            hm.sub_rule(bad)
    # 64 nodes against 256: the integrand is smooth on the row's own interval
    p, x0 = dict(cib.cib_defaults), hm.sed_break(1.75, 1.7)
    a = cbm.luminosities(ZS, MS, CHIS, NUS, p, x0, None, *hm.sub_rule(64))
    b = cbm.luminosities(ZS, MS, CHIS, NUS, p, x0, None, *hm.sub_rule(256))
    live = MS > p["M_min"]
    assert np.all(a["Ls"][..., ~live] == 0) and np.all(a["Lc"][..., MS < p["M_min"]] == 0) and (~live).any()
    assert np.all(a["Ls"][..., live] > 0) and np.allclose(a["Ls"], b["Ls"], rtol=1e-9, atol=0)
    # the node sum against NlnMsub itself
    hw = np.log(MS[-1] / p["M_min"])
    msub = p["M_min"] * np.exp(hw * hm.sub_rule(64)[0])
    L = cbm.prefactor(NUS, ZS, p, x0)[2, 1] * cbm.sigma(msub, p) * cib.INV4PI
    want = np.sum(hm.sub_rule(64)[1] * hw * tinker.NlnMsub(msub, MS[-1:])[:, 0] * L)
    assert a["Ls"][2, 1, -1] == pytest.approx(want, rel=1e-13)


def test_separable_without_a_cut_and_not_with_one():
    p, x0, t, w, ks, nzm, bh, us, Pzk = _setup()
    free = cbm.luminosities(ZS, MS, CHIS, NUS, p, x0, None, t, w)
    assert free["central_masked"] == 0 and free["node_masked"] == 0
    r = cbm.spectra(nzm, bh, MS, ks, Pzk, 4e10, us, free["Lc"], free["Ls"], 0.1)
    P, tol = r["P1h"]
    F = NUS.size
    ix = lambda f, g: cib.pair_index(f, g, F)  # noqa: E731
    for f in range(F):
        for g in range(f, F):
            lhs, rhs = P[ix(f, g)] * P[ix(0, 0)], P[ix(0, f)] * P[ix(0, g)]
            bound = (tol[ix(f, g)] * P[ix(0, 0)] + tol[ix(0, 0)] * P[ix(f, g)] + tol[ix(0, f)] * P[ix(0, g)]
                     + tol[ix(0, g)] * P[ix(0, f)] + 4 * cbm.EPS * np.abs(lhs))
            # L is separable in (nu; z, m) at each z: only the prefactor's own rounding is left, a few EPS per factor
            assert np.all(np.abs(lhs - rhs) <= bound + 64 * cbm.EPS * np.abs(lhs)), (f, g)
    fc = 0.37 * (free["Lc"] * 4 * np.pi / ((4 * np.pi * (1 + ZS)) * CHIS ** 2)[None, :, None]).max(axis=(1, 2))
    cut = cbm.luminosities(ZS, MS, CHIS, NUS, p, x0, fc, t, w)
    assert 0.01 < cut["central_masked"] < 0.6 and 0.01 < cut["node_masked"] < 0.6
    assert min(cut["central_margin"], cut["node_margin"]) >= 1e-9
    Pc = cbm.spectra(nzm, bh, MS, ks, Pzk, 4e10, us, cut["Lc"], cut["Ls"], 0.1)["P1h"][0]
    worst = max(float(np.max(np.abs(Pc[ix(f, g)] * Pc[ix(0, 0)] / (Pc[ix(0, f)] * Pc[ix(0, g)]) - 1)))
                for f in range(1, F) for g in range(f, F))
    assert worst > 1e-3
    # the term as written against the cancelling form, where it still has its digits (low k)
    lc, t_ = free["Lc"][..., None], free["Ls"][..., None] * us[None]
    wgt = (trapz_weights(MS)[None, :] * nzm)[None, :, :, None]
    G00 = (wgt * ((lc[0] + t_[0]) ** 2 - lc[0] ** 2)).sum(axis=-2)
    assert np.allclose(G00[0, :, 0], r["G"][0][0, :, 0], rtol=1e-10)


def test_cl_algebra_on_host_arrays():
    rng = np.random.default_rng(2)
    zs, ks = np.array([0.2, 0.9, 1.7, 2.5]), np.geomspace(1e-3, 5.0, 40)
    chis, hzs = 2900.0 * zs ** 0.8, 2.3e-4 * (1 + zs) ** 1.3
    planes = rng.uniform(1.0, 2.0, (3, 4, 40)) * ks[None, None, :] ** -1.5
    ells = np.array([2.0, 30.0, 500.0, 3000.0, 40000.0])
    Wj = cib.emission_window(zs, hzs)
    assert np.array_equal(Wj, 1.0 / ((1 + zs) * hzs))
    got = cib.cl_from_planes(ells, zs, ks, chis, hzs, planes, Wj, Wj)
    assert got.shape == (3, 5)
    tw = trapz_weights(zs)
    for i in range(3):
        for j, ell in enumerate(ells):
            k = np.clip((ell + 0.5) / chis, ks[0], ks[-1])
            want = sum(tw[z] / ((1 + zs[z]) ** 2 * hzs[z] * chis[z] ** 2) * np.interp(k[z], ks, planes[i, z]) for z in range(4))
            assert got[i, j] == pytest.approx(want, rel=1e-12)
    # a power law in k, linear in each cell, has a closed form: int dchi a^2 / chi^2 (alpha + beta k)
    lin = (3.0 + 2.0 * ks)[None, :] + 0.0 * zs[:, None]
    got = cib.cl_from_planes(np.array([100.0]), zs, ks, chis, hzs, lin, Wj, 1.0 + 0.0 * zs)
    want = np.sum(tw * hzs * Wj / chis ** 2 * (3.0 + 2.0 * 100.5 / chis))
    assert got[0] == pytest.approx(want, rel=1e-12)
    # assemble: the two-halo planes and the totals
    P1h, I = rng.uniform(1, 2, (3, 4, 6)), rng.uniform(1, 2, (2, 4, 6))
    X1h, Pzk, J = rng.uniform(1, 2, (1, 2, 4, 6)), rng.uniform(1, 2, (4, 6)), rng.uniform(1, 2, (1, 4, 6))
    auto, cross = cib.assemble(P1h, I, X1h, Pzk, J)
    assert np.array_equal(auto["2h"][1], (Pzk * I[0]) * I[1]) and np.array_equal(auto["total"], P1h + auto["2h"])
    assert np.array_equal(cross["2h"][0, 1], (Pzk * I[1]) * J[0]) and np.array_equal(cross["total"], X1h + cross["2h"])
    assert cib.assemble(P1h, I, None, Pzk, None)[1] is None


# ---------------------------------------------------------------- refusals
class StandIn:
    """A host-only stand-in for a HaloModel: any touch of a context fails the test."""
    zs = ZS
    ms = MS
    ks = np.geomspace(1e-2, 10, 9)
    p = {"kstar_damping": 0.01}
    _nz = property(lambda self: self.zs.size)
    _nm = property(lambda self: self.ms.size)
    _nk = property(lambda self: self.ks.size)

    def __init__(self):
        self.uk_profiles, self.pk_profiles, self.hods, self.version = {"nfw": None, "gas": None}, {"y": None}, {"g": None}, 0

    def _main(self, needs_aux=False):
        raise AssertionError("a context is touched")

    def _bump(self):
        self.version += 1

    def comoving_radial_distance(self, z):
        return 3000.0 * np.asarray(z)


def _record(F=2, jbar=None):
    jbar = np.ones((F, 3)) if jbar is None else jbar
    return cib.EmissionTables(Lc=None, Ls=None, jbar=jbar, bias=np.ones((F, 3)), F=F, nus=None, params=None, flux_cut=None,
                              shape=(F, 3, 70))


def test_every_refusal_touches_nothing():
    m = StandIn()
    for kw in (dict(nus_GHz=[]), dict(nus_GHz=[217.0, np.nan]), dict(nus_GHz=[[217.0]]), dict(nus_GHz=np.arange(1, 18) * 100.0),
               dict(nus_GHz=NUS, nsub=1), dict(nus_GHz=NUS, nsub=8.0), dict(nus_GHz=NUS, flux_cut=[1.0, 2.0]),
               dict(nus_GHz=NUS, flux_cut=-np.ones(5)), dict(nus_GHz=NUS, flux_cut=np.full(5, np.nan)),
               dict(nus_GHz=NUS, params={"sigma2": 0.0}), dict(nus_GHz=NUS, params={"nope": 1.0}),
               dict(nus_GHz=NUS, params={"M_min": -1.0}), dict(nus_GHz=NUS, params={"T0": np.inf})):
        with pytest.raises(ValueError):
            hm.cib_luminosities(m, **kw)
    shuffled = StandIn()
    shuffled.ms = MS[::-1]
    with pytest.raises(ValueError):
        hm.cib_luminosities(shuffled, NUS)
    good = np.ones((2, 3, 70))
    for Lc, Ls in ((np.ones((3, 70)), np.ones((3, 70))), (good, np.ones((2, 3, 69))), (good, np.ones((3, 3, 70))),
                   (np.ones((17, 3, 70)), np.ones((17, 3, 70))), (good, good * np.nan), (np.ones((0, 3, 70)), np.ones((0, 3, 70)))):
        with pytest.raises(ValueError):
            hm.emission_tables(m, Lc, Ls)
    with pytest.raises(ValueError):
        hm.emission_tables(shuffled, good, good)
    rec = _record()
    for kw in (dict(partners=("nope",)), dict(partners=("g",)), dict(partners=("nfw", "y", "gas")),
               dict(satellite_profile_name="y"), dict(satellite_profile_name="nope"), dict(kindex=[0, 9]), dict(kindex=[-1]),
               dict(kindex=[]), dict(kindex=[0.5])):
        with pytest.raises(ValueError):
            hm.emission_power_device(m, rec, **kw)
        with pytest.raises(ValueError):
            hm.get_power_cib(m, None, tables=rec, **{"partners": (), **kw})
    with pytest.raises(ValueError):
        hm.emission_power_device(m, dict(Lc=good))
    other = cib.EmissionTables(Lc=None, Ls=None, jbar=None, bias=None, F=2, nus=None, params=None, flux_cut=None, shape=(2, 3, 8))
    with pytest.raises(ValueError):
        hm.emission_power_device(m, other)
    with pytest.raises(ValueError):
        hm.get_power_cib(m, NUS, nsub=1)
    for kw in (dict(ells=[[2.0]]), dict(ells=[-1.0]), dict(ells=[]), dict(ells=[10.0], partners=("nope",)),
               dict(ells=[10.0], partners=("nfw",), windows=[np.ones(2)]), dict(ells=[10.0], partners=("nfw",), windows=[])):
        with pytest.raises(ValueError):
            hm.cl_cib(m, tables=rec, **kw)
    for kw in (dict(name="nfw", f=0), dict(name="y", f=0), dict(name="g", f=0), dict(name="", f=0), dict(name="c", f=2),
               dict(name="c", f=-1), dict(name="c", f=0.0), dict(name="c", f=0, satellite_profile_name="y")):
        with pytest.raises(ValueError):
            hm.register_emission(m, tables=rec, **kw)
    dark = np.ones((2, 3))
    dark[1, 2] = 0.0
    with pytest.raises(ValueError):
        hm.register_emission(m, "c", _record(jbar=dark), 1)
    assert set(m.hods) == {"g"} and m.version == 0
    with pytest.raises(AttributeError):
        rec.F = 3
    assert not rec.jbar.flags.writeable


# ---------------------------------------------------------------- ABI and exports
def test_entry_points_are_declared_and_bound_and_the_abi_version_stays():
    from hmvec_amd import _native as nat
    from hmvec_amd.halomodel import HaloModel
    header = open(os.path.join(REPO, "include", "hmgrid.h")).read()
    for name, count in (("hmg_cib_luminosity", 15), ("hmg_emission_power", 21)):
        m = re.search(r"\bint %s\(hmg_ctx\* ctx, ([^;]*)\);" % name, header)
        assert m, name
        declared = re.sub(r"/\*.*?\*/", "", m.group(0), flags=re.S)
        assert declared.count(",") + 1 == count == len(nat.SIGNATURES[name]) == len(nat.PARAMS[name])
    par = nat.PARAMS["hmg_cib_luminosity"]
    assert par == ("ctx", "F", "nz", "nm", "nsub", "d_nus", "d_zs", "d_ms", "d_chis", "d_scut", "d_t", "d_w", "h_par", "d_Lc", "d_Ls")
    par = nat.PARAMS["hmg_emission_power"]
    assert par[:11] == ("ctx", "F", "nz", "nm", "nk", "n", "d_us", "d_Lc", "d_Ls", "NP", "h_partners")
    assert par[-5:] == ("d_kindex", "d_damp", "d_P1h", "d_I", "d_X1h")
    assert [n for n in par if n in HaloModel._MODEL_BLOCK] == ["d_nzm", "d_bh", "d_ms", "d_wm", "rho_m0"]
    import ctypes as C
    assert nat.SIGNATURES["hmg_emission_power"][10] is C.POINTER(nat.Tracer)
    assert nat.DEFINES["HMG_CIB_NPAR"] == len(cib.PARAMETERS) + 1 == 11
    assert nat.DEFINES["HMG_CIB_FMAX"] == cib.FMAX >= 16
    assert int(re.search(r"#define HMG_ABI_VERSION (\d+)", header).group(1)) == 10 == nat.ABI_VERSION
    mk = open(os.path.join(REPO, "hmvec_amd", "csrc", "Makefile")).read()
    assert re.search(r"^KUNITS = .*\bcib\b", mk, flags=re.M) and re.search(r"^DEPS_cib\s*=\s*kernels/cib\.hpp", mk, flags=re.M)
    hpp = open(os.path.join(REPO, "hmvec_amd", "csrc", "kernels", "cib.hpp")).read()
    assert cib.FREQ_TILE == int(re.search(r"constexpr int CIB_T = (\d+);", hpp).group(1))
    assert float(re.search(r"CIB_KH = ([0-9.]+);", hpp).group(1)) == cib.KH_GHZ
    assert float(re.search(r"CIB_INV4PI = ([0-9.]+);", hpp).group(1)) == cib.INV4PI == 1.0 / (4.0 * np.pi)
    assert float(re.search(r"CIB_FOURPI = ([0-9.]+);", hpp).group(1)) == cib.FOURPI == 4.0 * np.pi
    nat.load()          # the library exports both symbols (AttributeError if not)


def test_exports():
    names = ("cib_defaults", "sed_break", "cib_sed", "sub_rule", "cib_luminosities", "emission_tables", "emission_power_device",
             "get_power_cib", "cl_cib", "register_emission")
    for name in names:
        assert getattr(hm, name) is getattr(cib, name) and name in hm.__all__ and name in cib.__all__
    assert hm.cib is cib and "cib" in hm.__all__
    assert list(inspect.signature(hm.cib_luminosities).parameters) == ["model", "nus_GHz", "params", "flux_cut", "nsub"]
    assert inspect.signature(hm.cib_luminosities).parameters["nsub"].default == 64
    assert list(inspect.signature(hm.emission_power_device).parameters) == ["model", "tables", "partners", "satellite_profile_name",
                                                                             "kindex", "damping"]
    assert inspect.signature(hm.get_power_cib).parameters["partners"].default == ("nfw",)
    assert list(inspect.signature(hm.register_emission).parameters)[:5] == ["model", "name", "tables", "f", "satellite_profile_name"]
    assert list(inspect.signature(hm.cl_cib).parameters)[:5] == ["model", "ells", "tables", "partners", "windows"]
    assert not any(hasattr(hm.HaloModel, n) for n in names)
