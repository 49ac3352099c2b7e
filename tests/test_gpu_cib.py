"""GPU checks of the CIB halo model (hmvec_amd.cib; hmg_cib_luminosity, hmg_emission_power); definitions and gates in
DESIGN.md section 26.

Three redshifts, one above z_p = 2; 70 masses (a full 64-mass tile and a partial one) with ms[0] < M_min, so the zero rows
exist; 33 wavenumbers; 217, 353, 545, 857 and 3000 GHz - 3000 GHz is on the power-law branch of the SED at z >= 0.5 -
extended to 9 frequencies; 16 and 64 nodes of the subhalo integral; F = 1, 4, 5 and 9 for the contraction's tile of 4
frequencies; the whole k grid and a strided subset; "nfw" (the satellite tensor itself: loaded once), a Battaglia gas
tensor and a pressure tensor as partners.

The luminosities are compared with the numpy restatement (tests/helpers/cib_model.py) at (nsub + C_DEVICE) EPS sum |w f|,
the flux-cut decisions exactly, the spectra with the restatement at its derived tol and with get_power_1halo /
get_power_2halo of the registered entry (twice the restatement's tol, the other kernel's damping tol added)."""
import os
import sys

import numpy as np
import pytest

import hmvec_amd as hm
from hmvec_amd import cib

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import cib_model as cbm  # noqa: E402
from lensing_model import model  # noqa: E402

pytestmark = pytest.mark.gpu

NM, NK = 70, 33
ZS = np.array([0.3, 1.2, 2.6])
NUS = np.array([217.0, 353.0, 545.0, 857.0, 3000.0])
NUS9 = np.concatenate([NUS, [100.0, 143.0, 1200.0, 2000.0]])
STRIDED = np.arange(1, NK, 5)
P = dict(cib.cib_defaults)
X0 = hm.sed_break(P["beta"], P["gamma"])


@pytest.fixture(scope="module")
def h():
    m = model(ZS, ks=np.geomspace(1e-3, 30, NK), ms=np.geomspace(7e9, 10 ** 15.5, NM))
    m.add_battaglia_profile("electron", family="AGN", xmax=20, nxs=512)
    m.add_battaglia_pres_profile("y", family="pres", xmax=5, nxs=512)
    return m


def chis(h):
    return np.asarray(h.comoving_radial_distance(ZS), dtype=float).reshape(-1)


_CUT, _TAB, _REF, _POW = {}, {}, {}, {}


def flux_cut(h, nus):
    """S_cut[f] = 0.37 max_{z, m} of the central flux, from the restatement alone."""
    key = nus.size
    if key not in _CUT:
        free = cbm.luminosities(ZS, h.ms, chis(h), nus, P, X0, None, *hm.sub_rule(16))
        S = (free["Lc"] / cib.INV4PI) / ((cib.FOURPI * (1 + ZS)) * chis(h) ** 2)[None, :, None]
        _CUT[key] = 0.37 * S.max(axis=(1, 2))
    return _CUT[key]


def tables(h, nus=NUS, cut=True, nsub=16):
    """The device tables of a case and their host copies, computed once and never changed."""
    key = (nus.size, cut, nsub)
    if key not in _TAB:
        t = hm.cib_luminosities(h, nus, flux_cut=flux_cut(h, nus) if cut else None, nsub=nsub)
        _TAB[key] = (t, t.Lc.numpy(), t.Ls.numpy())
    return _TAB[key]


def lum_ref(h, nus, cut, nsub):
    key = (nus.size, cut, nsub)
    if key not in _REF:
        _REF[key] = cbm.luminosities(ZS, h.ms, chis(h), nus, P, X0, flux_cut(h, nus) if cut else None, *hm.sub_rule(nsub))
    return _REF[key]


def power(h, nus=NUS, partners=("nfw", "y"), kidx=None):
    key = (nus.size, partners, kidx is not None)
    if key not in _POW:
        _POW[key] = hm.get_power_cib(h, None, partners=partners, tables=tables(h, nus)[0], kindex=kidx)
    return _POW[key]


def within(got, want, tol, what):
    err = np.abs(got - want)
    worst = float(np.max(err / np.maximum(tol, 1e-300))) if err.size else 0.0
    print(f"{what}: worst |got - ref| / tol = {worst:.3g}")
    return bool(np.all(err <= tol)), worst


# ---------------------------------------------------------------- 1. the integrand's constant
def test_integrand_constant_of_the_device(h):
    """The measurement of c: the worst error of one device integrand value (w hw) N L / 4 pi against 40-digit mpmath in
    units of EPS |f|, through hmg_cib_luminosity with one-node rules (w = 1) at the nodes of the 16-node rule, every
    eighth node of the 64-node rule and its two outermost.  The gate is twice the recorded value.
    Measured on an MI355X: c = 185.4 at the last node of the 64-node rule (t = 0.99965), 857 GHz, z = 1.2, the 69th mass
    (C_DEVICE_MEASURED in tests/helpers/cib_model.py)."""
    t64 = hm.sub_rule(64)[0]
    nodes = np.concatenate([hm.sub_rule(16)[0], t64[::8], t64[[0, -1]]])
    worst, at = 0.0, None
    for t in nodes:
        d_Lc, d_Ls = cib.luminosity_call(h, NUS, P, X0, None, np.array([t]), np.ones(1))
        got = d_Ls.numpy()
        assert np.all(got[..., h.ms <= P["M_min"]] == 0)
        c, where = cbm.measure_c(got, cbm.exact_integrand(ZS, h.ms, NUS, P, X0, t))
        if c > worst:
            worst, at = c, (float(t),) + where
    print(f"c of the device: {worst:.3f} at (t, f, z, m) = {at}; recorded {cbm.C_DEVICE_MEASURED}, gate {cbm.C_DEVICE}")
    assert worst <= cbm.C_DEVICE


# ---------------------------------------------------------------- 2. luminosities
@pytest.mark.parametrize("nsub", [16, 64])
@pytest.mark.parametrize("cut", [False, True], ids=["free", "cut"])
def test_luminosities_against_the_restatement(h, nsub, cut):
    """Measured on an MI355X, worst |got - restatement| / tol over the four cases: L_c 0.015, L_s 0.020; with the cut every
    source is at least 9.3e-5 from its threshold, 23.5 % of the centrals and 10.5 % of the nodes are masked (DESIGN.md
    section 26)."""
    _, Lc, Ls = tables(h, NUS, cut, nsub)
    ref = lum_ref(h, NUS, cut, nsub)
    ms = h.ms
    dead = ms <= P["M_min"]
    assert ms[0] < P["M_min"] and dead.sum() == 2 and Lc.shape == Ls.shape == (5, 3, NM)
    assert np.all(Lc[..., dead] == 0) and np.all(Ls[..., dead] == 0) and np.all(np.isfinite(Lc)) and np.all(np.isfinite(Ls))
    if cut:
        # the restatement alone: every source is clear of its threshold, and the cut masks a real share of them
        assert min(ref["central_margin"], ref["node_margin"]) >= 1e-9
        assert 0.01 < ref["central_masked"] < 0.6 and 0.01 < ref["node_masked"] < 0.6
        print(f"nsub {nsub}: margin {min(ref['central_margin'], ref['node_margin']):.3g}, masked centrals "
              f"{ref['central_masked']:.3f}, nodes {ref['node_masked']:.3f}")
        # ... so the device must have taken the same decisions: the zeros are the same zeros
        assert np.array_equal(Lc == 0, ref["Lc"] == 0)
        assert np.array_equal(Ls == 0, ref["Ls"] == 0)
    else:
        assert np.all(Lc[..., ~dead] > 0) and np.all(Ls[..., ~dead] > 0)
    tc, ts = cbm.luminosity_tols(ref, nsub)
    ok_c, _ = within(Lc, ref["Lc"], tc, f"L_c nsub {nsub} cut {cut}")
    ok_s, _ = within(Ls, ref["Ls"], ts, f"L_s nsub {nsub} cut {cut}")
    assert ok_c and ok_s
    # jbar and bias are the model's own sums of these arrays
    t = tables(h, NUS, cut, nsub)[0]
    for f in (0, 4):
        assert np.array_equal(t.jbar[f], h.get_ngal(Lc[f], Ls[f])) and np.array_equal(t.bias[f], h.get_bg(Lc[f], Ls[f], t.jbar[f]))


def test_a_luminosity_depends_on_its_own_frequency_only(h):
    t5, Lc5, Ls5 = tables(h, NUS, True, 16)
    t9, Lc9, Ls9 = tables(h, NUS9, True, 16)
    assert np.array_equal(flux_cut(h, NUS9)[:5], flux_cut(h, NUS))
    assert np.array_equal(Lc9[:5], Lc5) and np.array_equal(Ls9[:5], Ls5)
    one = hm.cib_luminosities(h, NUS[3:4], flux_cut=flux_cut(h, NUS)[3:4], nsub=16)
    assert np.array_equal(one.Lc.numpy()[0], Lc5[3]) and np.array_equal(one.Ls.numpy()[0], Ls5[3])
    again = hm.cib_luminosities(h, NUS, flux_cut=flux_cut(h, NUS), nsub=16)
    assert np.array_equal(again.Lc.numpy(), Lc5) and np.array_equal(again.Ls.numpy(), Ls5)


# ---------------------------------------------------------------- 3. spectra against the restatement
@pytest.mark.parametrize("F", [1, 4, 5, 9])
@pytest.mark.parametrize("kidx", [None, STRIDED], ids=["grid", "kindex"])
def test_spectra_against_the_restatement(h, F, kidx):
    """Measured on an MI355X, worst |got - restatement| / tol over the eight cases: 1h 0.080, I 0.055, 2h 0.054, total
    0.065, cross_1h 0.081, cross_2h 0.031, cross_total 0.077."""
    nus = NUS9[:F]
    _, Lc, Ls = tables(h, nus)
    got = power(h, nus, ("nfw", "y"), kidx)
    ref = cbm.from_model(h, Lc, Ls, partners=("nfw", "y"), kindex=kidx)
    n = NK if kidx is None else kidx.size
    npair = F * (F + 1) // 2
    assert got["1h"].shape == (npair, 3, n) and got["I"].shape == (F, 3, n) and got["cross_1h"].shape == (2, F, 3, n)
    assert got["pairs"] == cib.pair_list(F) and got["jbar"].shape == (F, 3)
    for key, rk in (("1h", "P1h"), ("I", "I"), ("2h", "2h"), ("total", "total"), ("cross_1h", "X1h"), ("cross_2h", "cross_2h"),
                    ("cross_total", "cross_total")):
        val, tol = ref[rk]
        assert np.all(np.isfinite(got[key])) and np.all(val > 0) and np.all(tol <= 1e-10 * np.abs(val)), key   # not vacuous
        ok, worst = within(got[key], val, tol, f"F {F} {key}")
        assert ok, (key, worst)


# ---------------------------------------------------------------- 4. against the existing kernels
def test_spectra_against_get_power_of_the_registered_entry(h):
    """Each gate is twice the restatement's tol of the same plane, plus hod_ensemble_model.damping_tol times the undamped sum
    for the one-halo planes (the other kernel's damping factor).  Measured on an MI355X, worst |got - get_power| / gate:
    1h 0.027, 2h 0.027, cross 1h 0.035."""
    t, Lc, Ls = tables(h, NUS)
    got = power(h, NUS, ("nfw", "y"))
    ref = cbm.from_model(h, Lc, Ls, partners=("nfw", "y"))
    dt = cbm.damping_tol(h.ks, h.p["kstar_damping"])[None, :]
    for f in range(NUS.size):
        name = f"cib{f}"
        hm.register_emission(h, name, t, f)
        jbar = t.jbar[f][:, None]
        i = cib.pair_index(f, f, NUS.size)
        tol = 2 * ref["P1h"][1][i] + dt * np.abs(ref["G"][0][i])
        ok, worst = within(got["1h"][i], h.get_power_1halo(name) * jbar ** 2, tol, f"f {f} 1h against get_power_1halo")
        assert ok, (f, worst)
        ok, worst = within(got["2h"][i], h.get_power_2halo(name) * jbar ** 2, 2 * ref["2h"][1][i], f"f {f} 2h against get_power_2halo")
        assert ok, (f, worst)
        for p, partner in enumerate(("nfw", "y")):
            tol = 2 * ref["X1h"][1][p, f] + dt * np.abs(ref["X"][0][p, f])
            ok, worst = within(got["cross_1h"][p, f], h.get_power_1halo(name, partner) * jbar, tol,
                               f"f {f} cross 1h against get_power_1halo(name, {partner!r})")
            assert ok, (f, partner, worst)
    # one derived statistic of a registered name
    xi = h.get_xi(np.array([0.5, 5.0, 50.0]), "cib2")
    assert xi.shape == (3, 3) and np.all(np.isfinite(xi)) and np.all(xi[:, 0] > 0)
    with pytest.raises(ValueError):
        hm.register_emission(h, "cib2", t, 2)
    hm.register_emission(h, "cib2", t, 2, ignore_existing=True)


# ---------------------------------------------------------------- 5. independence and determinism
def test_an_element_does_not_depend_on_the_rest_of_the_call(h):
    t9, Lc, Ls = tables(h, NUS9)
    whole = power(h, NUS9, ("nfw", "y"))
    again = hm.get_power_cib(h, None, partners=("nfw", "y"), tables=t9)
    for k in ("1h", "I", "cross_1h", "2h", "total"):
        assert np.array_equal(whole[k], again[k]), k                                   # a repeat
    ix = lambda f, g: cib.pair_index(f, g, 9)  # noqa: E731
    for f in (0, 3, 4, 8):                                                            # alone: F = 1, no partners
        one = hm.get_power_cib(h, None, partners=(), tables=hm.emission_tables(h, Lc[f:f + 1], Ls[f:f + 1]))
        assert np.array_equal(one["1h"][0], whole["1h"][ix(f, f)]) and np.array_equal(one["I"][0], whole["I"][f]), f
        assert "cross_1h" not in one
    sub = [1, 4, 6, 8]                                # other positions, other tiles, the order kept; one partner, the other
    part = hm.get_power_cib(h, None, partners=("y",), tables=hm.emission_tables(h, Lc[sub], Ls[sub]))
    for a, f in enumerate(sub):
        assert np.array_equal(part["I"][a], whole["I"][f]) and np.array_equal(part["cross_1h"][0, a], whole["cross_1h"][1, f])
        for b in range(a, 4):
            assert np.array_equal(part["1h"][cib.pair_index(a, b, 4)], whole["1h"][ix(f, sub[b])]), (f, sub[b])
    picked = power(h, NUS9, ("nfw", "y"), STRIDED)                                     # 64 threads a workgroup against 33 -> 64
    for k in ("1h", "I", "cross_1h"):
        assert np.array_equal(picked[k], whole[k][..., STRIDED]), k
    gas = hm.get_power_cib(h, None, partners=("electron", "nfw"), tables=t9)           # a partner tensor of its own
    assert np.array_equal(gas["cross_1h"][1], whole["cross_1h"][0]) and np.array_equal(gas["1h"], whole["1h"])
    assert not np.array_equal(gas["cross_1h"][0], gas["cross_1h"][1])
    undamped = hm.emission_power_device(h, t9, partners=("nfw",), damping=False)
    ref = cbm.from_model(h, Lc, Ls, partners=("nfw",), damping=False)
    assert within(undamped.P1h.numpy(), *ref["G"], "undamped P1h")[0] and within(undamped.X1h.numpy(), *ref["X"], "undamped X1h")[0]
    # two frequencies in the other order: the pair is formed with the other frequency first, within the tol
    swapped = hm.get_power_cib(h, None, partners=(), tables=hm.emission_tables(h, Lc[[4, 1]], Ls[[4, 1]]))
    val, tol = cbm.from_model(h, Lc[[1, 4]], Ls[[1, 4]])["P1h"]
    assert np.all(np.abs(swapped["1h"][1] - val[1]) <= tol[1]) and np.array_equal(swapped["1h"][0], whole["1h"][ix(4, 4)])


# ---------------------------------------------------------------- 6. separability and the Limber spectra
def test_separable_without_a_cut_and_the_cl_are_the_host_algebra(h):
    t, Lc, Ls = tables(h, NUS, cut=False)
    got = hm.get_power_cib(h, None, partners=(), tables=t)
    val, tol = cbm.from_model(h, Lc, Ls)["P1h"]
    Pg = got["1h"]
    ix = lambda f, g: cib.pair_index(f, g, 5)  # noqa: E731
    worst = 0.0
    for f in range(5):
        for g in range(f, 5):
            lhs, rhs = Pg[ix(f, g)] * Pg[ix(0, 0)], Pg[ix(0, f)] * Pg[ix(0, g)]
            # the sum of the tols of the four factors, each weighted with its partner, twice (device and restatement), and
            # the restatement's own departure from separability (the prefactor's rounding: 64 EPS, as on the CPU)
            bound = 2 * (tol[ix(f, g)] * val[ix(0, 0)] + tol[ix(0, 0)] * val[ix(f, g)] + tol[ix(0, f)] * val[ix(0, g)]
                         + tol[ix(0, g)] * val[ix(0, f)]) + 68 * cbm.EPS * np.abs(lhs)
            worst = max(worst, float(np.max(np.abs(lhs - rhs) / bound)))
    print(f"separability without a cut: worst |lhs - rhs| / bound = {worst:.3g}")
    assert worst <= 1.0
    cutP = power(h, NUS, ("nfw", "y"))["1h"]
    assert np.max(np.abs(cutP[ix(1, 4)] * cutP[ix(0, 0)] / (cutP[ix(0, 1)] * cutP[ix(0, 4)]) - 1)) > 1e-3
    # C_ell: the device's Limber sums of the device's planes against the host algebra of the same planes
    tc = tables(h, NUS)[0]
    ells = np.array([10.0, 100.0, 1000.0, 5000.0, 30000.0])
    cl = hm.cl_cib(h, ells, tc, partners=("nfw", "y"))
    planes = power(h, NUS, ("nfw", "y"))
    hzs = np.asarray(h.h_of_z(ZS), dtype=float).reshape(-1)
    Wj, Wk = cib.emission_window(ZS, hzs), h.lensing_window(ZS, 1100.0)
    want = cib.cl_from_planes(ells, ZS, h.ks, chis(h), hzs, planes["total"], Wj, Wj)
    assert cl["cl"].shape == (15, 5) and np.all(cl["cl"] > 0) and np.allclose(cl["cl"], want, rtol=1e-12, atol=0)
    for p, W in enumerate((Wk, np.ones(3))):
        want = cib.cl_from_planes(ells, ZS, h.ks, chis(h), hzs, planes["cross_total"][p], Wj, W)
        assert cl["cross"].shape == (2, 5, 5) and np.allclose(cl["cross"][p], want, rtol=1e-12, atol=0), p
    assert np.all(cl["cross"][0] > 0)


# ---------------------------------------------------------------- 7. refusals and no side effects
def test_refusals_and_no_side_effects(h):
    t = tables(h, NUS)[0]
    h.add_hod("g", mthresh=10 ** 10.5 + ZS * 0.0)
    names, version = set(h.hods), h._version
    cached = h.get_power("g", "nfw")
    ctx = h._ctx()
    launched = []
    orig_call, orig_now = ctx.call, ctx.call_now
    ctx.call = lambda name, *a, **kw: (launched.append(name), orig_call(name, *a, **kw))[1]
    ctx.call_now = lambda name, *a: (launched.append(name), orig_now(name, *a))[1]
    try:
        for fn in (lambda: hm.cib_luminosities(h, np.arange(1, 18) * 100.0), lambda: hm.cib_luminosities(h, NUS, nsub=1),
                   lambda: hm.cib_luminosities(h, NUS, flux_cut=-np.ones(5)), lambda: hm.cib_luminosities(h, NUS, flux_cut=np.ones(4)),
                   lambda: hm.emission_tables(h, np.ones((2, 3, NM - 1)), np.ones((2, 3, NM - 1))),
                   lambda: hm.emission_power_device(h, t, partners=("g",)), lambda: hm.emission_power_device(h, t, partners=("nope",)),
                   lambda: hm.emission_power_device(h, t, kindex=[0, NK]), lambda: hm.emission_power_device(h, t, satellite_profile_name="y"),
                   lambda: hm.get_power_cib(h, NUS, partners=("nfw", "y", "electron")),
                   lambda: hm.register_emission(h, "nfw", t, 0), lambda: hm.register_emission(h, "g", t, 0),
                   lambda: hm.register_emission(h, "c", t, 5), lambda: hm.cl_cib(h, [-1.0], t)):
            with pytest.raises(ValueError):
                fn()
        assert not [n for n in launched if "cib" in n or "emission" in n], launched    # every refusal was on the host
        assert set(h.hods) == names and h._version == version
        hm.get_power_cib(h, None, tables=t, kindex=STRIDED)
        assert "hmg_emission_power" in launched and set(h.hods) == names and h._version == version
        del launched[:]
        assert np.array_equal(h.get_power("g", "nfw"), cached)                         # still cached: no mass integrals
        assert not [n for n in launched if "power" in n or "hod" in n], launched
    finally:
        del ctx.call, ctx.call_now
    # the native refusals (a C caller has no host check in front of it)
    from hmvec_amd import _native as nat
    d_u, d_y = h.uk_profiles.dev("nfw"), h.pk_profiles.dev("y")
    P1h, I, X = ctx.empty((15, 3, 2)), ctx.empty((5, 3, 2)), ctx.empty((1, 5, 3, 2))
    d_damp = ctx.upload(np.ones(2))
    block = list(h._model_block("hmg_emission_power").values())      # (in the order of the entry point's parameters)

    def native(F=5, n=2, NP=0, partners=None, d_k=None, X1h=None):
        return ctx.lib.hmg_emission_power(ctx.handle, F, 3, NM, NK, n, d_u.ptr, t.Lc.ptr, t.Ls.ptr, NP, partners, *block,
                                          nat.ptr(d_k), d_damp.ptr, P1h.ptr, I.ptr, nat.ptr(X1h))

    for bad in ([0, NK], [-1, 5]):
        d_k = ctx.upload_int32(np.array(bad, dtype=np.int32))
        assert native(d_k=d_k) != 0 and b"outside 0 .. nk-1" in ctx.lib.hmg_last_error()
    assert native() != 0 and b"n must be nk" in ctx.lib.hmg_last_error()
    assert native(F=17) != 0 and b"HMG_CIB_FMAX" in ctx.lib.hmg_last_error()
    hod = (nat.Tracer * 1)(nat.Tracer(nat.TRACER_HOD, d_u.ptr))
    d_k = ctx.upload_int32(np.array([0, 3], dtype=np.int32))
    assert native(NP=1, partners=hod, d_k=d_k, X1h=X) != 0 and b"matter or a pressure tracer" in ctx.lib.hmg_last_error()
    pres = (nat.Tracer * 1)(nat.Tracer(nat.TRACER_PRESSURE, d_y.ptr))
    assert native(NP=1, partners=pres, d_k=d_k, X1h=X) == 0
    assert native(NP=3, partners=pres, d_k=d_k, X1h=X) != 0 and b"NP must be 0, 1 or 2" in ctx.lib.hmg_last_error()
    par = (nat.C.c_double * 11)(*[P[k] for k in cib.PARAMETERS], X0)
    d_n, d_c, (tt, ww) = ctx.upload(NUS), ctx.upload(chis(h)), hm.sub_rule(16)
    d_t, d_w, Lc, Ls = ctx.upload(tt), ctx.upload(ww), ctx.empty((5, 3, NM)), ctx.empty((5, 3, NM))
    rc = ctx.lib.hmg_cib_luminosity(ctx.handle, 17, 3, NM, 16, d_n.ptr, h._d_zs().ptr, h._d_ms().ptr, d_c.ptr, None, d_t.ptr,
                                    d_w.ptr, par, Lc.ptr, Ls.ptr)
    assert rc != 0 and b"HMG_CIB_FMAX" in ctx.lib.hmg_last_error()
    par[7] = 0.0
    rc = ctx.lib.hmg_cib_luminosity(ctx.handle, 5, 3, NM, 16, d_n.ptr, h._d_zs().ptr, h._d_ms().ptr, d_c.ptr, None, d_t.ptr,
                                    d_w.ptr, par, Lc.ptr, Ls.ptr)
    assert rc != 0 and b"must be positive" in ctx.lib.hmg_last_error()
    assert nat.ABI_VERSION == 10
