"""GPU checks of the response of halo-model spectra to a long-wavelength mode (HaloModel.response_device /
get_power_response, hmg_response), of the super-sample contraction (ssc_device, hmg_ssc) and of its Limber projection
hmvec_amd.cov.cl_cov_ssc; definition and gates in DESIGN.md section 17.  The reference computes no response, so the
device is compared with the numpy restatement of the definition on the model's own host tensors
(tests/helpers/response_model.py, pinned by tests/test_response_cpu.py) at its derived, propagated tols.

The model is section 15's: three redshifts across the HOD's z <= 0.8 split, 48 wavenumbers, 37 masses, and 70
interpolated samples; five pairs of 70 samples are 350 rows of the contraction: five full 64-tiles and one of 30.

Measured on an MI355X (worst |got - ref| / tol): node mode A1 0.031, I1 0.029, P2h 0.020, R 0.025; n = 1 at most 0.018;
70 interpolated samples A1 0.033, I1 0.025, P2h 0.032, R 0.032; undamped at most 0.025; A1 D against get_power_1halo at
most 0.018 of twice the tol, P2h against get_power_2halo at most 0.015 of it; Cov 0.026, with zscale 0.030, 0.76 of
5 2^-53 sum|g r r| against the sum of the device's own responses, np = 1, n = 1 0.0008; cl_cov_ssc 0.0080 (sigma_b given)
and 0.012 (from fsky).  Non-vacuity: the tol of R is <= 1e-10 |R| on every entry of the three positive pairs, its median
between 1.9e-14 and 3.3e-14 of |R|."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from hmvec_amd import _native as nat
from hmvec_amd import bispectrum as bs
from hmvec_amd import cov
from hmvec_amd.quadrature import trapz_weights

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import response_model as rm  # noqa: E402
from lensing_model import model  # noqa: E402

pytestmark = pytest.mark.gpu

NM, NK = 37, 48
PAIRS = [("nfw", "nfw"), ("g", "g"), ("g", "nfw"), ("y", "y"), ("nfw", "y"), ("g", "y"), ("gc", "electron"),
         ("y", "y2"), ("g", "gc")]
NON_VACUOUS = [("nfw", "nfw"), ("nfw", "y"), ("y", "y")]
SSC_PAIRS = [("nfw", "nfw"), ("g", "nfw"), ("y", "y"), ("g", "gc"), ("nfw", "y")]


@pytest.fixture(scope="module")
def h():
    zs = np.array([0.2, 0.8, 1.4])
    m = model(zs, ks=np.geomspace(1e-3, 30, NK), ms=np.geomspace(1e11, 10 ** 15.5, NM))
    m.add_battaglia_profile("electron", family="AGN", xmax=20, nxs=512)
    m.add_battaglia_pres_profile("y", family="pres", xmax=5, nxs=512)
    m.add_battaglia_pres_profile("y2", family="pres", xmax=3, nxs=512, param_override={"battaglia_pres_gamma": -0.5})
    m.add_hod("g", mthresh=10 ** 10.5 + zs * 0.0)
    m.add_hod("gc", mthresh=10 ** 11.0 + zs * 0.0, central_profile_name="electron")
    return m


@pytest.fixture(scope="module")
def tables70():
    """70 Limber-style samples per redshift: left nodes and fractions all over the grid, among them the last node with
    f = 0, an interior node with f = 0, a fraction close to 1 and a zero scale."""
    rng = np.random.default_rng(11)
    idx = rng.integers(0, 47, (3, 70))
    frac = rng.uniform(0.0, 1.0, (3, 70))
    scale = rng.uniform(0.5, 2.0, (3, 70))
    idx[:, 5], frac[:, 5] = 47, 0.0
    idx[1, 64], frac[1, 64] = 47, 0.0
    frac[:, 9] = 0.0
    frac[0, 66] = 1.0 - 2.0 ** -30
    scale[:, 13] = 0.0
    scale[2, 69] = 0.0
    return idx, frac, scale


def device(h, pairs, **kw):
    R, parts = h.response_device(pairs, parts=True, **kw)
    return R.numpy(), parts.numpy()


@pytest.fixture(scope="module")
def nodes(h):
    """All pairs at the 48 nodes, damped: the device's (R, parts) and the restatement.  Shared, never changed."""
    return device(h, PAIRS) + (rm.response(h, PAIRS),)


@pytest.fixture(scope="module")
def samples70(h, tables70):
    idx, frac, scale = tables70
    return device(h, PAIRS, idx=idx, frac=frac, scale=scale) + (rm.response(h, PAIRS, idx=idx, frac=frac, scale=scale),)


def within(got, ref, tol, what):
    err = np.abs(got - ref)
    worst = float(np.max(err / np.maximum(tol, 1e-300)))
    print(f"{what}: worst |got - ref| / tol = {worst:.3g}")
    return bool(np.all(err <= tol)), worst


def check(got, parts, ref, what):
    assert np.all(np.isfinite(got)) and np.all(np.isfinite(parts))
    for i, key in enumerate(("A1", "I1", "P2h")):
        ok, worst = within(parts[i], *ref[key], f"{what} {key}")
        assert ok, (key, worst)
    ok, worst = within(got, *ref["R"], f"{what} R")
    assert ok, worst


# ---------------------------------------------------------------- 1. against the restatement
def test_the_gate_is_not_vacuous(h, nodes, samples70):
    """From the restatement alone: for the pairs whose R has positive terms only, its tol is a small fraction of it."""
    for ref, what in ((nodes[2], "nodes"), (samples70[2], "n = 70")):
        for pair in NON_VACUOUS:
            p = PAIRS.index(pair)
            val, tol = ref["R"][0][p], ref["R"][1][p]
            share = float(np.mean(tol <= 1e-10 * np.abs(val)))
            print(f"{pair} {what}: tol <= 1e-10 |R| on {share:.3f} of the entries, median tol / |R| = "
                  f"{np.median(tol[val != 0] / np.abs(val[val != 0])):.3g}")
            assert share >= 0.95, (pair, what, share)
            assert np.all(ref["beta_sum"][0][p] == 0.0) and np.all(ref["ns"][0] <= 1.0)
            live = ref["scale"] != 0.0
            assert np.all(val[live] > 0.0)


def test_nodes_against_the_restatement(h, nodes):
    got, parts, ref = nodes
    assert got.shape == (len(PAIRS), 3, NK) and parts.shape == (3, len(PAIRS), 3, NK)
    check(got, parts, ref, "n = 48")
    assert np.all(got != 0)


def test_one_sample(h, nodes):
    _, _, ref = nodes
    got, parts = device(h, PAIRS, kindex=np.array([17]))
    assert got.shape == (len(PAIRS), 3, 1)
    one = rm.response(h, PAIRS, kindex=np.array([17]))
    check(got, parts, one, "n = 1")
    assert np.all(np.abs(one["R"][0][:, :, 0] - ref["R"][0][:, :, 17]) <= ref["R"][1][:, :, 17])     # (numpy's sums reorder)
    assert np.array_equal(h.get_power_response("g", "nfw", kindex=np.array([17])), got[PAIRS.index(("g", "nfw"))])


def test_interpolated_samples(h, samples70, tables70):
    got, parts, ref = samples70
    scale = tables70[2]
    assert got.shape == (len(PAIRS), 3, 70)
    check(got, parts, ref, "n = 70")
    assert np.all(got[:, scale == 0.0] == 0.0) and np.all(got[:, scale != 0.0] != 0.0)      # a zero scale: an exact zero
    assert np.all(parts[0][:, scale == 0.0] != 0.0)                                           # (the parts are unscaled)


def test_undamped(h, tables70):
    idx, frac, scale = tables70
    pairs = [("g", "gc"), ("nfw", "y")]
    got, parts = device(h, pairs, idx=idx, frac=frac, scale=scale, damping=False)
    check(got, parts, rm.response(h, pairs, idx=idx, frac=frac, scale=scale, damping=False), "undamped n = 70")


# ---------------------------------------------------------------- 2. the parts against existing code
@pytest.mark.parametrize("pair", PAIRS)
def test_parts_against_the_power_spectra(h, nodes, pair):
    """A1 D is the damped P_1h and P2h the P_2h the model returns - other kernels, other summation orders: each side is
    within the tol of the restatement's exact sum, so they agree within twice the tol."""
    _, parts, ref = nodes
    p = PAIRS.index(pair)
    D = ref["D"]
    assert np.array_equal(D, np.broadcast_to(bs.damping(h.ks, h.p["kstar_damping"]), D.shape))
    tolA, tolP = ref["A1"][1][p], ref["P2h"][1][p]
    ok, worst = within(parts[0][p] * D, h.get_power_1halo(*pair), 2 * (tolA * D + rm.EPS * np.abs(parts[0][p] * D)),
                       f"{pair} A1 D against get_power_1halo (of twice the tol)")
    assert ok, worst
    ok, worst = within(parts[2][p], h.get_power_2halo(*pair), 2 * tolP, f"{pair} P2h against get_power_2halo (of twice the tol)")
    assert ok, worst


def test_first_name_rule_for_two_pressure_names(h, nodes):
    got, _, ref = nodes
    a, = device(h, [("y", "y2")])[0]
    b, = device(h, [("y2", "y")])[0]
    tol = ref["R"][1][PAIRS.index(("y", "y2"))]
    assert np.all(np.abs(a - b) > 100 * tol)
    want = rm.response(h, [("y", "y2"), ("y2", "y")])["R"]
    assert np.all(np.abs(a - want[0][0]) <= want[1][0]) and np.all(np.abs(b - want[0][1]) <= want[1][1])
    # the 1-halo parts are the first name's alone; the 2-halo term takes each leg under its own name
    pa = device(h, [("y", "y2"), ("y", "y")])[1]
    assert np.array_equal(pa[0][0], pa[0][1]) and np.array_equal(pa[1][0], pa[1][1]) and np.all(pa[2][0] != pa[2][1])


# ---------------------------------------------------------------- 3. independence and determinism
def shifted(t, z, nm, nk):
    """The hmg_tracer of redshift z alone: every pointer moved to that redshift's slice."""
    o = nat.Tracer()
    C.memmove(C.byref(o), C.byref(t), C.sizeof(nat.Tracer))
    for field, step in (("d_prof", nm * nk), ("d_cprof", nm * nk), ("d_Nc", nm), ("d_Ns", nm), ("d_NcNs", nm),
                        ("d_NsNsm1", nm), ("d_ngal", 1)):
        p = getattr(o, field)
        if p:
            setattr(o, field, p + 8 * z * step)
    return o


def test_determinism_and_independence(h, samples70, tables70):
    full, fparts, _ = samples70
    idx, frac, scale = tables70
    again, aparts = device(h, PAIRS, idx=idx, frac=frac, scale=scale)
    assert np.array_equal(again, full) and np.array_equal(aparts, fparts)                       # repeat
    for p in (1, 6, 8):                                                                       # a pair alone
        alone, aparts = device(h, [PAIRS[p]], idx=idx, frac=frac, scale=scale)
        assert np.array_equal(alone[0], full[p]) and np.array_equal(aparts[:, 0], fparts[:, p]), PAIRS[p]
    sub = np.array([0, 5, 13, 63, 64, 66, 69])                                                # a subset of the samples alone
    part, pparts = device(h, PAIRS, idx=idx[:, sub], frac=frac[:, sub], scale=scale[:, sub])
    assert np.array_equal(part, full[:, :, sub]) and np.array_equal(pparts, fparts[:, :, :, sub])
    # one redshift alone: the entry point on that redshift's slices of every array
    pairs = [("gc", "electron"), ("g", "y"), ("g", "g")]
    rows = [PAIRS.index(p) for p in pairs]
    ctx = h._ctx()
    recs = h._resolve(*[nm_ for p in pairs for nm_ in p])
    tr = [h._tracer(r, 1) for r in recs]
    d_dlnP = ctx.upload(cov.dlnp_table(h.ks, h.Pzk))
    for z in range(3):
        tz = (nat.Tracer * len(tr))(*[shifted(t, z, NM, NK) for t in tr])
        d_idx, d_frac, d_scale = ctx.upload_int32(idx[z]), ctx.upload(frac[z]), ctx.upload(scale[z])
        out, outp = ctx.empty((3, 1, 70)), ctx.empty((3, 3, 1, 70))
        ctx.call("hmg_response", 1, NM, NK, 70, 3, tz, h._d_nzm.ptr + 8 * z * NM, h._d_bh.ptr + 8 * z * NM, h._d_ms().ptr,
                 h._d_wm().ptr, h._d_ks().ptr, h._d_Pzk().ptr + 8 * z * NK, d_dlnP.ptr + 8 * z * NK, h._rho_m0(),
                 float(h.p["kstar_damping"]), d_idx.ptr, d_frac.ptr, d_scale.ptr, out.ptr, outp.ptr)
        assert np.array_equal(out.numpy()[:, 0], full[rows, z]), z
        assert np.array_equal(outp.numpy()[:, :, 0], fparts[:, rows, z]), z


# ---------------------------------------------------------------- 4. the contraction
def test_ssc(h, tables70):
    idx, frac, scale = tables70
    g = np.array([0.7, -1.3, 2.1])
    zscale = np.random.default_rng(3).uniform(0.5, 2.0, (5, 3))
    ref = rm.response(h, SSC_PAIRS, idx=idx, frac=frac, scale=scale)
    for zs_, what in ((None, "np = 5, n = 70"), (zscale, "np = 5, n = 70, zscale")):
        got = h.ssc_device(SSC_PAIRS, g, zscale=zs_, idx=idx, frac=frac, scale=scale).numpy()
        assert got.shape == (5, 70, 5, 70) and np.all(np.isfinite(got))
        ok, worst = within(got, *rm.ssc(ref["R"], g, zs_), f"Cov {what}")
        assert ok, worst
        assert np.array_equal(got, got.transpose(2, 3, 0, 1))                                 # the same bits, no mirror pass
        assert np.all(got[:, 13] == 0) and np.all(got[:, :, :, 13] == 0)                      # zero scale
    # with zscale: the contraction of the scaled responses (the product zscale R is rounded once on either route)
    R = h.response_device(SSC_PAIRS, idx=idx, frac=frac, scale=scale)
    scaled = h._ctx().upload(zscale[:, :, None] * R.numpy())
    assert np.array_equal(h._ssc_launch(scaled, g, None).numpy(), got)
    # against the sum of the device's own responses: nz roundings of the running sum, one of each product and one of
    # the cast of the extended-precision sum below
    r = (zscale[:, :, None] * R.numpy()).transpose(0, 2, 1).reshape(350, 3).astype(np.longdouble)
    exact = np.einsum("z,az,bz->ab", g.astype(np.longdouble), r, r)
    absum = np.einsum("z,az,bz->ab", np.abs(g), np.abs(r), np.abs(r)).astype(np.float64)
    ok, worst = within(got.reshape(350, 350), exact.astype(np.float64), 5 * 2.0 ** -53 * absum,
                       "Cov against sum_z g r r of the device's R (of 5 2^-53 sum|g r r|)")
    assert ok, worst
    # np = 1, n = 1
    one = h.ssc_device([("g", "y")], g, kindex=np.array([30])).numpy()
    assert one.shape == (1, 1, 1, 1)
    ok, worst = within(one, *rm.ssc(rm.response(h, [("g", "y")], kindex=np.array([30]))["R"], g), "Cov np = 1, n = 1")
    assert ok, worst


# ---------------------------------------------------------------- 5. the Limber projection
def test_cl_cov_ssc(h):
    ells = np.array([200.0, 1000.0, 3000.0, 2500.0])
    pairs = [("nfw", "nfw"), ("g", "nfw"), ("y", "y")]
    windows = [(np.array([0.5, 1.0, 0.8]), 1.5), (1, np.array([2.0, 1.0, 0.5])), (1, 1)]
    zs = h.zs
    chis, hzs = h.comoving_radial_distance(zs), h.h_of_z(zs)
    idx, frac = cov.limber_samples(ells, chis, h.ks, zs=zs)
    ref = rm.response(h, pairs, idx=idx, frac=frac)
    zscale = np.stack([np.broadcast_to(np.asarray(a, dtype=float) * np.asarray(b, dtype=float), zs.shape) for a, b in windows])
    from hmvec_amd.cosmology import sigma2_kgrid
    kq = sigma2_kgrid(h.p["sigma2_kmin"], h.p["sigma2_kmax"], h.p["sigma2_numks"])
    for sigma_b, kw, what in ((np.array([3.0e-6, 1.0e-6, 0.4e-6]), {}, "sigma_b given"),
                              (cov.sigma_b_disc(kq, h.sPzk, chis, fsky=0.3), {"fsky": 0.3}, "sigma_b from fsky")):
        g = trapz_weights(zs) * hzs ** 3 * sigma_b / chis ** 4
        got = cov.cl_cov_ssc(h, ells, pairs, windows=windows, sigma_b=None if kw else sigma_b, **kw)
        assert got.shape == (3, 4, 3, 4) and np.all(got != 0) and np.all(sigma_b > 0)
        ok, worst = within(got, *rm.ssc(ref["R"], g, zscale), f"cl_cov_ssc, {what}")
        assert ok, worst
        assert np.array_equal(got, got.transpose(2, 3, 0, 1))
    assert np.all(np.einsum("pipi->pi", got) > 0)
    with pytest.raises(ValueError, match=r"ell = 200000\.0"):
        cov.cl_cov_ssc(h, [500.0, 200000.0], pairs, fsky=0.3)


# ---------------------------------------------------------------- 6. refusals, all before a launch
def test_errors(h):
    g = np.ones(3)
    with pytest.raises(ValueError, match="nosuch"):
        h.response_device([("nfw", "nosuch")])
    with pytest.raises(ValueError, match="nosuch"):
        h.get_power_response("nosuch")
    with pytest.raises(ValueError, match="empty"):
        h.response_device([])
    with pytest.raises(ValueError, match="at most 16"):
        h.response_device([("nfw", "nfw")] * 17)
    with pytest.raises(ValueError, match="at most 256"):
        h.response_device([("nfw", "nfw")], kindex=np.zeros(257, dtype=int))
    with pytest.raises(ValueError, match="frac = 0"):
        h.response_device([("nfw", "nfw")], idx=np.array([47]), frac=np.array([0.5]))
    with pytest.raises(ValueError, match="zweights"):
        h.ssc_device([("nfw", "nfw")], np.ones(4))
    with pytest.raises(ValueError, match="zscale"):
        h.ssc_device([("nfw", "nfw"), ("y", "y")], g, zscale=np.ones((3, 2)))
    with pytest.raises(ValueError, match="empty"):
        h.ssc_device([], g)
    with pytest.raises(ValueError, match="fsky"):
        cov.cl_cov_ssc(h, [500.0], [("nfw", "nfw")], fsky=1.5)
    with pytest.raises(ValueError, match="fsky"):
        cov.cl_cov_ssc(h, [500.0], [("nfw", "nfw")], fsky=0.0)
    with pytest.raises(ValueError, match="sigma_b"):
        cov.cl_cov_ssc(h, [500.0], [("nfw", "nfw")])
    with pytest.raises(ValueError, match="sigma_b"):
        cov.cl_cov_ssc(h, [500.0], [("nfw", "nfw")], sigma_b=np.ones(2))
    with pytest.raises(ValueError, match="windows"):
        cov.cl_cov_ssc(h, [500.0], [("nfw", "nfw")], windows=[(1, 1), (1, 1)], fsky=0.3)
    # the entry points themselves
    ctx = h._ctx()
    t = h._tracer(h._resolve("nfw")[0], 1)
    tr = (nat.Tracer * 34)(*[t] * 34)
    ones, zeros = ctx.upload(np.ones(6)), ctx.upload(np.zeros(6))
    d_idx = ctx.upload_int32(np.array([3, 4, 4, 5, 40, 41]))
    d_dlnP = ctx.upload(cov.dlnp_table(h.ks, h.Pzk))
    out = ctx.empty((17, 3, 2))

    def call(n, npairs, d_idx, d_frac, d_R):
        ctx.call("hmg_response", 3, NM, NK, n, npairs, tr, h._d_nzm.ptr, h._d_bh.ptr, h._d_ms().ptr, h._d_wm().ptr,
                 h._d_ks().ptr, h._d_Pzk().ptr, d_dlnP.ptr, h._rho_m0(), 0.01, d_idx.ptr, d_frac.ptr, ones.ptr,
                 nat.ptr(d_R), None)

    call(2, 2, d_idx, zeros, out)                                  # (good arguments; each call below has one bad one)
    with pytest.raises(nat.NativeError, match="nk-1"):
        call(2, 2, ctx.upload_int32(np.array([3, 4, 4, 3, 47, 47])), ctx.upload(np.array([0, 0, 0, 0, 0, 0.5])), out)
    with pytest.raises(nat.NativeError, match="nk-1"):
        call(2, 2, ctx.upload_int32(np.array([3, 4, 4, 3, 48, 47])), zeros, out)
    with pytest.raises(nat.NativeError, match="nk-1"):
        call(2, 2, ctx.upload_int32(np.array([3, -1, 4, 3, 4, 47])), zeros, out)
    for n, npairs, d_R, msg in ((0, 2, out, "no sample"), (257, 2, out, "256 samples"), (2, 0, out, "no pairs"),
                                (2, 17, out, "16 pairs"), (2, 2, None, "NULL"), ):
        with pytest.raises(nat.NativeError, match=msg):
            call(n, npairs, d_idx, zeros, d_R)
    covm = ctx.empty((4, 4))
    ctx.call("hmg_ssc", 3, 2, 2, out.ptr, None, ones.ptr, covm.ptr)
    for n, npairs, d_cov, msg in ((0, 2, covm, "no sample"), (257, 2, covm, "256 samples"), (2, 0, covm, "no pairs"),
                                  (2, 17, covm, "16 pairs"), (2, 2, None, "NULL")):
        with pytest.raises(nat.NativeError, match=msg):
            ctx.call("hmg_ssc", 3, n, npairs, out.ptr, None, ones.ptr, nat.ptr(d_cov))
