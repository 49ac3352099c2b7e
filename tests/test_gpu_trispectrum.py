"""GPU checks of the 1-halo trispectrum (HaloModel.get_trispectrum_1halo / trispectrum_device, hmg_trispectrum_1h) and of
its Limber projection hmvec_amd.cov.cl_cov_1halo; definition and gate in DESIGN.md section 15.  The reference computes no
trispectrum, so the device is compared with the numpy restatement of the definition on the model's own host tensors
(tests/helpers/trispectrum_model.py, pinned by tests/test_trispectrum_cpu.py) at the derived gate
(nm + 32) 2^-52 sum_m |terms|.

The model is the smallest on which the kernel can still go wrong: three redshifts across the HOD's z <= 0.8 split, 48
wavenumbers (one partial 64-tile), 37 masses (one full chunk of 32 and one of 5), and 70 interpolated samples (a full
tile and one of 6 in each direction).

Measured on an MI355X (worst |got - ref| / gate): node mode 4.0e-2 (n = 48) and 1.6e-2 (n = 1), 70 interpolated samples
5.7e-2 against the restatement and at most 5.9e-2 against the bilinear interpolant of the device's node result (2.9e-2
was measured against a bound up to twice the present one; not yet re-measured), exchanged spectra 0
(same bits), Tz 3.9e-2 against the restatement and 0.66 of nz 2^-53 sum|g T| against the sum of the device's own T,
cl_cov_1halo 1.6e-2, damping 0.34 of the 4 ulp."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from hmvec_amd import _native as nat
from hmvec_amd import cov

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import trispectrum_model as tm  # noqa: E402
from lensing_model import model  # noqa: E402

pytestmark = pytest.mark.gpu

NM = 37
PAIRS = [("nfw", "nfw", "nfw", "nfw"), ("g", "g", "g", "g"), ("g", "nfw", "g", "nfw"), ("y", "y", "y", "y"),
         ("g", "g", "nfw", "nfw"), ("g", "y", "nfw", "electron"), ("gc", "g", "gc", "electron"),
         ("y", "y2", "y2", "y")]          # (two pressure names: pk_y^2 against pk_y2^2, not pk_y pk_y2)


@pytest.fixture(scope="module")
def h():
    zs = np.array([0.2, 0.8, 1.4])
    m = model(zs, ks=np.geomspace(1e-3, 30, 48), ms=np.geomspace(1e11, 10 ** 15.5, NM))
    m.add_battaglia_profile("electron", family="AGN", xmax=20, nxs=512)
    m.add_battaglia_pres_profile("y", family="pres", xmax=5, nxs=512)
    m.add_battaglia_pres_profile("y2", family="pres", xmax=3, nxs=512, param_override={"battaglia_pres_gamma": -0.5})
    m.add_hod("g", mthresh=10 ** 10.5 + zs * 0.0)
    m.add_hod("gc", mthresh=10 ** 11.0 + zs * 0.0, central_profile_name="electron")
    return m


@pytest.fixture(scope="module")
def nodes(h):
    """Per pair: the device's T at all 48 nodes without damping, and the restatement's (T, A).  Shared, never changed."""
    out = {}
    for p in PAIRS:
        out[p] = (h.get_trispectrum_1halo(*p, damping=False),) + tm.trispectrum(h, *p, damping=False)
    return out


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


def within(got, ref, tol, what):
    err = np.abs(got - ref)
    worst = float(np.max(err / np.maximum(tol, 1e-300)))
    print(f"{what}: worst |T - ref| / gate = {worst:.3g}")
    return bool(np.all(err <= tol)), worst


# ---------------------------------------------------------------- 1. node mode against the restatement
def test_first_name_rule_for_two_pressure_names(h, nodes):
    """(y, y2) integrates pk_y^2 and (y2, y) pk_y2^2: neither is the product pk_y pk_y2, and the device follows."""
    got, ref, A = nodes[("y", "y2", "y2", "y")]
    w = tm.trapz_weights(h.ms)[None, :] * h.nzm
    product = h.pk_profiles["y"] * h.pk_profiles["y2"]
    other = np.einsum("zm,zmi,zmj->zij", w, product, product)
    assert np.any(np.abs(ref - other) > 100 * tm.gate(A, NM))           # off the diagonal the rules differ by far more than the gate
    assert np.all(np.abs(got - ref) <= tm.gate(A, NM))
    assert np.array_equal(got, h.get_trispectrum_1halo("y", "y", "y2", "y2", damping=False))     # same square terms


@pytest.mark.parametrize("pair", PAIRS)
def test_nodes_against_the_restatement(h, nodes, pair):
    got, ref, A = nodes[pair]
    assert got.shape == (3, 48, 48) and np.all(np.isfinite(got)) and np.any(got != 0)
    ok, worst = within(got, ref, tm.gate(A, NM), f"{pair} n = 48")
    assert ok, worst
    one = h.get_trispectrum_1halo(*pair, kindex=np.array([17]), damping=False)
    assert one.shape == (3, 1, 1)
    ok, worst = within(one, ref[:, 17:18, 17:18], tm.gate(A[:, 17:18, 17:18], NM), f"{pair} n = 1")
    assert ok, worst


# ---------------------------------------------------------------- 2. interpolated samples, full and partial tiles
@pytest.mark.parametrize("pair", [("g", "nfw", "g", "nfw"), ("g", "y", "nfw", "electron")])
def test_interpolated_samples(h, nodes, tables70, pair):
    idx, frac, scale = tables70
    got = h.trispectrum_device(*pair, idx=idx, frac=frac, scale=scale, damping=False)[0].numpy()
    ref, A = tm.trispectrum(h, *pair, idx=idx, frac=frac, scale=scale, damping=False)
    assert got.shape == (3, 70, 70)
    assert np.all(got[:, 13, :] == 0) and np.all(got[:, :, 13] == 0) and np.all(got[2, 69] == 0)     # zero scale
    ok, worst = within(got, ref, tm.gate(A, NM), f"{pair} n = 70")
    assert ok, worst
    # T at interpolated samples is the bilinear interpolant of T at the nodes, exactly so for the exact sums.  Each
    # device result is within half its gate of its exact sum and the sample's A is at most the corners' A combined with
    # the interpolation weights (`bound`), so the difference is at most the gate at the four corners - plus the
    # roundings of the numpy combination below: per corner three for the weight, one for the product, and the three
    # additions, no more than 8 2^-53 of `bound`.
    Tn, _, An = nodes[pair]
    z = np.arange(3)[:, None, None]
    up = np.minimum(idx + 1, 47)
    want, bound = np.zeros_like(got), np.zeros_like(got)
    for ci, wi in ((idx, 1.0 - frac), (up, frac)):
        for cj, wj in ((idx, 1.0 - frac), (up, frac)):
            w = (scale * wi)[:, :, None] * (scale * wj)[:, None, :]
            want += w * Tn[z, ci[:, :, None], cj[:, None, :]]
            bound += np.abs(w) * An[z, ci[:, :, None], cj[:, None, :]]
    ok, worst = within(got, want, tm.gate(bound, NM) + 4 * tm.EPS * bound, f"{pair} bilinear")
    assert ok, worst


# ---------------------------------------------------------------- 3. symmetry
def test_symmetry(h, nodes, tables70):
    for pair in (("nfw", "nfw", "nfw", "nfw"), ("g", "g", "g", "g"), ("g", "nfw", "g", "nfw"), ("y", "y", "y", "y")):
        T = nodes[pair][0]
        assert np.array_equal(T, T.transpose(0, 2, 1)), pair
    idx, frac, scale = tables70
    T = h.trispectrum_device("g", "nfw", idx=idx, frac=frac, scale=scale)[0].numpy()
    assert np.array_equal(T, T.transpose(0, 2, 1))
    # the two spectra exchanged: the transpose, within the gate (the weight multiplies the product of the two
    # sides, so it is in fact the same bits)
    a = h.trispectrum_device("g", "y", "nfw", "electron", idx=idx, frac=frac, scale=scale)[0].numpy()
    b = h.trispectrum_device("nfw", "electron", "g", "y", idx=idx, frac=frac, scale=scale)[0].numpy()
    _, A = tm.trispectrum(h, "g", "y", "nfw", "electron", idx=idx, frac=frac, scale=scale)
    ok, worst = within(a, b.transpose(0, 2, 1), tm.gate(A, NM), "exchanged spectra")
    assert ok, worst
    assert np.array_equal(a, b.transpose(0, 2, 1))
    assert not np.array_equal(a, a.transpose(0, 2, 1))


# ---------------------------------------------------------------- 4. independence and determinism
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


def test_determinism_and_independence(h, nodes, tables70):
    pair = ("gc", "g", "gc", "electron")
    T = nodes[pair][0]
    assert np.array_equal(h.get_trispectrum_1halo(*pair, damping=False), T)                      # repeat
    sub = np.array([3, 17, 18, 40, 47])
    assert np.array_equal(h.get_trispectrum_1halo(*pair, kindex=sub, damping=False), T[:, sub][:, :, sub])
    idx, frac, scale = tables70
    full = h.trispectrum_device(*pair, idx=idx, frac=frac, scale=scale, damping=False)[0].numpy()
    part = h.trispectrum_device(*pair, idx=idx[:, 60:], frac=frac[:, 60:], scale=scale[:, 60:], damping=False)[0].numpy()
    assert np.array_equal(part, full[:, 60:, 60:])               # samples that sat in two tiles, alone in one
    # one redshift alone: the entry point on that redshift's slices of every array
    nz, nm, nk, n = 3, NM, 48, 70
    ctx = h._ctx()
    tr = [h._tracer(r, 1) for r in h._resolve(*pair)]
    for z in range(nz):
        tz = [shifted(t, z, nm, nk) for t in tr]
        d_idx, d_frac, d_scale = ctx.upload_int32(idx[z]), ctx.upload(frac[z]), ctx.upload(scale[z])
        out = ctx.empty((1, n, n))
        ctx.call("hmg_trispectrum_1h", 1, nm, nk, n, *(C.byref(t) for t in tz), h._d_nzm.ptr + 8 * z * nm,
                 h._d_ms().ptr, h._d_wm().ptr, h._rho_m0(), d_idx.ptr, d_frac.ptr, d_scale.ptr, None, out.ptr, None)
        assert np.array_equal(out.numpy()[0], full[z]), z


# ---------------------------------------------------------------- 5. the z sum
def test_z_sum(h, tables70):
    pair = ("g", "y", "nfw", "electron")
    idx, frac, scale = tables70
    g = np.array([0.7, -1.3, 2.1])
    T, Tz = h.trispectrum_device(*pair, idx=idx, frac=frac, scale=scale, zweights=g)
    T, Tz = T.numpy(), Tz.numpy()
    assert Tz.shape == (70, 70)
    # against the sum of the device's own per-z matrices: nz roundings of the running sum
    absum = np.einsum("z,zij->ij", np.abs(g), np.abs(T))
    exact = np.einsum("z,zij->ij", g.astype(np.longdouble), T.astype(np.longdouble))          # (no rounding of its own)
    ok, worst = within(Tz, exact.astype(np.float64), 3 * 2.0 ** -53 * absum, "Tz against sum_z g T")
    assert ok, worst
    ref, A = tm.trispectrum(h, *pair, idx=idx, frac=frac, scale=scale)
    want, tol = tm.zsum(g, ref, A, NM)
    ok, worst = within(Tz, want, tol, "Tz against the restatement")
    assert ok, worst
    # asked for alone (the per-z matrices then live in a temporary block): the same bits
    none, alone = h.trispectrum_device(*pair, idx=idx, frac=frac, scale=scale, zweights=g, per_z=False)
    assert none is None and np.array_equal(alone.numpy(), Tz)


# ---------------------------------------------------------------- 6. the Limber covariance
@pytest.mark.parametrize("pair", [("y", "y"), ("g", "nfw")])
def test_cl_cov_1halo(h, pair):
    ells = np.array([200.0, 1000.0, 3000.0])
    W = (1.0, np.array([0.5, 1.0, 0.8]), 1.0, np.array([2.0, 1.0, 0.5]))
    got = cov.cl_cov_1halo(h, ells, *pair, W1=W[0], W2=W[1], W3=W[2], W4=W[3], fsky=0.4)
    assert got.shape == (3, 3) and np.all(got > 0)
    assert np.array_equal(got, got.T)
    zs = h.zs
    chis, hzs = h.comoving_radial_distance(zs), h.h_of_z(zs)
    idx, frac = cov.limber_samples(ells, chis, h.ks)
    g = tm.trapz_weights(zs) * hzs * W[1] * W[3] / chis ** 6 / (4 * np.pi * 0.4)
    T, A = tm.trispectrum(h, *pair, idx=idx, frac=frac, damping=True)
    want, tol = tm.zsum(g, T, A, NM)
    ok, worst = within(got, want, tol + 8 * tm.EPS * np.abs(want), f"cl_cov_1halo {pair}")     # (+ the host's own g)
    assert ok, worst
    undamped = cov.cl_cov_1halo(h, ells, *pair, W1=W[0], W2=W[1], W3=W[2], W4=W[3], fsky=0.4, damping=False)
    assert np.all(undamped >= got)          # (D <= 1; exactly 1 where k is far above kstar)


# ---------------------------------------------------------------- 7. damping
def test_damping_is_a_factor_per_sample(h, nodes):
    # the scale multiplies the finished sum as the one factor D_i D_j, the sum itself has the bits of the undamped one:
    # T (D_i D_j) against (T D_i) D_j is three roundings, inside the 4 ulp
    D = 1.0 - np.exp(-(h.ks / h.p["kstar_damping"]) ** 2.0)
    for pair in (("g", "nfw", "g", "nfw"), ("nfw", "nfw", "nfw", "nfw")):
        Tu = nodes[pair][0]
        Td = h.get_trispectrum_1halo(*pair)
        want = Tu * D[None, :, None] * D[None, None, :]
        ok, worst = within(Td, want, 4 * tm.EPS * np.abs(want), f"{pair} damping (of 4 ulp)")
        assert ok, worst


# ---------------------------------------------------------------- 8. refusals, all before any launch
def test_errors(h):
    with pytest.raises(ValueError, match="kindex"):
        h.get_trispectrum_1halo("nfw", kindex=np.zeros(1025, dtype=int))
    with pytest.raises(ValueError, match="0 .. nk - 1"):
        h.get_trispectrum_1halo("nfw", kindex=np.array([0, 48]))
    with pytest.raises(ValueError, match="0 .. nk - 1"):
        h.get_trispectrum_1halo("nfw", kindex=np.array([-1, 3]))
    with pytest.raises(ValueError, match="frac = 0"):
        h.trispectrum_device("nfw", idx=np.array([47]), frac=np.array([0.5]))
    with pytest.raises(ValueError, match="ell = 200000.0"):
        cov.cl_cov_1halo(h, [500.0, 200000.0], "nfw")
    with pytest.raises(ValueError, match="ell = 0.0"):
        cov.cl_cov_1halo(h, [0.0], "nfw")
    with pytest.raises(ValueError, match="nosuch"):
        h.get_trispectrum_1halo("nosuch")
    with pytest.raises(ValueError, match="nosuch"):
        h.get_trispectrum_1halo("nfw", "nfw", "g", "nosuch")
    # the entry point itself refuses a table that would read past a row, before it reads anything through it
    ctx = h._ctx()
    t = h._tracer(h._resolve("nfw")[0], 1)
    d_idx, d_f, d_s, out = ctx.upload_int32(np.array([47, 0, 0])), ctx.upload(np.array([0.5])), ctx.upload(np.ones(1)), ctx.empty((3,))
    with pytest.raises(nat.NativeError, match="nk-1"):
        ctx.call("hmg_trispectrum_1h", 3, NM, 48, 1, *(C.byref(t),) * 4, h._d_nzm.ptr, h._d_ms().ptr, h._d_wm().ptr,
                 h._rho_m0(), d_idx.ptr, ctx.upload(np.array([0.5, 0.0, 0.0])).ptr, ctx.upload(np.ones(3)).ptr, None,
                 out.ptr, None)
    with pytest.raises(nat.NativeError, match="no output"):
        ctx.call("hmg_trispectrum_1h", 3, NM, 48, 1, *(C.byref(t),) * 4, h._d_nzm.ptr, h._d_ms().ptr, h._d_wm().ptr,
                 h._rho_m0(), d_idx.ptr, d_f.ptr, d_s.ptr, None, None, None)
    with pytest.raises(nat.NativeError, match="d_zweights"):
        ctx.call("hmg_trispectrum_1h", 3, NM, 48, 1, *(C.byref(t),) * 4, h._d_nzm.ptr, h._d_ms().ptr, h._d_wm().ptr,
                 h._rho_m0(), d_idx.ptr, d_f.ptr, d_s.ptr, None, None, out.ptr)
    with pytest.raises(nat.NativeError, match="no sample"):
        ctx.call("hmg_trispectrum_1h", 3, NM, 48, 0, *(C.byref(t),) * 4, h._d_nzm.ptr, h._d_ms().ptr, h._d_wm().ptr,
                 h._rho_m0(), d_idx.ptr, d_f.ptr, d_s.ptr, None, out.ptr, None)
