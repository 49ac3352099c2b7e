"""GPU checks of the 2-, 3- and 4-halo terms of the trispectrum (hmvec_amd.connected: connected_trispectrum_device /
get_trispectrum / pt_averages_device / cl_cov_connected; hmg_trispectrum_connected, hmg_pt_averages); contract and gates
in DESIGN.md section 31.  The reference has no trispectrum, so the device is compared with the numpy restatement of the
contract on the model's own host tensors (tests/helpers/connected_model.py, pinned by tests/test_connected_cpu.py and,
below, against its 40-digit evaluator on this model), every quantity at its derived tol; no element is left out.

The model is section 15's with 65 masses: three redshifts across the HOD's z <= 0.8 split, 48 wavenumbers.  The mass
contraction stages 16 masses at a time and owns 32 x 32 tiles: masses 1, 31, 32, 33, 65 (the first masses of one
redshift, through the entry point itself) are one short chunk, one short of two, exactly two, two and one, four and
one; samples 1, 2, 63, 64, 65, 130 are one partial tile, two tiles less one, exactly two, two and one, four and a bit.
The PT kernel owns 256 pairs per workgroup: 130 samples are 8515 pairs, 33 full workgroups and a partial one.

The constants of the device's log and exp inside plin_at (connected_model.C_LOG, C_EXP) are 4 x the worst error the
math probe measures on the device against mpmath (tests/test_gpu_math_probe.py: log 0.70 ulp, exp 0.81 ulp)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from hmvec_amd import _native as nat
from hmvec_amd import connected as cn
from hmvec_amd import cov
from hmvec_amd.quadrature import trapz_weights

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import connected_model as cm  # noqa: E402
import trispectrum_model as tm  # noqa: E402
from lensing_model import model  # noqa: E402

pytestmark = pytest.mark.gpu

NZ, NM, NK = 3, 65, 48
QUADS = [("nfw", "nfw", "nfw", "nfw"), ("nfw", "electron", "y", "y"), ("g", "nfw", "g", "nfw"), ("g", "g", "nfw", "nfw"),
         ("g", "g", "g", "g")]
PT = ("Pbar", "Bbar", "Tbar")


@pytest.fixture(scope="module")
def h():
    zs = np.array([0.2, 0.8, 1.4])
    m = model(zs, ks=np.geomspace(1e-3, 30, NK), ms=np.geomspace(1e11, 10 ** 15.5, NM))
    m.add_battaglia_profile("electron", family="AGN", xmax=20, nxs=512)
    m.add_battaglia_pres_profile("y", family="pres", xmax=5, nxs=512)
    m.add_hod("g", mthresh=10 ** 10.5 + zs * 0.0)
    m.add_hod("g2", mthresh=10 ** 11.0 + zs * 0.0)
    return m


@pytest.fixture(scope="module")
def tables():
    """130 samples per redshift, Limber wavenumbers of 130 multipoles in any order, with section 15's special entries
    among the first 63: the last node with f = 0, an interior node with f = 0, a fraction close to 1, a zero and a
    negative scale; sample 64 repeats sample 3."""
    rng = np.random.default_rng(31)
    ells = rng.permutation(np.geomspace(30.0, 12000.0, 130))
    idx, frac = cov.limber_samples(ells, np.array([800.0, 2800.0, 4200.0]), np.geomspace(1e-3, 30, NK))
    idx, frac = idx.astype(np.int64), frac.copy()
    scale = rng.uniform(0.5, 2.0, (NZ, 130))
    idx[:, 5], frac[:, 5] = NK - 1, 0.0
    idx[1, 60], frac[1, 60] = NK - 1, 0.0
    frac[:, 9] = 0.0
    frac[0, 11] = 1.0 - 2.0 ** -30
    scale[:, 13] = 0.0
    scale[2, 1] = 0.0
    scale[:, 21] = -1.25
    idx[:, 64], frac[:, 64], scale[:, 64] = idx[:, 3], frac[:, 3], scale[:, 3]
    assert np.any(frac != 0) and np.all((idx < NK - 1) | (frac == 0))
    return idx, frac, scale


def first(tables, n):
    return dict(idx=tables[0][:, :n], frac=tables[1][:, :n], scale=tables[2][:, :n])


def device(h, names, rule, **kw):
    T, _ = cn.connected_trispectrum_device(h, *names, rule=rule, **kw)
    return T.numpy()


def within(got, ref, what, worst=None):
    val, tol = ref
    assert got.shape == val.shape and np.all(np.isfinite(got)), what
    err = np.abs(got - val)
    ratio = float(np.max(np.where(err == 0, 0.0, err / np.maximum(tol, 1e-300))))
    print(f"{what}: worst |got - ref| / tol = {ratio:.3g}")
    if worst is not None:
        worst[what.split()[-1]] = max(worst.get(what.split()[-1], 0.0), ratio)
    assert np.all(err <= tol), (what, ratio)


def check(T, ref, what):
    for q, key in enumerate(cm.TERMS):
        within(T[q], ref[key], f"{what} {key}")


def check_pt(h, rule, idx, frac, ref, what):
    got = cn.pt_averages_device(h.ks, h._d_Pzk(), idx, frac, rule, ctx=h._ctx()).numpy()
    for q, key in enumerate(PT):
        within(got[q], ref[key], f"{what} {key}")
        assert np.array_equal(got[q], np.swapaxes(got[q], 1, 2)), key                  # bit-symmetric
    return got


# ---------------------------------------------------------------- 1. the terms and the PT matrices against the restatement
@pytest.mark.parametrize("names", QUADS)
def test_quadruples_against_the_restatement(h, tables, names):
    rule = cn.angle_rule(33, "2d")
    kw = first(tables, 65)
    for damping in (True, False):
        T = device(h, names, rule, damping=damping, **kw)
        ref = cm.connected(h, names, rule, damping=damping, **kw)
        assert T.shape == (5, NZ, 65, 65) and all(np.any(T[q] != 0) for q in range(5))
        check(T, ref, f"{names} n = 65 damping={damping}")
        zero = (kw["scale"][:, :, None] == 0) | (kw["scale"][:, None, :] == 0)
        assert zero.any() and np.all(T[:, zero] == 0) and np.all(T[4][~zero] != 0)      # a zero scale: exact zeros
    check_pt(h, rule, kw["idx"], kw["frac"], ref, f"{names} n = 65")
    for key in cm.TERMS[1:] + PT:                                                          # the gates are not vacuous
        val, tol = ref[key]
        live = val != 0
        k = ref["k"]
        squeeze = (np.maximum(k[:, :, None], k[:, None, :]) / np.minimum(k[:, :, None], k[:, None, :])) ** 2
        assert np.all(tol[live] <= 1e-10 * (squeeze * np.abs(val))[live]), key


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 130])
def test_sample_counts(h, tables, n):
    names, rule = ("g", "nfw", "g", "nfw"), cn.angle_rule(2, "3d")
    kw = first(tables, n)
    T = device(h, names, rule, **kw)
    ref = cm.connected(h, names, rule, **kw)
    assert T.shape == (5, NZ, n, n)
    check(T, ref, f"n = {n}")
    check_pt(h, rule, kw["idx"], kw["frac"], ref, f"n = {n}")


@pytest.mark.parametrize("measure", ["2d", "3d"])
@pytest.mark.parametrize("nr", [1, 2, 33])
def test_rule_sizes(h, tables, nr, measure):
    names, rule = ("nfw", "electron", "y", "y"), cn.angle_rule(nr, measure)
    kw = first(tables, 12)
    T = device(h, names, rule, **kw)
    ref = cm.connected(h, names, rule, **kw)
    check(T, ref, f"nr = {nr} {measure}")
    check_pt(h, rule, kw["idx"], kw["frac"], ref, f"nr = {nr} {measure}")
    # through the public dict: the same bits, and total is the sum in the contract's order
    out = cn.get_trispectrum(h, *names, kindex=np.array([3, 17, 47]), rule=rule)
    Tn = device(h, names, rule, kindex=np.array([3, 17, 47]))
    assert list(out) == ["1h", "2h13", "2h22", "3h", "4h", "total"]
    assert all(np.array_equal(out[k], Tn[q]) for q, k in enumerate(cn.TERMS))
    assert np.array_equal(out["total"], (((Tn[0] + Tn[1]) + Tn[2]) + Tn[3]) + Tn[4])


# ---------------------------------------------------------------- the entry point itself, on slices of the model
def shifted(t, z):
    """The hmg_tracer of redshift z alone: every pointer moved to that redshift's slice."""
    o = nat.Tracer()
    C.memmove(C.byref(o), C.byref(t), C.sizeof(nat.Tracer))
    for field, step in (("d_prof", NM * NK), ("d_cprof", NM * NK), ("d_Nc", NM), ("d_Ns", NM), ("d_NcNs", NM),
                        ("d_NsNsm1", NM), ("d_ngal", 1)):
        p = getattr(o, field)
        if p:
            setattr(o, field, p + 8 * z * step)
    return o


def native_args(h, names, rule, idx, frac, scale, scale1h=None, *, z=None, nm=NM, kstar=None, n=None, nr=None,
                zweights=None, want_T=True, want_Tz=False, tracers=None):
    """The arguments of a direct call of hmg_trispectrum_connected by name, on the whole model (z None) or on the first
    nm masses of redshift z alone: (kwargs, T, Tz, what must stay alive until the call is issued)."""
    ctx = h._ctx()
    nz = NZ if z is None else 1
    zs = slice(None) if z is None else slice(z, z + 1)
    idx, frac, scale = (np.ascontiguousarray(np.broadcast_to(a, (NZ,) + np.shape(a)[-1:])[zs]) for a in (idx, frac, scale))
    scale1h = scale if scale1h is None else np.ascontiguousarray(scale1h[zs])
    n_ = idx.shape[1] if n is None else n
    tr = tracers or [h._tracer(r, 1) for r in h._resolve(*names)]
    if z is not None:
        tr = [shifted(t, z) for t in tr]
    off = 0 if z is None else z
    d = dict(d_idx=ctx.upload_int32(idx), d_frac=ctx.upload(frac), d_scale=ctx.upload(scale), d_scale1h=ctx.upload(scale1h),
             d_mu=ctx.upload(rule.mu), d_omm=ctx.upload(rule.one_minus_mu), d_opm=ctx.upload(rule.one_plus_mu),
             d_w=ctx.upload(rule.weights), d_wm=ctx.upload(trapz_weights(h.ms[:nm])))
    d_g = ctx.upload(zweights) if zweights is not None else None
    T = ctx.empty((5, nz, max(n_, 1), max(n_, 1))) if want_T else None
    Tz = ctx.empty((5, max(n_, 1), max(n_, 1))) if want_Tz else None
    kw = dict(nz=nz, nm=nm, nk=NK, n=n_, nr=rule.nr if nr is None else nr,
              h_a=C.byref(tr[0]), h_b=C.byref(tr[1]), h_c=C.byref(tr[2]), h_d=C.byref(tr[3]),
              d_nzm=h._d_nzm.ptr + 8 * off * NM, d_bh=h._d_bh.ptr + 8 * off * NM, d_ms=h._d_ms().ptr, d_ks=h._d_ks().ptr,
              d_Pzk=h._d_Pzk().ptr + 8 * off * NK, rho_m0=h._rho_m0(),
              kstar=float(h.p["kstar_damping"]) if kstar is None else kstar, d_zweights=nat.ptr(d_g), d_T=nat.ptr(T),
              d_Tz=nat.ptr(Tz), **{k: v.ptr for k, v in d.items()})
    return kw, T, Tz, (tr, d, d_g)


def native(h, *args, **kwargs):
    """hmg_trispectrum_connected called directly (native_args): (T, Tz) as host arrays (None where not asked for)."""
    kw, T, Tz, keep = native_args(h, *args, **kwargs)
    h._ctx().call("hmg_trispectrum_connected", **kw)
    del keep
    return (None if T is None else T.numpy()), (None if Tz is None else Tz.numpy())


@pytest.mark.parametrize("nm", [1, 31, 32, 33, 65])
def test_mass_bins(h, tables, nm):
    """The first nm masses of the second redshift alone, through the entry point: every chunk edge of the contraction."""
    # (one mass has no trapezoid weight: every mass sum is zero, an HOD's bracket with them, a matter leg's is 1)
    names = ("g", "nfw", "g", "electron") if nm > 1 else ("nfw", "electron", "nfw", "nfw")
    rule, z = cn.angle_rule(2, "2d"), 1
    kw = first(tables, 33)
    v = cm.view(h, z, z + 1, nm)
    ref = cm.connected(v, names, rule, idx=kw["idx"][z:z + 1], frac=kw["frac"][z:z + 1], scale=kw["scale"][z:z + 1])
    s1 = tm.tables(v, idx=kw["idx"][z:z + 1], frac=kw["frac"][z:z + 1], scale=kw["scale"][z:z + 1], damping=True)[2]
    T, _ = native(h, names, rule, kw["idx"], kw["frac"], kw["scale"], np.broadcast_to(s1, (NZ, 33)), z=z, nm=nm)
    assert T.shape == (5, 1, 33, 33)
    check(T, ref, f"nm = {nm}")
    if nm == 1:
        live = kw["scale"][z][:, None] * kw["scale"][z][None, :] != 0
        assert np.all(T[:4] == 0) and np.all(T[4, 0][live] != 0) and np.all(T[4, 0][~live] == 0)
    else:
        assert all(np.any(T[q] != 0) for q in range(5))


# ---------------------------------------------------------------- 2. the restatement against 40 digits, on this model
@pytest.mark.parametrize("names", [("g", "nfw", "g", "nfw"), ("nfw", "electron", "y", "y")])
def test_restatement_against_mpmath_on_the_model(h, tables, names):
    rule = cn.angle_rule(9, "2d")
    kw = first(tables, 12)
    ref = cm.connected(h, names, rule, **kw)
    worst = {}
    for z, i, j in ((0, 0, 0), (0, 5, 9), (1, 11, 3), (2, 7, 7), (1, 9, 5)):
        exact = cm.mp_element(h, names, rule, z, i, j, kw["idx"], kw["frac"], kw["scale"])
        for key in cm.TERMS + PT:
            err, tol = cm.mp_err(ref[key][0][z, i, j], exact[key]), ref[key][1][z, i, j]
            worst[key] = max(worst.get(key, 0.0), err / tol if tol > 0 else float(err > 0) * np.inf)
            assert err <= tol, (key, z, i, j, err, tol)
    print(f"{names}: worst |restatement - mpmath| / tol: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))


# ---------------------------------------------------------------- 3. bit-identities
def test_bit_identities(h, tables):
    names, rule = ("g", "nfw", "y", "electron"), cn.angle_rule(2, "3d")
    kw = first(tables, 130)
    full = device(h, names, rule, **kw)
    assert np.array_equal(device(h, names, rule, **kw), full)                                        # a repeat
    T1, _ = h.trispectrum_device(*names, **kw)
    assert np.array_equal(full[0], T1.numpy())                                                         # T1h is section 15's
    und = device(h, names, rule, damping=False, **kw)
    T1u, _ = h.trispectrum_device(*names, damping=False, **kw)
    assert np.array_equal(und[0], T1u.numpy())
    sub = np.array([0, 3, 31, 32, 64, 65, 97, 129])                                                   # from every tile, alone in one
    part = device(h, names, rule, idx=kw["idx"][:, sub], frac=kw["frac"][:, sub], scale=kw["scale"][:, sub])
    assert np.array_equal(part, full[:, :, sub][:, :, :, sub])
    assert np.array_equal(full[:, :, 64, :], full[:, :, 3, :]) and np.array_equal(full[:, :, :, 64], full[:, :, :, 3])
    # one redshift alone
    s1 = tm.tables(h, damping=True, **kw)[2]
    for z in range(NZ):
        Tz_, _ = native(h, names, rule, kw["idx"], kw["frac"], kw["scale"], s1, z=z)
        assert np.array_equal(Tz_[:, 0], full[:, z]), z
    # damping=False is kstar <= 0
    for kstar in (0.0, -1.0):
        Tk, _ = native(h, names, rule, kw["idx"], kw["frac"], kw["scale"], kw["scale"], kstar=kstar)
        assert np.array_equal(Tk, und)
    # the PT matrices: device input against host input, and under an exchange of the samples
    a = cn.pt_averages_device(h.ks, h._d_Pzk(), kw["idx"], kw["frac"], rule, ctx=h._ctx()).numpy()
    b = cn.pt_averages_device(h.ks, h.Pzk, kw["idx"], kw["frac"], rule, ctx=h._ctx()).numpy()
    assert np.array_equal(a, b)
    perm = np.random.default_rng(3).permutation(130)
    c = cn.pt_averages_device(h.ks, h.Pzk, kw["idx"][:, perm], kw["frac"][:, perm], rule, ctx=h._ctx()).numpy()
    assert np.array_equal(c, a[:, :, perm][:, :, :, perm])
    # the z sum: the device's own per-z planes, z in order, and asked for alone
    g = np.array([0.7, -1.3, 2.1])
    T, Tz = cn.connected_trispectrum_device(h, *names, rule=rule, zweights=g, **kw)
    assert np.array_equal(T.numpy(), full)
    want = np.zeros((5, 130, 130))
    for z in range(NZ):
        want = want + g[z] * full[:, z].astype(np.longdouble)
    absum = np.einsum("z,qzij->qij", np.abs(g), np.abs(full))
    assert np.all(np.abs(Tz.numpy() - want.astype(np.float64)) <= 3 * 2.0 ** -53 * absum)
    none, alone = cn.connected_trispectrum_device(h, *names, rule=rule, zweights=g, per_z=False, **kw)
    assert none is None and np.array_equal(alone.numpy(), Tz.numpy())


def test_exchange_of_the_two_spectra(h, tables):
    """T^{ab,cd}[z,i,j] against T^{cd,ab}[z,j,i]: within the gate (T1h and the PT matrices: the same bits)."""
    rule = cn.angle_rule(2, "2d")
    kw = first(tables, 40)
    for names in (("g", "nfw", "y", "electron"), ("g", "g", "nfw", "y")):
        one = device(h, names, rule, **kw)
        two = np.swapaxes(device(h, names[2:] + names[:2], rule, **kw), 2, 3)
        ref = cm.connected(h, names, rule, **kw)
        assert np.array_equal(one[0], two[0])
        for q, key in enumerate(cm.TERMS):
            within(two[q], (one[q], ref[key][1]), f"{names} exchanged {key}")


# ---------------------------------------------------------------- 4. the Limber matrix
@pytest.mark.parametrize("names", [("nfw", "nfw", "nfw", "nfw"), ("g", "nfw", "y", "y")])
def test_cl_cov_connected(h, names):
    ells = np.array([60.0, 200.0, 700.0, 701.0, 3000.0, 9000.0])
    W = (np.array([0.5, 1.0, 0.8]), 1.5, np.array([2.0, 1.0, 0.5]), 1.0)
    rule = cn.angle_rule(8, "2d")
    out = cn.cl_cov_connected(h, ells, *names, W1=W[0], W2=W[1], W3=W[2], W4=W[3], fsky=0.3, rule=rule)
    idx, frac, g = cn.limber_tables(h, ells, *W, fsky=0.3)
    ref = cm.connected(h, names, rule, idx=idx, frac=frac)
    z = {key: cm.zsum(g, ref[key]) for key in cm.TERMS}
    one = cov.cl_cov_1halo(h, ells, *names, W1=W[0], W2=W[1], W3=W[2], W4=W[3], fsky=0.3)
    assert np.array_equal(out["1h"], one)                                                # exactly cl_cov_1halo's
    within(out["1h"], z["T1h"], "cl_cov_connected 1h")
    within(out["2h"], cm.add(z["T2h13"], z["T2h22"]), "cl_cov_connected 2h")
    within(out["3h"], z["T3h"], "cl_cov_connected 3h")
    within(out["4h"], z["T4h"], "cl_cov_connected 4h")
    assert np.array_equal(out["total"], ((out["1h"] + out["2h"]) + out["3h"]) + out["4h"])
    assert all(v.shape == (6, 6) and np.all(v != 0) for v in out.values())
    default = cn.cl_cov_connected(h, ells[:2], *names)                                   # the default rule: 32 nodes, "2d"
    again = cn.cl_cov_connected(h, ells[:2], *names, rule=cn.angle_rule(32, "2d"))
    assert all(np.array_equal(default[k], again[k]) for k in default)


# ---------------------------------------------------------------- 5. refusals from the native layer
def test_native_refusals(h, tables):
    names, rule = ("nfw", "nfw", "nfw", "nfw"), cn.angle_rule(2, "2d")
    idx, frac, scale = (a[:, :2] for a in tables)
    good, _ = native(h, names, rule, idx, frac, scale)
    assert np.all(np.isfinite(good))
    big = cn.angle_rule(256, "2d")
    with pytest.raises(nat.NativeError, match="no sample"):
        native(h, names, rule, idx, frac, scale, n=0)
    with pytest.raises(nat.NativeError, match="256 samples"):
        native(h, names, rule, idx, frac, scale, n=257)
    with pytest.raises(nat.NativeError, match="no rule nodes"):
        native(h, names, rule, idx, frac, scale, nr=0)
    with pytest.raises(nat.NativeError, match="256 rule nodes"):
        native(h, names, big, idx, frac, scale, nr=257)
    with pytest.raises(nat.NativeError, match="no output"):
        native(h, names, rule, idx, frac, scale, want_T=False)
    with pytest.raises(nat.NativeError, match="d_zweights"):
        native(h, names, rule, idx, frac, scale, want_T=False, want_Tz=True)
    tr = [h._tracer(r, 1) for r in h._resolve("g", "nfw", "g2", "nfw")]
    with pytest.raises(nat.NativeError, match="two different HOD tracers"):
        native(h, names, rule, idx, frac, scale, tracers=tr)
    bad = idx.copy()
    bad[1, 1] = NK
    with pytest.raises(nat.NativeError, match="nk-1"):
        native(h, names, rule, bad, frac, scale)
    bad = idx.copy()
    bad[2, 0] = NK - 1
    with pytest.raises(nat.NativeError, match="nk-1"):
        native(h, names, rule, bad, np.full(frac.shape, 0.5), scale)
    ctx = h._ctx()
    d = [ctx.upload(a) for a in (rule.mu, rule.one_minus_mu, rule.one_plus_mu, rule.weights)]
    d_idx, d_frac, out = ctx.upload_int32(idx), ctx.upload(frac), ctx.empty((3, NZ, 2, 2))

    def pt(n=2, nr=2, nk=NK, d_idx=d_idx):
        ctx.call("hmg_pt_averages", NZ, nk, n, nr, h._d_ks().ptr, h._d_Pzk().ptr, d_idx.ptr, d_frac.ptr, *(a.ptr for a in d),
                 out.ptr, out.ptr + 8 * NZ * 4, out.ptr + 16 * NZ * 4)
    pt()
    for kw, match in ((dict(n=0), "no sample"), (dict(n=257), "256 samples"), (dict(nr=0), "no rule nodes"),
                      (dict(nr=257), "256 rule nodes"), (dict(nk=1), "two wavenumbers"),
                      (dict(d_idx=ctx.upload_int32(np.full((NZ, 2), -1))), "nk-1")):
        with pytest.raises(nat.NativeError, match=match):
            pt(**kw)
    # a captured step is refused before anything is enqueued or read (a context of its own: nothing of the model's is
    # queued in it; the arguments are never dereferenced)
    kw, _, _, keep = native_args(h, names, rule, idx, frac, scale)
    ctx2 = nat.Context(0)

    def body():
        with pytest.raises(nat.NativeError, match="captured step"):
            ctx2.call("hmg_trispectrum_connected", **kw)
        with pytest.raises(nat.NativeError, match="captured step"):
            ctx2.call("hmg_pt_averages", NZ, NK, 2, 2, h._d_ks().ptr, h._d_Pzk().ptr, d_idx.ptr, d_frac.ptr, *(a.ptr for a in d),
                      out.ptr, out.ptr + 8 * NZ * 4, out.ptr + 16 * NZ * 4)

    gid = ctx2.capture(body)
    ctx2.call("hmg_graph_destroy", gid)
    ctx2.close()
    del keep
    again, _ = native(h, names, rule, idx, frac, scale)
    assert np.array_equal(again, good)
