"""GPU checks of the redshift-space spectra of the dispersion halo model (HaloModel.rsd_device / get_power_rsd,
hmg_rsd_wedges; multipoles_device / get_power_multipoles, hmg_rsd_multipoles); definition and gates in DESIGN.md
section 19.  The reference computes nothing of the kind, so the device is compared with the numpy restatement of the
definition on the model's own host tensors (tests/helpers/rsd_model.py, pinned by tests/test_rsd_cpu.py) at its derived,
propagated tols.

The model is section 15's: three redshifts across the HOD's z <= 0.8 split, 48 wavenumbers, 37 masses; an HOD without a
central profile (g) and one with (g2).  The dispersion is the virial one with a zero column of mass bins: along a tensor
row t = (k sigma_s)^2 runs from ~ 1e-6 through the switch of the moments at 1 to > 1e4.

Measured on an MI355X (worst |got - ref| / tol over all cases): P1h 0.053, P2h 0.036, I^s 0.052, V^s 0.060, Q_n 0.084,
one-halo multipoles 0.082, two-halo multipoles 0.017; sigma_s = 0 against get_power_1halo 0.031 and, with f = 0, against
get_power_2halo 0.015 of twice the tol; the 32-node rule of the device's one-halo wedges against its closed-form
multipoles 0.025 of the bound.  Non-vacuity: the tol of both wedges and of P_0 of both terms is <= 1e-10 of the value on
every entry of ("nfw", "nfw") and ("g", "nfw"), its median between 1.2e-14 and 6.4e-14 of the value."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from hmvec_amd import _native as nat
from hmvec_amd import rsd

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import rsd_model as rs  # noqa: E402
from lensing_model import model  # noqa: E402

pytestmark = pytest.mark.gpu

NM, NK = 37, 48
ZS = np.array([0.2, 0.8, 1.4])
PAIRS = [("nfw", "nfw"), ("g", "nfw"), ("nfw", "g"), ("g", "g"), ("g", "g2"), ("g2", "g")]
NON_VACUOUS = [("nfw", "nfw"), ("g", "nfw")]
MUS9 = np.array([0.0, 0.11, 0.25, 0.4, 0.5, 0.63, 0.77, 0.9, 1.0])         # a full chunk of 8 and a partial one
SCATTERED = np.array([47, 3, 30, 0, 17, 31, 8])
WEDGE_KEYS = ("P1h", "P2h")
PART_KEYS = ("Ia", "Va", "Ib", "Vb")


def build(zs=ZS):
    m = model(zs, ks=np.geomspace(1e-3, 30, NK), ms=np.geomspace(1e11, 10 ** 15.5, NM))
    m.add_battaglia_profile("electron", family="AGN", xmax=20, nxs=512)
    m.add_battaglia_pres_profile("y", family="pres", xmax=5, nxs=512)
    m.add_hod("g", mthresh=10 ** 10.5 + zs * 0.0)
    m.add_hod("g2", mthresh=10 ** 11.0 + zs * 0.0, central_profile_name="electron")
    return m


@pytest.fixture(scope="module")
def h():
    return build()


@pytest.fixture(scope="module")
def sig(h):
    s = rsd.virial_dispersion(h)
    s[:, 5] = 0.0
    t = (h.ks.max() * s.max()) ** 2
    assert t >= 1e4 and (h.ks.min() * s[s > 0].min()) ** 2 < 1e-3, t
    return s


@pytest.fixture(scope="module")
def f(h):
    return h.get_growth_rate_f(h.zs)


def within(got, ref, tol, what):
    err = np.abs(got - ref)
    worst = float(np.max(err / np.maximum(tol, 1e-300)))
    print(f"{what}: worst |got - ref| / tol = {worst:.3g}")
    return bool(np.all(err <= tol)), worst


def check_wedges(out, parts, ref, what):
    assert np.all(np.isfinite(out))
    for i, key in enumerate(WEDGE_KEYS):
        ok, worst = within(out[i], *ref[key], f"{what} {key}")
        assert ok, (key, worst)
    if parts is not None:
        assert np.all(np.isfinite(parts))
        for i, key in enumerate(PART_KEYS):
            ok, worst = within(parts[i], *ref[key], f"{what} {key}")
            assert ok, (key, worst)


def check_multipoles(out, Q, ref, what):
    assert np.all(np.isfinite(out)) and np.all(np.isfinite(Q))
    ok, worst = within(Q, *ref["Q"], f"{what} Q_n")
    assert ok, worst
    for i, key in enumerate(WEDGE_KEYS):
        ok, worst = within(out[i], *ref[key], f"{what} multipoles of {key}")
        assert ok, (key, worst)


@pytest.fixture(scope="module")
def full(h, sig, f):
    """Every pair at the 48 nodes and the nine values of mu, damped: the device's wedges, parts, multipoles and Q, and the
    two restatements.  Shared, never changed."""
    out = {}
    for pair in PAIRS:
        w, p = h.rsd_device(*pair, mus=MUS9, sigma_s=sig, f=f, parts=True)
        m, q = h.multipoles_device(*pair, sigma_s=sig, f=f, parts=True)
        out[pair] = (w.numpy(), p.numpy(), m.numpy(), q.numpy(), rs.wedges(h, *pair, mus=MUS9, sigma_s=sig, f=f),
                     rs.multipoles(h, *pair, sigma_s=sig, f=f))
    return out


# ---------------------------------------------------------------- 1. against the restatement
def test_the_gate_is_not_vacuous(full):
    """From the restatement alone: where every term is positive the tol is a small fraction of the value."""
    for pair in NON_VACUOUS:
        _, _, _, _, wref, mref = full[pair]
        P0 = tuple(v[..., 0] for v in mref["P1h"]), tuple(v[..., 0] for v in mref["P2h"])
        for what, (val, tol) in (("P1h wedge", wref["P1h"]), ("P2h wedge", wref["P2h"]), ("P_0 1h", P0[0]), ("P_0 2h", P0[1])):
            tol = np.broadcast_to(tol, val.shape)
            share = float(np.mean(tol <= 1e-10 * np.abs(val)))
            print(f"{pair} {what}: tol <= 1e-10 |value| on {share:.3f} of the entries, median tol / |value| = "
                  f"{np.median(tol / np.abs(val)):.3g}")
            assert share >= 0.95, (pair, what, share)
            assert np.all(val > 0.0)


@pytest.mark.parametrize("pair", PAIRS)
def test_wedges_parts_and_multipoles(full, pair):
    w, p, m, q, wref, mref = full[pair]
    assert w.shape == (2, 3, NK, 9) and p.shape == (4, 3, NK, 9) and m.shape == (2, 3, NK, 3) and q.shape == (3, 3, NK)
    check_wedges(w, p, wref, f"{pair} n = 48, nmu = 9")
    check_multipoles(m, q, mref, f"{pair} n = 48")
    assert np.all(w != 0) and np.all(m[:, :, :, 0] > 0)


def test_first_name_rule(full):
    a, b = full[("g", "g2")], full[("g2", "g")]
    tol = a[4]["P1h"][1] + b[4]["P1h"][1]
    assert np.all(np.abs(a[0][0] - b[0][0]) > 100 * tol)                       # the 1-halo wedges differ ...
    assert np.all(np.abs(a[2][0, ..., 0] - b[2][0, ..., 0]) > 100 * (a[5]["P1h"][1] + b[5]["P1h"][1])[..., 0])
    assert np.array_equal(a[1][0], b[1][2]) and np.array_equal(a[1][1], b[1][3])   # ... and the legs only change places


@pytest.mark.parametrize("mus", [np.array([1.0]), np.array([0.0, 0.2, 0.5, 0.8, 1.0]),
                                 np.concatenate([[0.0], rsd.mu_rule(30)[0], [1.0]])], ids=["nmu1", "nmu5", "nmu32"])
def test_mu_counts(h, sig, f, full, mus):
    pair = ("g", "nfw")
    w, p = h.rsd_device(*pair, mus=mus, sigma_s=sig, f=f, parts=True)
    w, p = w.numpy(), p.numpy()
    assert w.shape == (2, 3, NK, mus.size)
    check_wedges(w, p, rs.wedges(h, *pair, mus=mus, sigma_s=sig, f=f), f"{pair} nmu = {mus.size}")
    # mu = 1 and mu = 0 of the nine-node call: the same bits (a result depends on its own mu alone)
    assert np.array_equal(w[..., -1], full[pair][0][..., -1])
    if mus.size > 1:
        assert np.array_equal(w[..., 0], full[pair][0][..., 0])
    if mus.size == 32:
        assert np.array_equal(h.get_power_rsd(*pair, mus=mus, sigma_s=sig, f=f)["total"], w[0] + w[1])


@pytest.mark.parametrize("kindex", [np.array([17]), SCATTERED], ids=["n1", "n7"])
def test_sample_counts(h, sig, f, full, kindex):
    for pair in (("g", "g2"), ("nfw", "nfw")):
        w, p = h.rsd_device(*pair, mus=MUS9, kindex=kindex, sigma_s=sig, f=f, parts=True)
        m, q = h.multipoles_device(*pair, kindex=kindex, sigma_s=sig, f=f, parts=True)
        w, p, m, q = w.numpy(), p.numpy(), m.numpy(), q.numpy()
        assert w.shape == (2, 3, kindex.size, 9) and m.shape == (2, 3, kindex.size, 3)
        check_wedges(w, p, rs.wedges(h, *pair, mus=MUS9, kindex=kindex, sigma_s=sig, f=f), f"{pair} n = {kindex.size}")
        check_multipoles(m, q, rs.multipoles(h, *pair, kindex=kindex, sigma_s=sig, f=f), f"{pair} n = {kindex.size}")
        # a subset of the nodes alone: the bits of the full call
        fw, fp, fm, fq = full[pair][:4]
        assert np.array_equal(w, fw[:, :, kindex]) and np.array_equal(p, fp[:, :, kindex])
        assert np.array_equal(m, fm[:, :, kindex]) and np.array_equal(q, fq[:, :, kindex])


@pytest.mark.parametrize("pair", [("g", "g2"), ("g2", "nfw"), ("g2", "g2")])
def test_velocity_factors_with_moving_centrals(h, sig, f, pair):
    alphas = (0.9, 0.6, 1.2)
    w, p = h.rsd_device(*pair, mus=MUS9, sigma_s=sig, f=f, alphas=alphas, parts=True)
    m, q = h.multipoles_device(*pair, nmu=7, sigma_s=sig, f=f, alphas=alphas, parts=True)
    check_wedges(w.numpy(), p.numpy(), rs.wedges(h, *pair, mus=MUS9, sigma_s=sig, f=f, alphas=alphas), f"{pair} alphas {alphas}")
    check_multipoles(m.numpy(), q.numpy(), rs.multipoles(h, *pair, nmu=7, sigma_s=sig, f=f, alphas=alphas),
                     f"{pair} alphas {alphas}")


def test_undamped(h, sig, f, full):
    pair = ("g", "nfw")
    w = h.rsd_device(*pair, mus=MUS9, sigma_s=sig, f=f, damping=False).numpy()
    m = h.multipoles_device(*pair, sigma_s=sig, f=f, damping=False).numpy()
    check_wedges(w, None, rs.wedges(h, *pair, mus=MUS9, sigma_s=sig, f=f, damping=False), f"{pair} undamped")
    ref = rs.multipoles(h, *pair, sigma_s=sig, f=f, damping=False)
    for i, key in enumerate(WEDGE_KEYS):
        ok, worst = within(m[i], *ref[key], f"{pair} undamped multipoles of {key}")
        assert ok, worst
    assert np.array_equal(w[1], full[pair][0][1])                                     # D is on the 1-halo term only
    assert np.all(w[0] >= full[pair][0][0]) and np.all(w[0][:, :10] > full[pair][0][0][:, :10])  # (D = 1 exactly at high k)


# ---------------------------------------------------------------- 2. against existing code
@pytest.mark.parametrize("pair", PAIRS)
def test_no_dispersion_against_the_power_spectra(h, f, pair):
    """sigma_s = 0: P1h at every mu is the damped P_1h the model returns, and with f = 0 P2h is its P_2h - other kernels,
    other summation orders: each side is within the tol of the restatement's exact sum, so they agree within twice it."""
    zero = np.zeros((3, NM))
    mus = np.array([0.0, 0.6, 1.0])
    w = h.rsd_device(*pair, mus=mus, sigma_s=zero, f=np.zeros(3)).numpy()
    ref = rs.wedges(h, *pair, mus=mus, sigma_s=zero, f=np.zeros(3))
    for i, (key, real) in enumerate((("P1h", h.get_power_1halo(*pair)), ("P2h", h.get_power_2halo(*pair)))):
        ok, worst = within(w[i], real[..., None], 2 * ref[key][1], f"{pair} {key} against get_power (of twice the tol)")
        assert ok, (key, worst)
    assert np.array_equal(w[..., 0], w[..., 1]) and np.array_equal(w[..., 0], w[..., 2])
    m = h.multipoles_device(*pair, nmu=5, sigma_s=zero, f=np.zeros(3)).numpy()
    mref = rs.multipoles(h, *pair, nmu=5, sigma_s=zero, f=np.zeros(3))
    for i, key in enumerate(WEDGE_KEYS):
        assert np.all(np.abs(m[i][..., 0] - w[i][..., 0]) <= 2 * mref[key][1][..., 0]), key          # P_0 = P
        assert np.all(np.abs(m[i][..., 1:]) <= mref[key][1][..., 1:]), key                            # P_2 = P_4 = 0
    with_f = h.rsd_device(*pair, mus=mus, sigma_s=zero, f=f).numpy()
    assert np.array_equal(with_f[0], w[0]) and np.array_equal(with_f[1][..., 0], w[1][..., 0])  # f enters through mu alone


def test_one_halo_multipoles_against_a_quadrature_of_the_wedges(h, sig, f):
    """At small k sigma_s a 32-node rule resolves the Gaussians: the rule's sum of the device's own 1-halo wedges is the
    device's closed-form multipoles within the rule's own error - which the restatement gives as the distance between the
    same two routes on its side - plus the tols of both."""
    small = 0.005 * sig
    assert (h.ks.max() * small.max()) ** 2 < 40.0
    mus, _ = rsd.mu_rule(32)
    wl = rsd.legendre_weights(32)
    for pair in (("g", "g2"), ("nfw", "nfw")):
        w = h.rsd_device(*pair, mus=mus, sigma_s=small, f=f).numpy()[0]
        m = h.multipoles_device(*pair, sigma_s=small, f=f).numpy()[0]
        wref = rs.wedges(h, *pair, mus=mus, sigma_s=small, f=f)["P1h"]
        mref = rs.multipoles(h, *pair, sigma_s=small, f=f)["P1h"]
        quad, qtol = rs.rule(wref, wl)
        rule_error = np.abs(quad - mref[0])
        got = np.einsum("lq,zsq->zsl", wl, w)
        ok, worst = within(got, m, rule_error + qtol + mref[1], f"{pair} 32-node rule of the wedges against the moments")
        assert ok, worst
        assert np.all(rule_error <= 1e-12 * np.abs(mref[0][..., :1]))             # (the rule does resolve them here)


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


def test_determinism_and_independence(h, sig, f, full):
    pair = ("g", "g2")
    fw, fp, fm, fq = full[pair][:4]
    w, p = h.rsd_device(*pair, mus=MUS9, sigma_s=sig, f=f, parts=True)
    m, q = h.multipoles_device(*pair, sigma_s=sig, f=f, parts=True)
    assert np.array_equal(w.numpy(), fw) and np.array_equal(p.numpy(), fp)                      # repeat
    assert np.array_equal(m.numpy(), fm) and np.array_equal(q.numpy(), fq)
    # one redshift alone: the entry points on that redshift's slices of every array
    ctx = h._ctx()
    ta, tb = (h._tracer(r, 1) for r in h._resolve(*pair))
    kidx = ctx.upload_int32(np.arange(NK, dtype=np.int32))
    from hmvec_amd import bispectrum as bs
    damp = ctx.upload(bs.damping(h.ks, h.p["kstar_damping"]))
    d_mus, d_sig, d_f = ctx.upload(MUS9), ctx.upload(sig), ctx.upload(f)
    rmu, d_wl = ctx.upload(np.ascontiguousarray(rsd.mu_rule(16)[0])), ctx.upload(rsd.legendre_weights(16))
    for z in range(3):
        a, b = shifted(ta, z, NM, NK), shifted(tb, z, NM, NK)
        common = (h._d_nzm.ptr + 8 * z * NM, h._d_bh.ptr + 8 * z * NM, h._d_ms().ptr, h._d_wm().ptr, h._d_ks().ptr,
                  h._d_Pzk().ptr + 8 * z * NK, h._rho_m0(), kidx.ptr, damp.ptr)
        tail = (d_sig.ptr + 8 * z * NM, d_f.ptr + 8 * z, 1.0, 0.0, 1.0)
        out, parts = ctx.empty((2, 1, NK, 9)), ctx.empty((4, 1, NK, 9))
        ctx.call("hmg_rsd_wedges", 1, NM, NK, NK, 9, C.byref(a), C.byref(b), *common, d_mus.ptr, *tail, out.ptr, parts.ptr)
        assert np.array_equal(out.numpy()[:, 0], fw[:, z]) and np.array_equal(parts.numpy()[:, 0], fp[:, z]), z
        out, Q = ctx.empty((2, 1, NK, 3)), ctx.empty((3, 1, NK))
        ctx.call("hmg_rsd_multipoles", 1, NM, NK, NK, 16, C.byref(a), C.byref(b), *common, rmu.ptr, d_wl.ptr, *tail, out.ptr,
                 Q.ptr)
        assert np.array_equal(out.numpy()[:, 0], fm[:, z]) and np.array_equal(Q.numpy()[:, 0], fq[:, z]), z


def test_after_a_deferring_pass_results_equal_those_on_a_whole_tensor(monkeypatch):
    """The NFW tensor's deferred short-series tiles are filled before these kernels read it: poisoned before the pass, the
    results are finite and have the bits of a model that writes its tensors whole.  The grid of
    tests/test_gpu_series_deferral.py: 300 wavenumbers from 1e-4, rows with none, one and two whole deferred tiles."""
    zs, ks, ms = np.linspace(0.1, 2.5, 3), np.geomspace(1e-4, 50, 300), np.geomspace(2e10, 1e17, 70)

    def step(m):
        m.init_mass_function(m.ms)
        m.add_nfw_profile("nfw", ignore_existing=True)
        m.add_battaglia_profile("electron", family="AGN", xmax=20, nxs=1000, ignore_existing=True)
        m.add_hod("g", mthresh=10 ** 10.5 + m.zs * 0.0, ignore_existing=True)

    def make(defer):
        monkeypatch.delenv("HMG_NO_HINTS", raising=False)
        monkeypatch.setenv("HMG_NO_GROUPS", "0")
        monkeypatch.setenv("HMG_NO_PREFIX_DEFERRAL", "0" if defer else "1")
        m = model(zs, ks=ks, ms=ms)
        assert m.prefix_deferral == defer
        step(m)
        return m

    def pending(m):
        ctx = m._ctx()
        ctx.flush()
        n = C.c_int()
        assert ctx.lib.hmg_prefix_pending(ctx.handle, m.uk_profiles.dev("nfw", fill=False).ptr, C.byref(n)) == 0
        return n.value

    whole = make(False)
    kw = dict(sigma_s=rsd.virial_dispersion(whole), f=whole.get_growth_rate_f(zs))
    want_w = whole.rsd_device("g", "nfw", mus=MUS9, **kw).numpy()
    want_m = whole.multipoles_device("g", "nfw", **kw).numpy()
    m = make(True)
    for entry, want in (("w", want_w), ("m", want_m)):
        d = m.uk_profiles.dev("nfw", fill=False)
        m._ctx().write(d, np.full(d.shape, np.nan))
        step(m)
        assert pending(m) == 1
        got = (m.rsd_device("g", "nfw", mus=MUS9, **kw) if entry == "w" else m.multipoles_device("g", "nfw", **kw)).numpy()
        assert pending(m) == 0
        assert np.all(np.isfinite(got)) and np.array_equal(got, want), entry


# ---------------------------------------------------------------- 4. the entry points' own refusals
def test_entry_point_errors(h, sig, f):
    ctx = h._ctx()
    ta, tb = (h._tracer(r, 1) for r in h._resolve("g", "nfw"))
    ty = nat.Tracer(nat.TRACER_PRESSURE, ta.d_prof, None, None, None, None, None, None, None, None, None)
    ones = ctx.upload(np.ones(NK))
    d_mus, d_sig, d_f = ctx.upload(np.linspace(0, 1, 33)), ctx.upload(sig), ctx.upload(f)
    d_wl = ctx.upload(np.ones((3, 33)))
    good_k = ctx.upload_int32(np.arange(NK, dtype=np.int32))
    outw, outm = ctx.empty((2, 3, NK, 32)), ctx.empty((2, 3, NK, 3))

    def wedges(n=NK, nmu=9, a=ta, b=tb, kidx=good_k, out=outw):
        ctx.call("hmg_rsd_wedges", 3, NM, NK, n, nmu, C.byref(a), C.byref(b), h._d_nzm.ptr, h._d_bh.ptr, h._d_ms().ptr,
                 h._d_wm().ptr, h._d_ks().ptr, h._d_Pzk().ptr, h._rho_m0(), kidx.ptr, ones.ptr, d_mus.ptr, d_sig.ptr, d_f.ptr,
                 1.0, 0.0, 1.0, nat.ptr(out), None)

    def multipoles(n=NK, nmu=9, a=ta, b=tb, kidx=good_k, out=outm):
        ctx.call("hmg_rsd_multipoles", 3, NM, NK, n, nmu, C.byref(a), C.byref(b), h._d_nzm.ptr, h._d_bh.ptr, h._d_ms().ptr,
                 h._d_wm().ptr, h._d_ks().ptr, h._d_Pzk().ptr, h._rho_m0(), kidx.ptr, ones.ptr, d_mus.ptr, d_wl.ptr, d_sig.ptr,
                 d_f.ptr, 1.0, 0.0, 1.0, nat.ptr(out), None)

    for call in (wedges, multipoles):
        call()                                                     # (good arguments; each call below has one bad one)
        for kw, msg in ((dict(n=0), "no sample"), (dict(n=NK + 1), "more samples than nodes"), (dict(nmu=0), "no mu"),
                        (dict(nmu=33), "32 mu"), (dict(out=None), "NULL"), (dict(a=ty), "pressure"), (dict(b=ty), "pressure")):
            with pytest.raises(nat.NativeError, match=msg):
                call(**kw)
        for bad in ([3, 4, NK], [3, -1, 4]):
            with pytest.raises(nat.NativeError, match="nk-1"):
                call(n=3, kidx=ctx.upload_int32(np.array(bad, dtype=np.int32)))
    # a captured step is refused before anything is enqueued or read (a context of its own: nothing of the model's is
    # queued in it; the arguments are never dereferenced)
    ctx2 = nat.Context(0)

    def body():
        for entry, extra in (("hmg_rsd_wedges", ()), ("hmg_rsd_multipoles", (d_wl.ptr,))):
            with pytest.raises(nat.NativeError, match="captured step"):
                ctx2.call(entry, 3, NM, NK, NK, 9, C.byref(ta), C.byref(tb), h._d_nzm.ptr, h._d_bh.ptr, h._d_ms().ptr,
                          h._d_wm().ptr, h._d_ks().ptr, h._d_Pzk().ptr, h._rho_m0(), good_k.ptr, ones.ptr, d_mus.ptr, *extra,
                          d_sig.ptr, d_f.ptr, 1.0, 0.0, 1.0, outw.ptr, None)

    gid = ctx2.capture(body)
    ctx2.call("hmg_graph_destroy", gid)
    ctx2.close()
    with pytest.raises(ValueError, match="pressure"):
        h.rsd_device("nfw", "y")
    with pytest.raises(ValueError, match="pressure"):
        h.get_power_multipoles("y")
