"""Cluster number counts on the device (hmg_cluster_selection, hmvec_amd/clusters.py) against the numpy
restatement tests/helpers/cluster_counts_model.py within its derived tolerance, and the properties the section states:
closure, bit-identity of an element whatever else shares the call, additivity of bins, the closed form of
noise_model="none", the z sums and the covariances, and the measurement of the tolerance's constant c.

Measured on an MI355X: c of the device 1.402 at (q, bin) = (2.105, 38 .. inf) (see test_erfc_constant_of_the_device); worst |got - ref| / tol of the sweep
is printed by every test."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import cluster_counts_model as cm  # noqa: E402
import lensing_model  # noqa: E402

pytestmark = pytest.mark.gpu

ZS = np.array([0.2, 0.8, 1.4])
NM = 70                                  # a full 64-mass tile and a partial one
MS = np.geomspace(1e12, 1e16, NM)
WINDOW = (MS[20] * 0.999, MS[66] * 1.001)          # starts mid-tile: grid masses 20 .. 66
EDGES = {1: np.array([5.0, 5.001]),
         4: np.array([-np.inf, 5.0, 5.001, 8.0, np.inf]),
         17: np.array([-np.inf, 0.0, 2.0, 3.0, 4.0, 5.0, 5.001, 5.5, 6.0, 7.0, 8.0, 10.0, 12.0, 16.0, 20.0, 30.0, 38.0,
                       np.inf])}
EDGES_NONE = {1: EDGES[1], 4: np.concatenate([[0.0], EDGES[4][1:]]), 17: np.concatenate([[0.0, 1.0], EDGES[17][2:]])}


@pytest.fixture(scope="module")
def h():
    return lensing_model.model(ZS, ms=MS)


@pytest.fixture(scope="module")
def host(h):
    """The model's own arrays on the host and the two mean observables of the sweep, computed once."""
    import hmvec_amd as hm
    from hmvec_amd.quadrature import trapz_weights
    lnobs = hm.powerlaw_lnobs(h, np.log(6.0), 1.5, C=0.7, mpivot=3e14)
    rng = np.random.default_rng(5)
    sig = rng.uniform(0.1, 0.45, (ZS.size, NM))
    return dict(nzm=np.array(h.nzm), bh=np.array(h.bh), wm=trapz_weights(MS), lnobs=lnobs, sig=sig)


def survey(T, seed=0):
    """T tiles whose noise spans a factor of 30: the same halo is far below, inside and far above the bins."""
    rng = np.random.default_rng(100 + T + seed)
    noise = np.geomspace(0.2, 6.0, T) if T > 1 else np.array([1.1])
    return noise, rng.uniform(1e-3, 5e-3, T)


def rule(G):
    import hmvec_amd as hm
    if G == 7:                  # (not symmetric, not sorted: the kernel is rule-agnostic)
        t = np.array([0.3, -2.0, 1.1, -0.7, 2.4, 0.0, -1.3])
        w = np.array([0.2, 0.05, 0.15, 0.2, 0.05, 0.25, 0.1])
        return t, w / w.sum()
    return hm.scatter_rule(G=G)


def reference(host, sel, sig, window):
    kind = 0 if sel.noise_model == "gaussian" else 1
    S, Mb, Xb = cm.selection(host["lnobs"], sig, sel.lnnoise, sel.area, sel.t, sel.w, sel.edges, kind, window, bound=True)
    n, bn = cm.mass_sums(S, host["wm"], host["nzm"], host["bh"], window)
    return S, Mb, Xb, n, bn


def check(host, sel, sig, window, got, sides=2, c=None, ref=None):
    S, Mb, Xb, n, bn = ref if ref is not None else reference(host, sel, sig, window)
    count = sel.T * sel.G if sel.noise_model == "gaussian" else sel.T
    c = cm.CE_DEVICE + cm.CE_NUMPY if c is None else c
    tS, tn, tbn = cm.tolerances(S, Mb, Xb, host["wm"], host["nzm"], host["bh"], count, c, sides, window, sel.area.max())
    worst = {}
    for name, g, r, t in (("n", got["n"], n, tn), ("bn", got["bn"], bn, tbn), ("S", got["S"], S, tS)):
        assert g.shape == r.shape and np.all(np.isfinite(g))
        ratio = np.abs(g - r) / np.where(t > 0, t, 1.0)
        assert np.all((t > 0) | (g == r)), name
        worst[name] = float(ratio.max())
    return worst


SWEEP = [(T, G, nq, i) for i, (T, G, nq) in enumerate(
    [(1, 1, 17), (1, 7, 4), (1, 64, 1), (5, 1, 4), (5, 7, 17), (5, 64, 4), (67, 1, 1), (67, 7, 4), (67, 64, 17)])]


@pytest.mark.parametrize("T,G,nq,i", SWEEP, ids=lambda v: str(v))
def test_gaussian_selection_against_the_restatement(h, host, T, G, nq, i):
    """sigma_ln a scalar (even cases) or an (nz, nm) array (odd), the mass window whole (cases 0, 1, 2 mod 4) or starting
    mid-tile (3 mod 4 and the largest case)."""
    import hmvec_amd as hm
    noise, area = survey(T)
    sigma = 0.2 if i % 2 == 0 else host["sig"]
    sel = hm.cluster_selection(EDGES[nq], noise, area, sigma_ln=sigma, rule=rule(G))
    windowed = i % 4 == 3 or i == 8
    mm = dict(mmin=WINDOW[0], mmax=WINDOW[1]) if windowed else {}
    got = hm.get_cluster_abundance(h, host["lnobs"], sel, selection=True, **mm)
    sig = np.broadcast_to(np.asarray(sigma, dtype=np.float64), (ZS.size, NM))
    worst = check(host, sel, sig, (20, 67) if windowed else None, got)
    print(f"T = {T}, G = {G}, nq = {nq}: worst |got - ref| / tol  n {worst['n']:.3f}  bn {worst['bn']:.3f}  S {worst['S']:.3f}")
    assert max(worst.values()) <= 1.0
    with np.errstate(all="ignore"):
        assert np.array_equal(got["bias"], got["bn"] / got["n"], equal_nan=True)
    if windowed:
        assert not got["S"][:, :20].any() and not got["S"][:, 67:].any() and got["S"][:, 20:67].any()


@pytest.mark.parametrize("T,nq", [(1, 4), (5, 17), (67, 1)])
def test_selection_without_noise_against_the_restatement_and_mpmath(h, host, T, nq):
    """noise_model="none" against the restatement, and 50 of its elements against the closed form with 40-digit mpmath
    (one-sided: the device's own bound alone)."""
    import mpmath as mp
    import hmvec_amd as hm
    mp.mp.dps = 40
    noise, area = survey(T, seed=1)
    sig = host["sig"] if T != 5 else np.full((ZS.size, NM), 0.3)
    sel = hm.cluster_selection(EDGES_NONE[nq], noise, area, sigma_ln=sig if T != 5 else 0.3, noise_model="none")
    window = (20, 67) if T == 67 else None
    mm = dict(mmin=WINDOW[0], mmax=WINDOW[1]) if window else {}
    got = hm.get_cluster_abundance(h, host["lnobs"], sel, selection=True, **mm)
    ref = reference(host, sel, sig, window)
    worst = check(host, sel, sig, window, got, ref=ref)
    print(f"none, T = {T}, nq = {nq}: worst |got - ref| / tol  n {worst['n']:.3f}  bn {worst['bn']:.3f}  S {worst['S']:.3f}")
    assert max(worst.values()) <= 1.0
    S, Mb, Xb = ref[:3]
    tS = cm.tolerances(S, Mb, Xb, host["wm"], host["nzm"], host["bh"], T, cm.CE_DEVICE, 1, window, area.max())[0]
    rng = np.random.default_rng(T)
    lo, hi = window or (0, NM)
    ln_e = [-np.inf if e == 0 else float(np.log(e)) for e in sel.edges]         # (the doubles the device compares with)
    ratio = 0.0
    for _ in range(50):
        z, m, a = rng.integers(ZS.size), rng.integers(lo, hi), rng.integers(nq)
        scale = 1 / (mp.sqrt(2) * mp.mpf(float(sig[z, m])))
        exact = sum(mp.mpf(float(ar)) * cm.p_exact(mp.mpf(float(host["lnobs"][z, m])) - mp.mpf(float(l)), ln_e[a], ln_e[a + 1],
                                                   scale=scale) for ar, l in zip(sel.area, sel.lnnoise))
        ratio = max(ratio, float(abs(mp.mpf(float(got["S"][z, m, a])) - exact)) / tS[z, m, a])
    print(f"none, T = {T}: worst |S - closed form| / tol at 50 elements {ratio:.3f}")
    assert ratio <= 1.0


@pytest.mark.parametrize("T,G", [(1, 1), (5, 7), (67, 64)])
def test_closure_of_the_whole_line(h, host, T, G):
    """One bin (-inf, +inf): every halo is found, n / sum of area is the model's own sum_m wm nzm."""
    import hmvec_amd as hm
    noise, area = survey(T)
    sel = hm.cluster_selection([-np.inf, np.inf], noise, area, sigma_ln=host["sig"], rule=rule(G))
    got = hm.get_cluster_abundance(h, host["lnobs"], sel, mmin=WINDOW[0], mmax=WINDOW[1])
    want = np.sum((host["wm"][None, :] * host["nzm"])[:, 20:67], axis=1)
    wantb = np.sum((host["wm"][None, :] * host["nzm"] * host["bh"])[:, 20:67], axis=1)
    depth = 6 + 6 + 2 + 3 + 47             # the two trees, the tiles, the products, numpy's own sum of 47 terms
    tol = (G + T + depth) * cm.U
    rn, rb = np.abs(got["n"][:, 0] / sel.omega / want - 1.0), np.abs(got["bn"][:, 0] / sel.omega / wantb - 1.0)
    print(f"closure T = {T}, G = {G}: worst relative error / tol  n {rn.max() / tol:.3f}  bn {rb.max() / tol:.3f}")
    assert rn.max() <= tol and rb.max() <= tol


def test_an_element_does_not_depend_on_what_shares_the_call(h, host):
    """Bit-identity: bin a alone against bin a among 17 (over three launches of 8 bins); one redshift against three;
    selection=True against False; a device lnobs against a host one."""
    import hmvec_amd as hm
    from hmvec_amd import _native as nat
    noise, area = survey(5)
    kw = dict(noise=noise, area=area, sigma_ln=host["sig"], rule=rule(7))
    sel = hm.cluster_selection(EDGES[17], **kw)
    mm = dict(mmin=WINDOW[0], mmax=WINDOW[1])
    full = hm.get_cluster_abundance(h, host["lnobs"], sel, selection=True, **mm)
    for a in (0, 6, 7, 8, 11, 16):
        one = hm.get_cluster_abundance(h, host["lnobs"], hm.cluster_selection(EDGES[17][a:a + 2], **kw), selection=True, **mm)
        for k in ("n", "bn", "S"):
            assert np.array_equal(one[k][..., 0], full[k][..., a]), (k, a)
    plain = hm.get_cluster_abundance(h, host["lnobs"], sel, **mm)
    assert "S" not in plain and np.array_equal(plain["n"], full["n"]) and np.array_equal(plain["bn"], full["bn"])
    ctx = h._main()
    d_ln = ctx.upload(host["lnobs"])
    dev = hm.cluster_abundance_device(h, d_ln, sel, selection=True, **mm)
    assert all(isinstance(d, nat.DeviceArray) for d in dev)
    assert [d.shape for d in dev] == [(3, 17), (3, 17), (3, NM, 17)]
    for d, k in zip(dev, ("n", "bn", "S")):
        assert np.array_equal(d.numpy(), full[k]), k
    # one redshift alone: the entry point on row 1 of every (nz, nm) array
    row = 8 * NM
    d_sig, d_lnn, d_area = ctx.upload(host["sig"]), ctx.upload(sel.lnnoise), ctx.upload(sel.area)
    d_t, d_w, d_e = ctx.upload(sel.t), ctx.upload(sel.w), ctx.upload(sel.edges)
    n1, bn1, S1 = ctx.empty((1, 17)), ctx.empty((1, 17)), ctx.empty((1, NM, 17))
    ctx.call("hmg_cluster_selection", nz=1, nm=NM, T=5, G=7, nq=17, kind=0, d_lnobs=d_ln.ptr + row, d_sigln=d_sig.ptr + row,
             d_lnnoise=d_lnn.ptr, d_area=d_area.ptr, d_t=d_t.ptr, d_w=d_w.ptr, d_edges=d_e.ptr, m_lo=20, m_hi=67,
             d_nzm=h._d_nzm.ptr + row, d_bh=h._d_bh.ptr + row, d_wm=h._d_wm().ptr, d_n=n1.ptr, d_bn=bn1.ptr, d_S=S1.ptr)
    assert np.array_equal(n1.numpy()[0], full["n"][1]) and np.array_equal(bn1.numpy()[0], full["bn"][1])
    assert np.array_equal(S1.numpy()[0], full["S"][1])
    again = hm.get_cluster_abundance(h, host["lnobs"], sel, selection=True, **mm)
    assert all(np.array_equal(again[k], full[k]) for k in ("n", "bn", "S"))


def test_bins_add_up(h, host):
    """Bins 5 - 6 plus 6 - 8 against the bin 5 - 8, within the sum of their tolerances."""
    import hmvec_amd as hm
    noise, area = survey(67)
    kw = dict(noise=noise, area=area, sigma_ln=0.2, rule=rule(64))
    two, one = hm.cluster_selection([5.0, 6.0, 8.0], **kw), hm.cluster_selection([5.0, 8.0], **kw)
    g2 = hm.get_cluster_abundance(h, host["lnobs"], two, selection=True)
    g1 = hm.get_cluster_abundance(h, host["lnobs"], one, selection=True)
    sig = np.full((ZS.size, NM), 0.2)
    worst = 0.0
    tols = []
    for sel in (two, one):
        S, Mb, Xb, _, _ = reference(host, sel, sig, None)
        tols.append(cm.tolerances(S, Mb, Xb, host["wm"], host["nzm"], host["bh"], 67 * 64, cm.CE_DEVICE, 1, None, area.max()))
    for i, k in enumerate(("S", "n", "bn")):
        tol = tols[0][i].sum(axis=-1) + tols[1][i][..., 0]
        worst = max(worst, float(np.max(np.abs(g2[k].sum(axis=-1) - g1[k][..., 0]) / tol)))
    print(f"additivity of bins: worst |(5-6) + (6-8) - (5-8)| / tol {worst:.3f}")
    assert worst <= 1.0 and g1["n"].min() > 0


def test_counts_and_covariances_are_the_algebra_of_the_abundances(h, host):
    """get_cluster_counts, cluster_counts_cov and cluster_cl_cov against the helper's plain loops on the downloaded n, bn and
    response_device's R."""
    import hmvec_amd as hm
    from hmvec_amd import clusters
    from hmvec_amd.cov import limber_samples, sigma_b_disc
    from hmvec_amd.cosmology import sigma2_kgrid
    noise, area = survey(5)
    sel = hm.cluster_selection(EDGES[4], noise, area * 40.0, sigma_ln=0.25, rule=rule(7))
    ab = hm.get_cluster_abundance(h, host["lnobs"], sel)
    chis, hzs = h.comoving_radial_distance(ZS), h.h_of_z(ZS)
    for z_edges in ([0.2, 1.4], [0.2, 0.8, 1.4]):
        tw = clusters.z_bin_weights(ZS, z_edges)
        zw = tw * (chis ** 2 / hzs)[None, :]
        got = hm.get_cluster_counts(h, host["lnobs"], sel, z_edges=z_edges)
        assert np.array_equal(got["n"], ab["n"]) and np.array_equal(got["bn"], ab["bn"])
        N = cm.counts(ab["n"], zw)
        assert np.allclose(got["N"], N, rtol=1e-14) and np.allclose(got["bN"], cm.counts(ab["bn"], zw), rtol=1e-14)
        assert np.allclose(got["bias"], got["bN"] / got["N"], rtol=1e-15)
        same = hm.get_cluster_counts(h, host["lnobs"], sel, zweights=zw)
        assert np.array_equal(same["N"], got["N"])
        kq = sigma2_kgrid(h.p["sigma2_kmin"], h.p["sigma2_kmax"], h.p["sigma2_numks"])
        sb = sigma_b_disc(kq, h.sPzk, chis, fsky=sel.omega / (4 * np.pi))
        cov = hm.cluster_counts_cov(h, host["lnobs"], sel, z_edges)
        rp, rs = cm.counts_cov(N, ab["bn"], tw, chis, hzs, sb)
        assert np.allclose(cov["N"], N, rtol=1e-14) and np.allclose(cov["poisson"], rp, rtol=1e-14)
        assert np.allclose(cov["sample"], rs, rtol=1e-13) and np.array_equal(cov["cov"], cov["poisson"] + cov["sample"])
        assert cov["sample"][0, 1, 0, 1] > 0
        given = hm.cluster_counts_cov(h, host["lnobs"], sel, z_edges, sigma_b=2.0 * sb)
        assert np.allclose(given["sample"], 2.0 * cov["sample"], rtol=1e-14)
        ells, pairs = np.array([100.0, 1000.0]), [("nfw", "nfw")]
        W = 1.0 + ZS
        idx, frac = limber_samples(ells, chis, h.ks, zs=ZS)
        R = h.response_device(pairs, idx=idx, frac=frac).numpy()
        cl = hm.cluster_cl_cov(h, host["lnobs"], sel, z_edges, ells, pairs, windows=[(W, 2.0)])
        want = cm.cl_cov(ab["bn"], R, tw, hzs, sb, (2.0 * W)[None, :])
        assert cl.shape == (len(z_edges) - 1, 4, 1, 2) and np.allclose(cl, want, rtol=1e-13) and np.all(cl != 0)


def test_erfc_constant_of_the_device(h):
    """The measurement of c: the worst error of the device's P_a(q) against 40-digit mpmath in units of the bound's own
    unit error (tests/helpers/cluster_counts_model.py), through the public interface with T = G = 1, area = 1, over
    q in linspace(-2, 40, 400), q > 0, against the edges {-inf, 0, 5, 5.001, 6, 8, 38, +inf}.  The gate is twice the
    recorded value."""
    import hmvec_amd as hm
    sel = hm.cluster_selection(cm.CE_EDGES, 1.0, 1.0, sigma_ln=0.0, rule=(np.zeros(1), np.ones(1)))
    lnq = np.log(cm.CE_Q)
    slots = ZS.size * NM
    P = np.empty((lnq.size, cm.CE_EDGES.size - 1))
    for start in range(0, lnq.size, slots):
        part = lnq[start:start + slots]
        lnobs = np.resize(part, slots).reshape(ZS.size, NM)
        S = hm.get_cluster_abundance(h, lnobs, sel, selection=True)["S"].reshape(slots, -1)
        P[start:start + part.size] = S[:part.size]
    c, at = cm.measure_c(lnq, P)
    print(f"c of the device: {c:.3f} at (q, bin) = {at}; recorded {cm.CE_DEVICE_MEASURED}, gate {cm.CE_DEVICE}")
    assert c <= cm.CE_DEVICE
