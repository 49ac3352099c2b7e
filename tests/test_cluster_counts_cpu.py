"""Cluster number counts, the parts that need no GPU: the default scatter rule against adaptive
quadrature, the restatement's tail form and its erfc constant against 40-digit mpmath, every refusal, the z bin
weights, the covariance algebra, the mean observables against their formulas, the ABI and the exports."""
import inspect
import os
import re
import sys
import warnings

import numpy as np
import pytest
from scipy.integrate import quad
from scipy.special import erfc

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import cluster_counts_model as cm  # noqa: E402

import hmvec_amd as hm  # noqa: E402
from hmvec_amd import clusters  # noqa: E402
from hmvec_amd.quadrature import trapz_weights  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE = np.ones(1)


# ---------------------------------------------------------------- 1. the default rule
RULE_BINS = [(5.0, 6.0), (6.0, 8.0), (8.0, np.inf)]
RULE_Q0 = np.geomspace(0.5, 30.0, 40)


def _p(q, ea, eb):
    return 0.5 * (erfc((ea - q) / np.sqrt(2.0)) - erfc((eb - q) / np.sqrt(2.0)))


def _quad_reference(sigma):
    ref = np.empty((RULE_Q0.size, len(RULE_BINS)))
    for i, q0 in enumerate(RULE_Q0):
        for a, (ea, eb) in enumerate(RULE_BINS):
            f = lambda t: np.exp(-0.5 * t * t) / np.sqrt(2.0 * np.pi) * _p(q0 * np.exp(sigma * t), ea, eb)  # noqa: E731
            pts = sorted({float(np.clip(np.log(e / q0) / sigma, -11.9, 11.9)) for e in (ea, eb) if np.isfinite(e)})
            with warnings.catch_warnings():          # (where the integral is 1e-30 quad cannot reach epsrel and says so)
                warnings.simplefilter("ignore")
                ref[i, a] = quad(f, -12.0, 12.0, points=pts, epsabs=0.0, epsrel=1e-13, limit=400)[0]
    return ref


def _rule_error(rule, sigma, ref):
    worst = 0.0
    for a, (ea, eb) in enumerate(RULE_BINS):
        S = cm.selection(np.log(RULE_Q0)[None, :], np.full((1, RULE_Q0.size), sigma), np.zeros(1), ONE, *rule,
                         np.array([ea, eb]), 0)
        worst = max(worst, float(np.max(np.abs(S[0, :, 0] - ref[:, a]))))
    return worst


@pytest.fixture(scope="module")
def quad_refs():
    return {s: _quad_reference(s) for s in (0.1, 0.2, 0.4)}


def test_default_rule_integrates_the_selection_to_1e_10(quad_refs):
    """Gate 1e-10 absolute: ten times the 1.0e-11 measured for the 64-node trapezoid, above the 2.6e-12 truncation floor at
    +-7; the 32-node rule must be worse than 1e-6, so the default is not quietly lowered."""
    t, w = hm.scatter_rule()
    assert t.size == 64 and t[0] == -7.0 and t[-1] == 7.0 and abs(w.sum() - 1.0) <= 1e-15
    e64 = max(_rule_error((t, w), s, quad_refs[s]) for s in (0.1, 0.2, 0.4))
    e32 = max(_rule_error(hm.scatter_rule(G=32), s, quad_refs[s]) for s in (0.2, 0.4))
    print(f"scatter rule against quad: 64 nodes {e64:.2e}, 32 nodes {e32:.2e}")
    assert e64 <= 1e-10
    assert e32 > 1e-6
    assert np.array_equal(hm.scatter_rule(G=1)[0], [0.0]) and np.array_equal(hm.scatter_rule(G=1)[1], [1.0])
    for bad in (dict(G=0), dict(G=2.5), dict(tmax=0.0), dict(tmax=np.inf)):
        with pytest.raises(ValueError):
            hm.scatter_rule(**bad)


# ---------------------------------------------------------------- 2. the restatement against mpmath
def test_tail_form_keeps_a_halo_ten_sigma_away():
    import mpmath as mp
    mp.mp.dps = 40
    for q, edges in ((1.0, (11.0, 12.0)), (16.0, (5.0, 6.0))):          # 10 sigma below the lowest edge; above a finite bin
        lnq = np.log([[q]])
        S = cm.selection(lnq, np.zeros((1, 1)), np.zeros(1), ONE, np.zeros(1), ONE, np.array(edges), 0)[0, 0, 0]
        exact = cm.p_exact(mp.exp(mp.mpf(float(lnq[0, 0]))), *edges)
        rel = float(abs(mp.mpf(float(S)) - exact) / exact)
        print(f"q = {q}, bin {edges}: P = {S:.6e}, relative error {rel:.2e}")
        assert 1e-24 < S < 1e-22 and rel <= 1e-12


def test_erfc_constant_of_the_restatement():
    """c of tests/helpers/cluster_counts_model.py for scipy's erfc and numpy's exp; the gate is twice the recorded value."""
    lnq = np.log(cm.CE_Q)
    S = cm.selection(lnq[None, :], np.zeros((1, lnq.size)), np.zeros(1), ONE, np.zeros(1), ONE, cm.CE_EDGES, 0)[0]
    c, at = cm.measure_c(lnq, S)
    print(f"c of the restatement: {c:.3f} at (q, bin) = {at}; recorded {cm.CE_NUMPY_MEASURED}, gate {cm.CE_NUMPY}")
    assert cm.CE_NUMPY == 2.0 * cm.CE_NUMPY_MEASURED and cm.CE_DEVICE == 2.0 * cm.CE_DEVICE_MEASURED
    assert c <= cm.CE_NUMPY


def test_restatement_none_is_its_closed_form():
    import mpmath as mp
    mp.mp.dps = 40
    lnobs, sg, lnn = np.array([[1.3]]), np.array([[0.35]]), np.log(np.array([0.4, 2.0]))
    area, edges = np.array([0.3, 0.7]), np.array([0.0, 1.0, 3.0, np.inf])
    S = cm.selection(lnobs, sg, lnn, area, np.zeros(1), ONE, edges, 1)[0, 0]
    for a in range(3):
        ref = sum(ar * cm.p_exact(mp.mpf(1.3) - mp.mpf(float(l)), np.log(edges[a]) if edges[a] > 0 else -np.inf,
                                  np.log(edges[a + 1]), scale=1.0 / (mp.sqrt(2) * mp.mpf(0.35))) for ar, l in zip(area, lnn))
        assert abs(S[a] - float(ref)) <= 1e-14 * float(ref)
    assert abs(S.sum() - 1.0) <= 4e-16


# ---------------------------------------------------------------- 3. every refusal
GOOD = dict(q_edges=[5.0, 6.0, 8.0, np.inf], noise=[1.0, 2.0], area=[0.1, 0.2])


@pytest.mark.parametrize("change", [
    dict(q_edges=[5.0, np.nan, 8.0]), dict(q_edges=[5.0, np.inf, 8.0]), dict(q_edges=[5.0, 5.0, 8.0]),
    dict(q_edges=[6.0, 5.0]), dict(q_edges=[5.0]), dict(q_edges=[[5.0, 6.0]]), dict(q_edges=[np.inf, np.inf]),
    dict(q_edges=[-np.inf, 5.0], noise_model="none"), dict(q_edges=[-1.0, 5.0], noise_model="none"),
    dict(noise=0.0), dict(noise=[1.0, -2.0]), dict(noise=np.nan), dict(area=[0.1, -0.2]), dict(area=np.inf),
    dict(noise=[1.0, 2.0, 3.0]), dict(area=[[0.1, 0.2]]), dict(sigma_ln=-0.1), dict(sigma_ln=np.nan),
    dict(sigma_ln=[0.1, 0.2]), dict(sigma_ln=0.0, noise_model="none"), dict(sigma_ln=np.zeros((2, 3)), noise_model="none"),
    dict(rule=(np.zeros(1), np.ones(1)), noise_model="none"),
    dict(rule=(np.array([-1.0, 1.0]), np.array([0.5, 0.5 + 1e-11]))), dict(rule=(np.zeros(2), np.ones(3) / 3)),
    dict(rule=(np.zeros((1, 2)), np.ones((1, 2)) / 2)), dict(rule=(np.array([np.nan]), np.ones(1))), dict(rule=3.0),
    dict(rule=(np.zeros(0), np.zeros(0))), dict(noise_model="poisson"),
], ids=lambda c: ",".join(c))
def test_cluster_selection_refuses(change):
    with pytest.raises(ValueError):
        hm.cluster_selection(**{**GOOD, **change})


def test_cluster_selection_record():
    sel = hm.cluster_selection(**GOOD, sigma_ln=0.3)
    assert (sel.nq, sel.T, sel.G, sel.noise_model, sel.sigma_ln) == (3, 2, 64, "gaussian", 0.3)
    assert np.array_equal(sel.lnnoise, np.log([1.0, 2.0])) and sel.omega == 0.1 + 0.2
    t, w = hm.scatter_rule()
    assert np.array_equal(sel.t, t) and np.array_equal(sel.w, w)
    with pytest.raises(AttributeError):
        sel.nq = 4
    with pytest.raises(ValueError):
        sel.edges[0] = 1.0
    wide = hm.cluster_selection([-np.inf, np.inf], 2.0, 0.5, rule=(np.zeros(1), ONE))
    assert (wide.nq, wide.T, wide.G) == (1, 1, 1)
    none = hm.cluster_selection([0.0, 20.0, np.inf], 1.0, [0.5, 0.5], noise_model="none")
    assert (none.G, none.T) == (1, 2)


class StandIn:
    """A host-only stand-in for a HaloModel: any touch of a context fails the test."""
    zs = np.array([0.2, 0.5, 0.8, 1.1, 1.4])
    ms = np.geomspace(1e13, 1e15, 7)
    H0, omm = 70.0, 0.3
    mdef = "vir"

    def _main(self, needs_aux=False):
        raise AssertionError("a context is touched")

    _nz = property(lambda self: self.zs.size)
    _nm = property(lambda self: self.ms.size)

    def hubble_parameter(self, z):
        z = np.asarray(z, dtype=np.float64)
        return self.H0 * np.sqrt(self.omm * (1 + z) ** 3 + 1 - self.omm)

    def h_of_z(self, z):
        return self.hubble_parameter(z) / 299792.458

    def comoving_radial_distance(self, z):
        return np.array([quad(lambda x: 1.0 / self.h_of_z(x), 0.0, zz)[0] for zz in np.atleast_1d(z)])

    def angular_diameter_distance(self, z):
        return self.comoving_radial_distance(z) / (1.0 + np.asarray(z))

    def rho_critical_z(self, z):
        return 2.775e11 * (self.hubble_parameter(z) / 100.0) ** 2

    def _mdef_delta_rho(self):
        return 100.0 + 0.0 * self.zs, self.rho_critical_z(self.zs)

    def concentration(self):
        return 5.0 + np.zeros((self.zs.size, self.ms.size))


def test_model_level_refusals_touch_no_context():
    model, sel = StandIn(), hm.cluster_selection(**GOOD)
    lnobs = np.zeros((5, 7))
    calls = [lambda **k: hm.cluster_abundance_device(model, **k), lambda **k: hm.get_cluster_abundance(model, **k),
             lambda **k: hm.get_cluster_counts(model, z_edges=[0.2, 1.4], **k),
             lambda **k: hm.cluster_counts_cov(model, z_edges=[0.2, 1.4], sigma_b=np.ones(5), **k),
             lambda **k: hm.cluster_cl_cov(model, z_edges=[0.2, 1.4], ells=[100.0], pairs=[("nfw", "nfw")],
                                           sigma_b=np.ones(5), **k)]
    for call in calls:
        for bad in (dict(lnobs=np.zeros((5, 6)), sel=sel), dict(lnobs=np.full((5, 7), np.nan), sel=sel),
                    dict(lnobs=lnobs, sel=dict(GOOD)), dict(lnobs=lnobs, sel=sel, mmin=2e15),          # an empty window
                    dict(lnobs=lnobs, sel=sel, mmin=-1.0), dict(lnobs=lnobs, sel=sel, mmax=np.inf),
                    dict(lnobs=lnobs, sel=hm.cluster_selection(**GOOD, sigma_ln=np.full((5, 6), 0.2)))):
            with pytest.raises(ValueError):
                call(**bad)
    for bad in (dict(), dict(z_edges=[0.2, 1.4], zweights=np.ones((1, 5))), dict(z_edges=[0.2, 0.9]), dict(z_edges=[0.2]),
                dict(z_edges=[0.8, 0.2]), dict(zweights=np.ones((1, 4))), dict(zweights=np.ones(5))):
        with pytest.raises(ValueError):
            hm.get_cluster_counts(model, lnobs, sel, **bad)
    with pytest.raises(ValueError, match="0.9"):
        hm.get_cluster_counts(model, lnobs, sel, z_edges=[0.2, 0.9, 1.4])
    with pytest.raises(ValueError):
        hm.cluster_counts_cov(model, lnobs, sel, [0.2, 1.4], sigma_b=np.ones(4))
    assert clusters.mass_window(model.ms, 3e13, 5e14) == (2, 6) and clusters.mass_window(model.ms, None, None) == (0, 7)


# ---------------------------------------------------------------- 4. the z bin weights
def test_z_bin_weights_are_the_trapezoid_of_each_sub_grid():
    zs = np.array([0.1, 0.2, 0.4, 0.5, 0.9, 1.0, 1.6])
    tw = clusters.z_bin_weights(zs, [0.2, 0.5, 0.9, 1.6])
    assert tw.shape == (3, 7)
    want = np.zeros((3, 7))
    want[0, 1:4], want[1, 3:5], want[2, 4:7] = trapz_weights(zs[1:4]), trapz_weights(zs[3:5]), trapz_weights(zs[4:7])
    assert np.array_equal(tw, want)
    assert np.allclose(tw.sum(axis=1), [0.3, 0.4, 0.7], rtol=1e-15)
    for bad in ([0.2, 0.45], [0.2], [0.5, 0.2], [0.1, np.inf]):
        with pytest.raises(ValueError):
            clusters.z_bin_weights(zs, bad)


# ---------------------------------------------------------------- 5. the covariance algebra
def test_covariance_algebra_on_synthetic_abundances():
    rng = np.random.default_rng(11)
    nz, nq = 9, 4
    zs = np.sort(rng.uniform(0.1, 1.5, nz))
    chis, hzs, sb = 3000.0 * zs, 2.3e-4 * (1 + zs), 1e-7 / (1 + zs)
    n, bn = rng.uniform(1e-7, 1e-5, (nz, nq)), rng.uniform(1e-7, 5e-5, (nz, nq))
    tw = clusters.z_bin_weights(zs, zs[[0, 3, 8]])
    zw = tw * (chis ** 2 / hzs)[None, :]
    N = clusters.counts_from_abundance(n, zw)
    assert np.allclose(N, cm.counts(n, zw), rtol=1e-14)
    poisson, sample = clusters.counts_cov_from_abundance(N, bn, tw, chis, hzs, sb)
    rp, rs = cm.counts_cov(N, bn, tw, chis, hzs, sb)
    assert np.array_equal(poisson, rp) and np.allclose(sample, rs, rtol=1e-13)
    flat = sample.reshape(2 * nq, 2 * nq)
    assert np.array_equal(flat, flat.T) or np.allclose(flat, flat.T, rtol=1e-15, atol=0)
    assert np.linalg.eigvalsh(0.5 * (flat + flat.T)).min() >= -1e-12 * np.abs(flat).max()
    assert not sample[0, :, 1, :].any() and not sample[1, :, 0, :].any() and not poisson[0, :, 1, :].any()
    # a (-inf, +inf) bin sees every halo: bn = Omega b, and the sample variance is Omega^2 sum tw chi^4 sigma_b / H b^2
    omega, b = 0.37, rng.uniform(1.0, 3.0, nz)
    _, one = clusters.counts_cov_from_abundance(np.ones((2, 1)), (omega * b)[:, None], tw, chis, hzs, sb)
    for i in range(2):
        assert one[i, 0, i, 0] == pytest.approx(omega ** 2 * np.sum(tw[i] * chis ** 4 * sb / hzs * b * b), rel=1e-14)
    R, zscale = rng.normal(size=(2, nz, 5)), rng.uniform(0.5, 2.0, (2, nz))
    got = clusters.cl_cov_from_abundance(bn, R, tw, hzs, sb, zscale)
    assert got.shape == (2, nq, 2, 5) and np.allclose(got, cm.cl_cov(bn, R, tw, hzs, sb, zscale), rtol=1e-12, atol=1e-30)


# ---------------------------------------------------------------- 6. the mean observables
def test_sz_and_powerlaw_lnobs_are_their_formulas(monkeypatch):
    model = StandIn()
    seen = {}

    def host_mdelta(M1, C1, d1, d2):            # (a host stand-in for the conversion: the arguments are what is checked)
        seen["args"] = (M1, C1, d1, d2)
        return 0.7 * M1[None, :] * (d1 / d2)[:, None] ** 0.1

    monkeypatch.setattr(clusters, "mdelta_from_mdelta", host_mdelta)
    zs, ms = model.zs, model.ms
    A0, B0, C0, bias, mpivot = -4.3, 0.08, 0.5, 0.8, 2e14
    theta, Q = np.geomspace(1e-4, 1e-2, 12), np.linspace(0.3, 1.2, 12)
    got = hm.sz_lnobs(model, A0, B0, C0=C0, mpivot=mpivot, bias=bias, Q=(theta, Q))
    rhoc = model.rho_critical_z(zs)
    assert np.array_equal(seen["args"][0], ms) and np.array_equal(seen["args"][2], 100.0 * rhoc)
    assert np.array_equal(seen["args"][3], 500.0 * rhoc) and np.array_equal(seen["args"][1], model.concentration())
    m500 = host_mdelta(ms, None, 100.0 * rhoc, 500.0 * rhoc)
    ez = model.hubble_parameter(zs) / model.H0
    th = (3.0 * m500 / (4.0 * np.pi * 500.0 * rhoc[:, None])) ** (1.0 / 3.0) / model.angular_diameter_distance(zs)[:, None]
    want = np.log(10.0 ** A0 * ez[:, None] ** 2 * (bias * m500 / mpivot) ** (1 + B0) * (1 + zs)[:, None] ** C0
                  * np.interp(th, theta, Q))
    assert got.shape == (5, 7) and np.allclose(got, want, rtol=1e-13, atol=1e-13)
    plain = hm.sz_lnobs(model, A0, B0)
    assert np.allclose(plain, np.log(10.0 ** A0 * ez[:, None] ** 2 * (m500 / 3e14) ** (1 + B0)), rtol=1e-13, atol=1e-13)
    with pytest.raises(ValueError):
        hm.sz_lnobs(model, A0, B0, Q=(theta[::-1], Q))
    got = hm.powerlaw_lnobs(model, np.log(30.0), 1.1, C=0.4, mpivot=2e14, zpivot=0.6)
    want = np.log(30.0 * (ms[None, :] / 2e14) ** 1.1 * ((1 + zs)[:, None] / 1.6) ** 0.4)
    assert np.allclose(got, want, rtol=1e-13, atol=1e-13)
    assert "mpivot" in clusters.SZ_DEFAULTS and not any(k.startswith("cluster") for k in hm.default_params)


# ---------------------------------------------------------------- 7. ABI and exports
def test_entry_point_is_declared_and_bound_and_the_abi_version_stays():
    from hmvec_amd import _native as nat
    header = open(os.path.join(REPO, "include", "hmgrid.h")).read()
    m = re.search(r"\bint hmg_cluster_selection\(hmg_ctx\* ctx, ([^;]*)\);", header)
    assert m
    declared = re.sub(r"/\*.*?\*/", "", m.group(0), flags=re.S)
    assert declared.count(",") + 1 == 22 == len(nat.SIGNATURES["hmg_cluster_selection"])
    par = nat.PARAMS["hmg_cluster_selection"]
    assert par[:7] == ("ctx", "nz", "nm", "T", "G", "nq", "kind") and par[-6:] == ("d_nzm", "d_bh", "d_wm", "d_n", "d_bn", "d_S")
    sig = nat.SIGNATURES["hmg_cluster_selection"]
    assert all(s is nat._P for s, n in zip(sig, par) if n.startswith("d_") or n == "ctx")
    assert all(s is nat._I for s, n in zip(sig, par) if not (n.startswith("d_") or n == "ctx"))
    assert int(re.search(r"#define HMG_ABI_VERSION (\d+)", header).group(1)) == 10 == nat.ABI_VERSION
    mk = open(os.path.join(REPO, "hmvec_amd", "csrc", "Makefile")).read()
    assert re.search(r"^KUNITS = .*\bclusters\b", mk, flags=re.M)
    assert re.search(r"^DEPS_clusters\s*=\s*kernels/clusters\.hpp", mk, flags=re.M)
    assert clusters.BINS_PER_LAUNCH == int(re.search(r"constexpr int CL_BINS = (\d+);", open(os.path.join(
        REPO, "hmvec_amd", "csrc", "kernels", "clusters.hpp")).read()).group(1))


def test_the_model_block_is_passed_by_name():
    from hmvec_amd import _native as nat
    from hmvec_amd.halomodel import HaloModel
    block = [n for n in nat.PARAMS["hmg_cluster_selection"] if n in HaloModel._MODEL_BLOCK]
    assert block == ["d_nzm", "d_bh", "d_wm"]


def test_exports():
    names = ("cluster_selection", "scatter_rule", "cluster_abundance_device", "get_cluster_abundance", "get_cluster_counts",
             "cluster_counts_cov", "cluster_cl_cov", "sz_lnobs", "powerlaw_lnobs")
    for name in names:
        assert getattr(hm, name) is getattr(clusters, name) and name in hm.__all__ and name in clusters.__all__
    assert hm.clusters is clusters and "clusters" in hm.__all__
    par = inspect.signature(hm.cluster_selection).parameters
    assert list(par) == ["q_edges", "noise", "area", "sigma_ln", "rule", "noise_model"]
    assert par["sigma_ln"].default == 0.2 and par["rule"].default is None and par["noise_model"].default == "gaussian"
    assert list(inspect.signature(hm.cluster_abundance_device).parameters) == ["model", "lnobs", "sel", "mmin", "mmax",
                                                                               "selection"]
    assert list(inspect.signature(hm.cluster_cl_cov).parameters)[:10] == ["model", "lnobs", "sel", "z_edges", "ells", "pairs",
                                                                          "windows", "fsky", "sigma_b", "damping"]
    assert list(inspect.signature(hm.scatter_rule).parameters) == ["G", "tmax"]
