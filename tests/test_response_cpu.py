"""Host-side checks of the response / super-sample covariance contract; no GPU.  The numpy
restatement tests/helpers/response_model.py - the reference of tests/test_gpu_response.py - is pinned against plain
Python loops over (z, s, m) on synthetic arrays behind a stand-in object; the slope table, sigma_b_disc and the
bindings of the two entry points are checked on their own."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

import hmvec_amd
from hmvec_amd import _native as nat
from hmvec_amd import bispectrum as bs
from hmvec_amd import cov
from hmvec_amd.quadrature import simpson_weights, trapz_weights

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import response_model as rm  # noqa: E402

EPS = rm.EPS
NZ, NM, NK = 2, 5, 6
RHO = 3.7e10


class StandIn:
    """The attributes the restatement reads, filled with synthetic positive arrays."""

    def __init__(self):
        rng = np.random.default_rng(5)
        self.zs = np.array([0.3, 1.1])
        self.ks = np.geomspace(1e-2, 5.0, NK)
        self.ms = np.geomspace(1e12, 1e15, NM)
        self.nzm = rng.uniform(0.5, 2.0, (NZ, NM)) * 1e-16 * (self.ms[None, :] / 1e12) ** -1.9
        self.bh = rng.uniform(0.6, 4.0, (NZ, NM))
        self.Pzk = rng.uniform(0.8, 1.2, (NZ, NK)) * 1e4 * self.ks[None, :] ** -1.3
        self.p = {"kstar_damping": 0.4}
        prof = lambda lo, hi: rng.uniform(lo, hi, (NZ, NM, NK))  # noqa: E731
        self.uk_profiles = {"nfw": prof(0.1, 1.0), "e": prof(0.1, 1.0)}
        self.pk_profiles = {"y": prof(1e-3, 2e-3), "y2": prof(2e-3, 5e-3)}
        self.hods = {}
        for name, cen in (("g", None), ("gc", "e")):
            Nc, Ns = rng.uniform(0.1, 1.0, (NZ, NM)), rng.uniform(0.0, 8.0, (NZ, NM))
            self.hods[name] = {"Nc": Nc, "Ns": Ns, "NcNs": Nc * Ns * rng.uniform(0.9, 1.1, (NZ, NM)),
                               "NsNsm1": Ns * Ns * rng.uniform(0.9, 1.1, (NZ, NM)),
                               "ngal": rng.uniform(1e-4, 2e-4, NZ), "satellite_profile": "nfw", "central_profile": cen}

    def rho_matter_z(self, z):
        return np.array([RHO])


@pytest.fixture(scope="module")
def h():
    return StandIn()


@pytest.fixture(scope="module")
def tables():
    idx = np.array([[0, 2, 5, 3], [1, 4, 0, 5]])
    frac = np.array([[0.25, 0.0, 0.0, 0.9], [0.5, 1.0 - 2.0 ** -30, 0.0, 0.0]])
    scale = np.array([[1.0, 0.5, 2.0, 0.0], [1.5, 1.0, 1.0, 0.7]])
    return idx, frac, scale


PAIRS = [("nfw", "nfw"), ("g", "g"), ("g", "nfw"), ("y", "y"), ("nfw", "y"), ("gc", "e"), ("y", "y2"), ("g", "gc")]


# ---------------------------------------------------------------- plain loops
def _kind(h, name):
    return "h" if name in h.hods else "m" if name in h.uk_profiles else "p"


def _weight(h, name, z, m, k):
    kind = _kind(h, name)
    if kind == "m":
        return h.ms[m] * h.uk_profiles[name][z, m, k] / RHO
    if kind == "p":
        return h.pk_profiles[name][z, m, k]
    hod = h.hods[name]
    uc = 1.0 if hod["central_profile"] is None else h.uk_profiles[hod["central_profile"]][z, m, k]
    return (uc * hod["Nc"][z, m] + h.uk_profiles[hod["satellite_profile"]][z, m, k] * hod["Ns"][z, m]) / hod["ngal"][z]


def _square(h, a, b, z, m, k):
    ka, kb = _kind(h, a), _kind(h, b)
    if ka == "h" and kb == "h":
        hod = h.hods[a]
        uc = 1.0 if hod["central_profile"] is None else h.uk_profiles[hod["central_profile"]][z, m, k]
        us = h.uk_profiles[hod["satellite_profile"]][z, m, k]
        return (2.0 * uc * us * hod["NcNs"][z, m] + hod["NsNsm1"][z, m] * us * us) / hod["ngal"][z] ** 2
    if ka == "p" and kb == "p":
        return h.pk_profiles[a][z, m, k] ** 2
    return _weight(h, a, z, m, k) * _weight(h, b, z, m, k)


def _lerp(fn, k, f):
    return fn(k) if f == 0.0 else (1.0 - f) * fn(k) + f * fn(k + 1)


def _loops(h, a, b, idx, frac, scale, damping):
    wm = trapz_weights(h.ms)
    dl = cov.dlnp_table(h.ks, h.Pzk)
    R = np.zeros(idx.shape)
    parts = np.zeros((3,) + idx.shape)
    for z in range(NZ):
        for s in range(idx.shape[1]):
            k, f = int(idx[z, s]), float(frac[z, s])
            A1 = I1 = 0.0
            J, beta = {}, {}
            for name in (a, b):
                J[name] = beta[name] = 0.0
            low = dict.fromkeys((a, b), 0.0)
            for m in range(NM):
                w = wm[m] * h.nzm[z, m]
                S = _lerp(lambda kk: _square(h, a, b, z, m, kk), k, f)
                A1 += w * S
                I1 += w * h.bh[z, m] * S
                for name in set((a, b)):
                    J[name] += w * h.bh[z, m] * _lerp(lambda kk: _weight(h, name, z, m, kk), k, f)
                    kind = _kind(h, name)
                    if kind == "m":
                        low[name] += w * h.bh[z, m] * h.ms[m] / RHO
                    elif kind == "h":
                        hod = h.hods[name]
                        low[name] += w * h.bh[z, m] * (hod["Nc"][z, m] + hod["Ns"][z, m]) / hod["ngal"][z]
            for name in set((a, b)):
                kind = _kind(h, name)
                beta[name] = low[name] if kind == "h" else 0.0
                J[name] = (J[name] + (1.0 if kind == "m" else 0.0 if kind == "p" else low[name])) - low[name]
            P = _lerp(lambda kk: h.Pzk[z, kk], k, f)
            ns = _lerp(lambda kk: dl[z, kk], k, f)
            ksamp = _lerp(lambda kk: h.ks[kk], k, f)
            D = float(bs.damping(ksamp, h.p["kstar_damping"])) if damping else 1.0
            P2h = P * J[a] * J[b]
            R[z, s] = scale[z, s] * ((47.0 / 21.0 - ns / 3.0) * P2h + D * I1 - (beta[a] + beta[b]) * (P2h + D * A1))
            parts[:, z, s] = A1, I1, P2h
    return R, parts


@pytest.mark.parametrize("damping", [False, True])
def test_restatement_against_plain_loops(h, tables, damping):
    idx, frac, scale = tables
    ref = rm.response(h, PAIRS, idx=idx, frac=frac, scale=scale, damping=damping)
    assert ref["R"][0].shape == (len(PAIRS), NZ, 4)
    for p, (a, b) in enumerate(PAIRS):
        R, parts = _loops(h, a, b, idx, frac, scale, damping)
        for key, got in (("A1", parts[0]), ("I1", parts[1]), ("P2h", parts[2])):
            val, tol = ref[key]
            assert np.all(np.abs(got - val[p]) <= tol[p]), (a, b, key)
        val, tol = ref["R"]
        assert np.all(np.abs(R - val[p]) <= tol[p]), (a, b)
        assert np.all(R[scale == 0.0] == 0.0) and np.all(val[p][scale == 0.0] == 0.0)


def test_first_name_rule_and_galaxy_bias_terms(h, tables):
    idx, frac, scale = tables
    ref = rm.response(h, [("y", "y2"), ("y2", "y"), ("nfw", "nfw"), ("g", "g")], idx=idx, frac=frac, scale=scale)
    (R, tol), live = ref["R"], scale != 0.0
    assert np.all(np.abs(R[0] - R[1])[live] > 100 * (tol[0] + tol[1])[live])           # pk_y^2 against pk_y2^2
    assert np.all(ref["beta_sum"][0][2] == 0.0) and np.all(ref["beta_sum"][0][3] > 0.0)
    assert np.all(R[2][live] > 0.0)                                                    # every term of a matter pair is positive


def test_slope_of_an_exact_power_law_is_its_index():
    ks = np.geomspace(1e-4, 30.0, 57)
    P = np.stack([2.0e4 * ks ** -1.7, 3.0 * ks ** 0.96])
    dl = cov.dlnp_table(ks, P)
    # a difference quotient of logarithms: each log is within an ulp of itself and P within two of the exact power
    # (8 EPS per difference with the three-point weights), over the narrowest spacing of log k
    bound = 8 * EPS * (np.abs(np.log(P)).max() + 4.0) / np.diff(np.log(ks)).min()
    assert np.all(np.abs(dl - np.array([[-1.7], [0.96]])) <= bound) and bound < 1e-12
    assert np.array_equal(dl, rm.dlnp(type("M", (), {"ks": ks, "Pzk": P})))


# ---------------------------------------------------------------- sigma_b
def test_sigma_b_disc():
    ks = np.geomspace(1e-4, 20.0, 401)
    P = np.stack([3e4 * ks / (1.0 + (ks / 0.02) ** 2.4), 1e4 * ks / (1.0 + (ks / 0.02) ** 2.4)])
    chis = np.array([900.0, 3100.0])
    flat = (simpson_weights(ks) * ks)[None, :] * P
    want, absum = flat.sum(axis=1) / (2 * np.pi), np.abs(flat).sum(axis=1) / (2 * np.pi)
    assert np.array_equal(cov.sigma_b_disc(ks, P, chis, theta_s=0.0), want)                  # x == 0: a window of 1
    assert np.all(np.abs(cov.sigma_b_disc(ks, P, chis, theta_s=1e-13) - want) <= ks.size * EPS * absum)
    s = [cov.sigma_b_disc(ks, P, chis, fsky=f) for f in (0.01, 0.1, 0.4, 1.0)]
    assert all(np.all(hi > lo) and np.all(lo > 0) for hi, lo in zip(s[:-1], s[1:]))          # decreasing in fsky
    assert np.array_equal(s[1], cov.sigma_b_disc(ks, P, chis, theta_s=np.arccos(1.0 - 2.0 * 0.1)))
    assert cov.sigma_b_disc(ks, P[0], chis[:1], fsky=0.1).shape == (1,)
    for kw in ({}, {"fsky": 0.1, "theta_s": 0.3}):
        with pytest.raises(ValueError, match="exactly one"):
            cov.sigma_b_disc(ks, P, chis, **kw)
    for f in (0.0, -0.1, 1.5, np.nan):
        with pytest.raises(ValueError, match="fsky"):
            cov.sigma_b_disc(ks, P, chis, fsky=f)
    with pytest.raises(ValueError, match="theta_s"):
        cov.sigma_b_disc(ks, P, chis, theta_s=-0.1)
    with pytest.raises(ValueError, match="shape"):
        cov.sigma_b_disc(ks, P[:, :-1], chis, fsky=0.1)


# ---------------------------------------------------------------- the contraction of the restatement
def test_ssc_of_the_restatement_is_symmetric_of_rank_nz(h, tables):
    idx, frac, scale = tables
    ref = rm.response(h, PAIRS[:3], idx=idx, frac=frac, scale=scale)
    g = np.array([0.7, 1.9])
    zscale = np.array([[1.0, 2.0], [0.5, 0.25], [3.0, 1.0]])
    covm, tol = rm.ssc(ref["R"], g, zscale)
    assert covm.shape == tol.shape == (3, 4, 3, 4)
    flat = covm.reshape(12, 12)
    assert np.all(np.abs(flat - flat.T) <= tol.reshape(12, 12))
    sv = np.linalg.svd(flat, compute_uv=False)
    assert np.all(sv[NZ:] <= 1e-12 * sv[0]) and sv[NZ - 1] > 1e-6 * sv[0]
    plain = rm.ssc((ref["R"][0] * zscale[:, :, None], ref["R"][1] * zscale[:, :, None]), g)      # scaling R first
    assert np.allclose(plain[0], covm, rtol=1e-13, atol=0)
    r = ref["R"][0] * zscale[:, :, None]
    assert np.isclose(covm[1, 0, 2, 3], sum(g[z] * r[1, z, 0] * r[2, z, 3] for z in range(NZ)), rtol=1e-13)


# ---------------------------------------------------------------- declared, exported, bound
@pytest.mark.parametrize("name,count", [("hmg_response", 21), ("hmg_ssc", 8)])
def test_entry_points_are_declared_exported_and_bound(name, count):
    with open(os.path.join(HERE, "..", "include", "hmgrid.h")) as f:
        header = f.read()
    m = re.search(r"int " + name + r"\((.*?)\);", header, re.S)
    assert m, f"{name} is not declared in include/hmgrid.h"
    args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")
    sig = nat.SIGNATURES[name]
    assert len(args) == len(sig) == count
    for a, t in zip(args, sig):
        a = a.strip()
        if "*" in a:
            assert t is C.c_void_p or issubclass(t, C._Pointer), a
        else:
            assert t is (C.c_double if a.startswith("double") else C.c_int), a
    assert os.path.exists(nat.LIB_PATH), "libhmgrid.so not built"
    assert hasattr(C.CDLL(nat.LIB_PATH), name)
    assert "#define HMG_ABI_VERSION 10" in header and nat.ABI_VERSION == 10


def test_exports():
    for name in ("sigma_b_disc", "cl_cov_ssc"):
        assert getattr(hmvec_amd, name) is getattr(cov, name) and name in hmvec_amd.__all__ and name in cov.__all__
    for name in ("response_device", "get_power_response", "ssc_device"):
        assert callable(getattr(hmvec_amd.HaloModel, name))
    assert hmvec_amd.HaloModel.RESPONSE_MAX_PAIRS == 16 and bs.MAX_SAMPLES == 256
