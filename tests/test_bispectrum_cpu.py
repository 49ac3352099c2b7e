"""Host-side checks of the bispectrum code, no GPU: the numpy restatement the GPU tests compare
with (tests/helpers/bispectrum_model.py) against a plain Python loop over (z, t, m); known answers of F2 and B_tree; the
factored cosine against exact rational arithmetic on squeezed triangles (and the naive numerator leaving the bound);
that B_tree does not sit on a cancellation on the GPU tests' grid; the damping factor's fixed operation sequence; the
host tables of cl_bispectrum and the triangle checks; and that the new entry point is declared, exported and bound."""
import ctypes as C
import itertools
import math
import os
import re
import sys
import types
from fractions import Fraction

import numpy as np
import pytest

import hmvec_amd
from hmvec_amd import _native as nat
from hmvec_amd import bispectrum as bs
from hmvec_amd.quadrature import trapz_weights

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import bispectrum_model as bm  # noqa: E402

EPS = 2.0 ** -52


# ---------------------------------------------------------------- the restatement against plain loops
def toy_model():
    """A stand-in with the facade's host arrays on a 2 x 5 x 6 grid (the toy of test_trispectrum_cpu.py with bh and Pzk
    added): two matter profiles, two pressure profiles, two HODs (one with a central profile).  The wavenumbers are
    close enough together for every triangle of them to close."""
    rng = np.random.default_rng(7)
    nz, nm, nk = 2, 5, 6
    h = types.SimpleNamespace()
    h.zs, h.ms, h.ks = np.array([0.3, 1.1]), np.geomspace(1e12, 1e15, nm), np.linspace(2.0, 3.0, nk)
    h.p = {"kstar_damping": 2.5}
    h.nzm = rng.uniform(0.5, 2.0, (nz, nm)) * 1e-18 * (h.ms / 1e13) ** -1.9
    h.bh = rng.uniform(0.6, 4.0, (nz, nm))
    h.Pzk = rng.uniform(0.5, 2.0, (nz, nk)) * 1e3 * h.ks[None, :] ** -1.5
    h.rho_matter_z = lambda z: np.array([3.9e10])
    h.uk_profiles = {"nfw": rng.uniform(0.1, 1.0, (nz, nm, nk)), "cen": rng.uniform(0.5, 1.0, (nz, nm, nk))}
    h.pk_profiles = {"y": rng.uniform(-0.2, 1.0, (nz, nm, nk)) * 1e-3, "y2": rng.uniform(0.1, 1.0, (nz, nm, nk))}

    def hod(cen):
        return dict(Nc=rng.uniform(0, 1, (nz, nm)), Ns=rng.uniform(0, 5, (nz, nm)), NcNs=rng.uniform(0, 3, (nz, nm)),
                    NsNsm1=rng.uniform(0, 9, (nz, nm)), ngal=rng.uniform(1e-4, 1e-3, nz), satellite_profile="nfw",
                    central_profile=cen)
    h.hods = {"g": hod(None), "gc": hod("cen")}
    return h


IDX = np.array([[0, 2, 5, 4], [5, 1, 1, 3]])                 # the last node with f = 0, f = 1, a zero and a negative scale
FRAC = np.array([[0.0, 0.25, 0.0, 1.0], [0.0, 0.5, 0.0, 0.125]])
SCALE = np.array([[1.0, 2.0, 0.0, -1.5], [0.5, 1.0, 1.0, 3.0]])
TRI = np.array([[0, 0, 0], [0, 1, 3], [3, 1, 0], [1, 1, 3], [2, 0, 1], [3, 3, 1], [1, 3, 2]])


def loop_weight(h, nm_, z, m, k):
    if nm_ in h.hods:
        d = h.hods[nm_]
        uc = 1.0 if d["central_profile"] is None else h.uk_profiles[d["central_profile"]][z, m, k]
        return (uc * d["Nc"][z, m] + h.uk_profiles[d["satellite_profile"]][z, m, k] * d["Ns"][z, m]) / d["ngal"][z]
    if nm_ in h.uk_profiles:
        return h.ms[m] * h.uk_profiles[nm_][z, m, k] / h.rho_matter_z(0)[0]
    return h.pk_profiles[nm_][z, m, k]


def loop_F2(p, q, r):
    p, q = max(p, q), min(p, q)
    mu = max(-1.0, min(1.0, ((r - p) * (r + p) - q * q) / (2 * p * q)))
    return 5 / 7 + 0.5 * mu * (p / q + q / p) + 2 / 7 * mu * mu


@pytest.mark.parametrize("names", [("nfw", "nfw", "nfw"), ("g", "nfw", "nfw"), ("gc", "y", "nfw"), ("y", "y2", "y")])
@pytest.mark.parametrize("damping", [False, True])
def test_restatement_against_plain_loops(names, damping):
    h = toy_model()
    nz, nm = h.nzm.shape
    nk = h.ks.size
    got = bm.bispectrum(h, names, TRI, idx=IDX, frac=FRAC, scale=SCALE, damping=damping)
    wm = trapz_weights(h.ms)
    rho = h.rho_matter_z(0)[0]

    def w(nm_, z, m, s):
        f, left = FRAC[z, s], loop_weight(h, nm_, z, m, IDX[z, s])
        return left if f == 0 else (1 - f) * left + f * loop_weight(h, nm_, z, m, IDX[z, s] + 1)

    def lin(row, z, s):
        f = FRAC[z, s]
        return row[IDX[z, s]] if f == 0 else (1 - f) * row[IDX[z, s]] + f * row[IDX[z, s] + 1]

    def J(nm_, z, s):
        wnb = [wm[m] * h.nzm[z, m] * h.bh[z, m] for m in range(nm)]
        I = sum(wnb[m] * w(nm_, z, m, s) for m in range(nm))
        if nm_ in h.hods:
            d = h.hods[nm_]
            C = sum(wnb[m] * (d["Nc"][z, m] + d["Ns"][z, m]) / d["ngal"][z] for m in range(nm))
            b = sum(wnb[m] * (d["Nc"][z, m] + d["Ns"][z, m]) for m in range(nm)) / d["ngal"][z]
        elif nm_ in h.uk_profiles:
            C, b = sum(wnb[m] * h.ms[m] / rho for m in range(nm)), 1.0
        else:
            C, b = 0.0, 0.0
        return I + b - C

    a, b, c = names
    for z in range(nz):
        for s in range(IDX.shape[1]):
            for leg, nm_ in enumerate(names):
                assert abs(got["J"][0][leg, z, s] - J(nm_, z, s)) <= got["J"][1][leg, z, s]
        for t, (s1, s2, s3) in enumerate(TRI):
            k = [lin(h.ks, z, s) for s in (s1, s2, s3)]
            P = [lin(h.Pzk[z], z, s) for s in (s1, s2, s3)]
            # (D through the contract's fixed operation sequence; test_damping_follows_the_function checks that one)
            D = [float(bs.damping(ki, h.p["kstar_damping"])) if damping else 1.0 for ki in k]
            sig = SCALE[z, s1] * SCALE[z, s2] * SCALE[z, s3]
            one = iab = ibc = iac = 0.0
            for m in range(nm):
                wn = wm[m] * h.nzm[z, m]
                wa, wb, wc = w(a, z, m, s1), w(b, z, m, s2), w(c, z, m, s3)
                one += wn * wa * wb * wc
                iab += wn * h.bh[z, m] * wa * wb
                ibc += wn * h.bh[z, m] * wb * wc
                iac += wn * h.bh[z, m] * wa * wc
            B1 = sig * D[0] * D[1] * D[2] * one
            B2 = sig * (D[0] * D[1] * iab * J(c, z, s3) * P[2] + D[1] * D[2] * ibc * J(a, z, s1) * P[0]
                        + D[0] * D[2] * iac * J(b, z, s2) * P[1])
            tree = 2 * (loop_F2(k[0], k[1], k[2]) * P[0] * P[1] + loop_F2(k[1], k[2], k[0]) * P[1] * P[2]
                        + loop_F2(k[2], k[0], k[1]) * P[2] * P[0])
            B3 = sig * J(a, z, s1) * J(b, z, s2) * J(c, z, s3) * tree
            for key, ref in (("B1h", B1), ("B2h", B2), ("B3h", B3)):
                val, tol = got[key][0][z, t], got[key][1][z, t]
                assert abs(val - ref) <= tol, (key, z, t, val, ref, tol)
    zero = np.any(SCALE[:, TRI] == 0, axis=2)                      # a zero scale gives an exact zero in every term
    assert zero.any()
    for key in ("B1h", "B2h", "B3h"):
        assert np.all(got[key][0][zero] == 0) and np.all(got[key][0][~zero] != 0)
    if names == ("y", "y2", "y"):                                  # two pressure names are two legs: no first-name rule
        other = bm.bispectrum(h, ("y", "y", "y"), TRI, idx=IDX, frac=FRAC, scale=SCALE, damping=damping)
        assert np.all(np.abs(other["B1h"][0] - got["B1h"][0])[~zero] > 100 * got["B1h"][1][~zero])


# ---------------------------------------------------------------- F2 and B_tree: known answers
def test_F2_known_answers():
    assert abs(bs.F2(1.3, 1.3, 1.3) - 2 / 7) <= 4 * EPS                       # equilateral: mu = -1/2
    P = 3.7
    assert abs(bs.tree_bispectrum(0.2, 0.2, 0.2, P, P, P) - 12 / 7 * P * P) <= 8 * EPS * P * P
    for p, q in ((1.0, 1.0), (0.25, 2.5), (7.0, 2.0 ** -7)):          # (p + q and |p - q| are exact in binary)
        s = p / q + q / p
        assert abs(bs.F2(p, q, p + q) - (5 / 7 + 0.5 * s + 2 / 7)) <= 8 * EPS * (1 + s)      # folded: mu = 1
        assert abs(bs.F2(p, q, abs(p - q)) - (5 / 7 - 0.5 * s + 2 / 7)) <= 8 * EPS * (1 + s)      # mu = -1
    assert bs.F2(1.0, 1.0, 0.0) == 5 / 7 - 1.0 + 2 / 7
    assert bs.F2(1.0, 2.0, 3.0 * (1 + 2.0 ** -41)) == bs.F2(1.0, 2.0, 3.0)   # the clamp: a triangle inside the closure slack


def test_tree_bispectrum_is_symmetric_under_leg_permutations():
    rng = np.random.default_rng(3)
    k = np.sort(rng.uniform(0.1, 1.0, (50, 3)), axis=1)
    k[:, 2] = np.minimum(k[:, 2], 0.98 * (k[:, 0] + k[:, 1]))
    P = rng.uniform(0.5, 2.0, (50, 3))
    ref = bs.tree_bispectrum(*k.T, *P.T)
    absum = 2 * sum(np.abs(bs.F2(k[:, i], k[:, j], k[:, 3 - i - j])) * P[:, i] * P[:, j] for i, j in ((0, 1), (1, 2), (2, 0)))
    for perm in itertools.permutations(range(3)):
        got = bs.tree_bispectrum(*k[:, perm].T, *P[:, perm].T)
        assert np.all(np.abs(got - ref) <= 16 * EPS * absum), perm


# ---------------------------------------------------------------- the factored cosine on squeezed triangles
def exact_mu(p, q, r):
    p, q, r = Fraction(p), Fraction(q), Fraction(r)
    return (r * r - p * p - q * q) / (2 * p * q)


def test_factored_cosine_against_exact_arithmetic():
    """|mu_float - mu_exact| <= 4 EPS (|(r-p)(r+p)| + q^2) / (2 p q) for the factored numerator, in every position of
    the short side and up to k_max / k_min = 3e4, against rational arithmetic on the same doubles; the naive numerator
    r^2 - p^2 - q^2 leaves that bound on the most squeezed triangle.  With the longer of (p, q) as p - the order F2 is
    evaluated in - the bound is itself a few ulp; with the short side as p it grows as k_max / k_min."""
    rng = np.random.default_rng(5)
    worst, worst_naive = 0.0, {}
    for ratio in (3.0, 1e2, 3e3, 3e4):
        for _ in range(40):
            short = rng.uniform(0.5, 2.0) * 1e-3
            long1 = short * ratio * rng.uniform(0.9, 1.0)
            long2 = long1 + short * rng.uniform(-0.99, 0.99)
            for p, q, r in itertools.permutations((short, long1, long2)):
                mu = ((r - p) * (r + p) - q * q) / (2.0 * p * q)
                naive = (r * r - p * p - q * q) / (2.0 * p * q)
                ex = exact_mu(p, q, r)
                bound = 4 * EPS * (abs((r - p) * (r + p)) + q * q) / (2.0 * p * q)
                err = abs(float(Fraction(mu) - ex))
                assert err <= bound, (p, q, r, err, bound)
                worst = max(worst, err / bound)
                if p >= q:          # the order F2 evaluates in: the bound itself is a few ulp, whatever the squeeze
                    assert bound <= 6 * EPS, (p, q, r, bound)
                worst_naive[ratio] = max(worst_naive.get(ratio, 0.0), abs(float(Fraction(naive) - ex)) / bound)
    print(f"factored: worst error / bound = {worst:.3g}; naive: {worst_naive}")
    assert worst_naive[3e4] > 1.0


def test_F2_tol_covers_the_factored_form():
    """The restatement's F2 bound against F2 of the exact cosine, evaluated in rational arithmetic."""
    rng = np.random.default_rng(6)
    for ratio in (1.5, 30.0, 3e4):
        for _ in range(30):
            short = rng.uniform(0.5, 2.0) * 1e-3
            long1 = short * ratio
            long2 = long1 + short * rng.uniform(-0.99, 0.99)
            for p, q, r in itertools.permutations((short, long1, long2)):
                mu = max(Fraction(-1), min(Fraction(1), exact_mu(p, q, r)))
                ex = Fraction(5, 7) + mu / 2 * (Fraction(p) / Fraction(q) + Fraction(q) / Fraction(p)) + Fraction(2, 7) * mu * mu
                val, tol = bm.F2_tol(p, q, r)
                assert abs(float(Fraction(float(val)) - ex)) <= tol, (p, q, r)


# ---------------------------------------------------------------- B_tree does not sit on a cancellation
def test_tree_bispectrum_has_no_cancellation_on_the_test_grid():
    """On the GPU tests' grid - all closing node triangles of geomspace(1e-3, 30, 48), the model's own P_lin_approx -
    sum |terms| / |sum terms| of B_tree stays below 20 and B_tree keeps its sign: its gate, a small multiple of EPS of
    the absolute sum, is a relative one."""
    ks = np.geomspace(1e-3, 30, 48)
    tri = bs.default_triangles(ks[None, :])
    assert tri.shape == (1664, 3)
    cosmo = hmvec_amd.Cosmology(engine="analytic", accuracy="low")
    for z in (0.2, 0.8, 1.4):
        P = cosmo.P_lin_approx(ks, np.array([z]))[0]
        k1, k2, k3 = (ks[tri[:, i]] for i in range(3))
        P1, P2, P3 = (P[tri[:, i]] for i in range(3))
        terms = np.stack([bs.F2(k1, k2, k3) * P1 * P2, bs.F2(k2, k3, k1) * P2 * P3, bs.F2(k3, k1, k2) * P3 * P1])
        total = bs.tree_bispectrum(k1, k2, k3, P1, P2, P3)
        ratio = 2 * np.abs(terms).sum(axis=0) / np.abs(total)
        print(f"z = {z}: worst sum|terms| / |sum| = {ratio.max():.3g}")
        assert ratio.max() <= 20.0
        assert np.all(total > 0)


# ---------------------------------------------------------------- damping, sample wavenumbers, closure
def test_damping_follows_the_function():
    k = np.concatenate([np.geomspace(1e-6, 1e3, 400), [0.0, 0.01 * math.sqrt(40.0), 0.0632456, 1e9]])
    D = bs.damping(k, 0.01)
    ref = -np.expm1(-(k / 0.01) ** 2)
    e = np.exp(-(k / 0.01) ** 2)
    assert np.all(np.abs(D - ref) <= 4 * EPS * e + 0.5 * EPS * ref)          # exp(-x) within 3 ulp (+ x's own rounding)
    assert D[-4] == 0.0 and D[-1] == 1.0 and np.all((D >= 0) & (D <= 1))
    assert bs.damping(0.3, 0.7) == bs.damping(np.array([0.3]), 0.7)[0]


def test_sample_wavenumbers_and_closure():
    ks = np.geomspace(1e-3, 30, 48)
    idx, frac = np.array([[0, 47, 3, 3]]), np.array([[0.0, 0.0, 0.25, 1.0]])
    k = bs.sample_wavenumbers(ks, idx, frac)
    assert k[0, 0] == ks[0] and k[0, 1] == ks[47] and k[0, 2] == 0.75 * ks[3] + 0.25 * ks[4] and k[0, 3] == ks[4]
    assert bs.closes(1.0, 2.0, 3.0) and bs.closes(3.0, 1.0, 2.0) and bs.closes(1.0, 3.0 * (1 + 2.0 ** -41), 2.0)
    assert not bs.closes(1.0, 2.0, 3.0 * (1 + 2.0 ** -39)) and not bs.closes(5.0, 1.0, 2.0)
    tri = bs.check_triangles(None, ks[None, :], [0.5])
    assert tri.dtype == np.int32 and tri.shape == (1664, 3) and np.all(tri[:, 0] <= tri[:, 1]) and np.all(tri[:, 1] <= tri[:, 2])
    assert np.all(bs.closes(*(ks[tri[:, i]] for i in range(3))))
    k2 = np.stack([ks, ks])
    k2[1, 5] *= 3.0
    with pytest.raises(ValueError, match=r"t = 1 does not close at z = 0\.9"):
        bs.check_triangles([[0, 0, 0], [5, 6, 6], [1, 1, 1]], k2, [0.1, 0.9])
    with pytest.raises(ValueError, match=r"t = 2 names sample .*0 \.\. n - 1 = 47"):
        bs.check_triangles([[0, 0, 0], [1, 1, 1], [1, 48, 1]], k2, [0.1, 0.9])
    with pytest.raises(ValueError, match="t = 0"):
        bs.check_triangles([[-1, 0, 0]], k2, [0.1, 0.9])
    with pytest.raises(ValueError, match=r"\(nt, 3\)"):
        bs.check_triangles([[0, 0]], k2, [0.1, 0.9])
    with pytest.raises(ValueError, match=r"\(nt, 3\)"):
        bs.check_triangles(np.zeros((2, 3)), k2, [0.1, 0.9])


# ---------------------------------------------------------------- cl_bispectrum's host tables
def stub_model():
    m = types.SimpleNamespace()
    m.zs = np.array([0.2, 0.8, 1.4])
    m.ks = np.geomspace(1e-3, 30, 48)
    m.comoving_radial_distance = lambda zs: 3000.0 * np.asarray(zs)
    m.h_of_z = lambda zs: 2.3e-4 * (1.0 + np.asarray(zs)) ** 1.5
    return m


def test_cl_bispectrum_host_tables():
    m = stub_model()
    ell = np.array([[200.0, 1000.0, 1000.0], [3000.0, 3000.0, 200.0], [1000.0, 3000.0, 2500.0]])
    W2 = np.array([0.5, 1.0, 0.8])
    tri, idx, frac, g = bs.limber_tables(m, ell, W1=2.0, W2=W2, W3=1)
    distinct = np.array([200.0, 1000.0, 2500.0, 3000.0])
    assert tri.dtype == np.int32 and np.array_equal(distinct[tri], ell)                      # the distinct-ell mapping
    assert idx.shape == frac.shape == (3, 4)
    chis = 3000.0 * m.zs
    k = (distinct[None, :] + 0.5) / chis[:, None]
    assert np.allclose(bs.sample_wavenumbers(m.ks, idx, frac), k, rtol=1e-14, atol=0)
    want = trapz_weights(m.zs) * m.h_of_z(m.zs) * 2.0 * W2 / chis ** 4
    assert np.allclose(g, want, rtol=8 * EPS, atol=0)
    with pytest.raises(ValueError, match=r"ell = 200000\.0"):
        bs.limber_tables(m, [[200.0, 200000.0, 200000.0]])
    with pytest.raises(ValueError, match=r"ell = 0\.0.*z = 0\.2"):
        bs.limber_tables(m, [[0.0, 500.0, 500.0]])                   # k = 0.5 / 600 below the grid at the first redshift
    with pytest.raises(ValueError, match=r"\(nt, 3\)"):
        bs.limber_tables(m, [200.0, 300.0, 400.0])
    with pytest.raises(ValueError, match="term"):
        bs.cl_bispectrum(m, ell, "nfw", term="4h")
    B = np.arange(24.0).reshape(3, 2, 4)
    assert np.array_equal(bs.pick_term(B, "total"), B[0] + B[1] + B[2]) and np.array_equal(bs.pick_term(B, "2h"), B[1])


# ---------------------------------------------------------------- declared, exported, bound
def test_entry_point_is_declared_exported_and_bound():
    with open(os.path.join(HERE, "..", "include", "hmgrid.h")) as f:
        header = f.read()
    m = re.search(r"int hmg_bispectrum\((.*?)\);", header, re.S)
    assert m, "hmg_bispectrum is not declared in include/hmgrid.h"
    args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")
    sig = nat.SIGNATURES["hmg_bispectrum"]
    assert len(args) == len(sig) == 25
    for a, t in zip(args, sig):
        a = a.strip()
        if "*" in a:
            assert t is C.c_void_p or issubclass(t, C._Pointer), a
        else:
            assert t is (C.c_double if a.startswith("double") else C.c_int), a
    assert os.path.exists(nat.LIB_PATH), "libhmgrid.so not built"
    assert hasattr(C.CDLL(nat.LIB_PATH), "hmg_bispectrum")
    assert "#define HMG_ABI_VERSION 10" in header and nat.ABI_VERSION == 10


def test_exports():
    for name in ("F2", "tree_bispectrum", "cl_bispectrum"):
        assert getattr(hmvec_amd, name) is getattr(bs, name) and name in hmvec_amd.__all__ and name in bs.__all__
    assert hmvec_amd.bispectrum is bs
    for name in ("get_bispectrum", "bispectrum_device"):
        assert callable(getattr(hmvec_amd.HaloModel, name))


# ---------------------------------------------------------------- refusals by name: before anything touches a device
def test_name_refusals_need_no_device():
    from hmvec_amd import spectra
    hods = {"g": dict(satellite_profile="nfw", central_profile=None), "g2": dict(satellite_profile="nfw", central_profile=None),
            "both": dict(satellite_profile="nfw", central_profile=None)}
    uk, pk = {"nfw", "both"}, {"y"}
    stub = types.SimpleNamespace(_resolve=lambda *names: [spectra.resolve(n, hods, uk, pk) for n in names])

    def call(*names):
        return hmvec_amd.HaloModel._bispectrum(stub, *names, None, None, True, None, None, None, None, True)

    with pytest.raises(NotImplementedError, match=r"\('g', 'g2', 'nfw'\).*third factorial moments"):
        call("g", "g2", "nfw")
    with pytest.raises(NotImplementedError, match=r"\('y', 'g', 'g'\)"):
        call("y", "g", "g")
    with pytest.raises(ValueError, match="'both'"):          # an HOD for the 1-halo lookup, a matter profile for the 2-halo one
        call("nfw", "both", "y")
    with pytest.raises(ValueError, match="nosuch"):
        call("nfw", "nosuch", "y")
