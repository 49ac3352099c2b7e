"""Host-side checks of the trispectrum and covariance code, no GPU: the numpy restatement the GPU
tests compare with (tests/helpers/trispectrum_model.py) against a triple Python loop; the Limber sample tables
(hmvec_amd.cov.limber_samples); the Gaussian covariance mirror against a fixture recorded from the unmodified
reference (tests/golden/cov_gaussian.npz, tools/make_golden.py); and that the new entry point is declared and bound."""
import ctypes as C
import os
import re
import sys
import types

import numpy as np
import pytest

import hmvec_amd
from hmvec_amd import _native as nat
from hmvec_amd import cov
from hmvec_amd.quadrature import trapz_weights

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import trispectrum_model as tm  # noqa: E402


# ---------------------------------------------------------------- the restatement against plain loops
def toy_model():
    """A stand-in with the facade's host arrays on a 2 x 5 x 6 grid: an NFW-like matter profile, a second matter
    profile, a pressure profile, two HODs (one with a central profile)."""
    rng = np.random.default_rng(7)
    nz, nm, nk = 2, 5, 6
    h = types.SimpleNamespace()
    h.zs, h.ms, h.ks = np.array([0.3, 1.1]), np.geomspace(1e12, 1e15, nm), np.geomspace(1e-2, 5.0, nk)
    h.p = {"kstar_damping": 0.7}
    h.nzm = rng.uniform(0.5, 2.0, (nz, nm)) * 1e-18 * (h.ms / 1e13) ** -1.9
    h.rho_matter_z = lambda z: np.array([3.9e10])
    h.uk_profiles = {"nfw": rng.uniform(0.1, 1.0, (nz, nm, nk)), "cen": rng.uniform(0.5, 1.0, (nz, nm, nk))}
    h.pk_profiles = {"y": rng.uniform(-0.2, 1.0, (nz, nm, nk)) * 1e-3, "y2": rng.uniform(0.1, 1.0, (nz, nm, nk))}
    def hod(cen):
        return dict(Nc=rng.uniform(0, 1, (nz, nm)), Ns=rng.uniform(0, 5, (nz, nm)), NcNs=rng.uniform(0, 3, (nz, nm)),
                    NsNsm1=rng.uniform(0, 9, (nz, nm)), ngal=rng.uniform(1e-4, 1e-3, nz), satellite_profile="nfw",
                    central_profile=cen)
    h.hods = {"g": hod(None), "gc": hod("cen")}
    return h


def loop_square(h, a, b, z, m, k):
    def w(nm_):
        if nm_ in h.hods:
            d = h.hods[nm_]
            uc = 1.0 if d["central_profile"] is None else h.uk_profiles[d["central_profile"]][z, m, k]
            return (uc * d["Nc"][z, m] + h.uk_profiles[d["satellite_profile"]][z, m, k] * d["Ns"][z, m]) / d["ngal"][z]
        if nm_ in h.uk_profiles:
            return h.ms[m] * h.uk_profiles[nm_][z, m, k] / h.rho_matter_z(0)[0]
        return h.pk_profiles[nm_][z, m, k]
    if a in h.hods and b in h.hods:
        d = h.hods[a]
        uc = 1.0 if d["central_profile"] is None else h.uk_profiles[d["central_profile"]][z, m, k]
        us = h.uk_profiles[d["satellite_profile"]][z, m, k]
        return (2 * uc * us * d["NcNs"][z, m] + d["NsNsm1"][z, m] * us ** 2) / d["ngal"][z] ** 2
    if a in h.pk_profiles and b in h.pk_profiles:
        return h.pk_profiles[a][z, m, k] ** 2
    return w(a) * w(b)


@pytest.mark.parametrize("names", [("nfw", "nfw", "nfw", "nfw"), ("g", "g", "g", "g"), ("gc", "g", "nfw", "nfw"),
                                   ("g", "nfw", "gc", "nfw"), ("y", "y2", "y2", "y"), ("gc", "y", "nfw", "cen")])
def test_restatement_against_triple_loop(names):
    h = toy_model()
    nz, nm, nk = h.nzm.shape + (h.ks.size,)
    idx = np.array([[0, 2, 5, 4], [5, 1, 1, 3]])
    frac = np.array([[0.0, 0.25, 0.0, 1.0], [0.0, 0.5, 0.0, 0.125]])
    scale = np.array([[1.0, 2.0, 0.0, -1.5], [0.5, 1.0, 1.0, 3.0]])
    T, A = tm.trispectrum(h, *names, idx=idx, frac=frac, scale=scale, damping=False)
    wm = trapz_weights(h.ms)
    ref, aref = np.zeros_like(T), np.zeros_like(T)

    def s(a, b, z, m, i):
        f, left = frac[z, i], loop_square(h, a, b, z, m, idx[z, i])
        return scale[z, i] * (left if f == 0 else (1 - f) * left + f * loop_square(h, a, b, z, m, idx[z, i] + 1))

    for z in range(nz):
        for i in range(idx.shape[1]):
            for j in range(idx.shape[1]):
                terms = [wm[m] * h.nzm[z, m] * s(names[0], names[1], z, m, i) * s(names[2], names[3], z, m, j)
                         for m in range(nm)]
                ref[z, i, j], aref[z, i, j] = sum(terms), sum(abs(t) for t in terms)
    assert np.all(np.abs(T - ref) <= tm.gate(aref, nm))
    assert np.allclose(A, aref, rtol=1e-12, atol=0)
    assert np.all(T[0, 2, :] == 0) and np.all(T[0, :, 2] == 0)          # the zero scale of z 0, sample 2


def test_restatement_damping_and_node_mode():
    h = toy_model()
    T, _ = tm.trispectrum(h, "g", "nfw", kindex=[1, 4], damping=True)
    T0, _ = tm.trispectrum(h, "g", "nfw", kindex=[1, 4], damping=False)
    D = 1 - np.exp(-(h.ks[[1, 4]] / h.p["kstar_damping"]) ** 2)
    assert np.allclose(T, T0 * D[None, :, None] * D[None, None, :], rtol=1e-14, atol=0)
    # the diagonal of a pair with itself is the mass integral of the squared square term: P_1h's integrand, squared
    S = tm.square_term(h, "g", "nfw")[:, :, [1, 4]]
    diag = np.einsum("zm,zmi->zi", trapz_weights(h.ms)[None, :] * h.nzm, S ** 2)
    assert np.allclose(np.einsum("zii->zi", T0), diag, rtol=1e-13, atol=0)


# ---------------------------------------------------------------- limber_samples
def test_limber_samples_nodes_and_interior():
    # a dyadic grid, so that (ell + 1/2) / chi lands on the grid points exactly: every node, the last one included,
    # is found as itself with f = 0 (idx = nk - 1, f = 0: the node to its right is never read)
    ks2 = 2.0 ** np.arange(-10, 5)
    ells = ks2 * 1024.0 - 0.5
    assert np.array_equal((ells + 0.5) / 1024.0, ks2)
    idx, frac = cov.limber_samples(ells, [1024.0], ks2)
    assert idx.dtype == np.int32 and idx.shape == frac.shape == (1, ks2.size)
    assert np.array_equal(idx[0], np.arange(ks2.size)) and np.all(frac == 0.0)
    assert idx[0, -1] == ks2.size - 1 and frac[0, -1] == 0.0
    # between the points of the model grid of the GPU tests, two redshifts
    ks = np.geomspace(1e-3, 30, 48)
    chis = np.array([800.0, 2500.0])
    ells = np.array([10.0, 200.0, 1000.0, 3000.0, 20000.0])
    idx, frac = cov.limber_samples(ells, chis, ks)
    assert idx.shape == frac.shape == (2, 5)
    assert np.all((frac >= 0) & (frac < 1)) and np.all((idx >= 0) & (idx < ks.size - 1))
    k = (ells[None, :] + 0.5) / chis[:, None]
    assert np.all((ks[idx] <= k) & (k < ks[idx + 1]))
    assert np.allclose((1 - frac) * ks[idx] + frac * ks[idx + 1], k, rtol=1e-14, atol=0)


def test_limber_samples_refuses_wavenumbers_off_the_grid():
    ks = np.geomspace(1e-3, 30, 48)
    with pytest.raises(ValueError, match=r"ell = 1\.0.*z = 0\.5"):
        cov.limber_samples([1.0, 500.0], [3000.0], ks, zs=[0.5])            # k = 5e-4 below the grid
    with pytest.raises(ValueError, match="ell = 40000.0"):
        cov.limber_samples([500.0, 40000.0], [1000.0], ks)                   # k = 40 above it
    with pytest.raises(ValueError, match="redshift index 0"):
        cov.limber_samples([500.0], [0.0, 1000.0], ks)                       # chi = 0 (z = 0)


# ---------------------------------------------------------------- the Gaussian covariance against the reference
@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(HERE, "golden", "cov_gaussian.npz")) as f:
        return {k: f[k] for k in f.files}


def same(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref)
    return got.shape == ref.shape and np.allclose(got, ref, rtol=1e-13, atol=0, equal_nan=True)


def test_cov_free_functions(golden):
    g = golden
    assert same(cov.shot_noise(g["ngal"]), g["shot_noise"])
    assert same(cov.lensing_shape_noise(g["ngal"]), g["shape_noise_default"])
    assert same(cov.lensing_shape_noise(g["ngal"], 0.26), g["shape_noise_0p26"])
    binned = cov.bin_annuli(g["ells"], g["cls_holes"], g["edges_holes"])
    assert np.isnan(g["binned_holes"]).sum() == 1 and same(binned, g["binned_holes"])
    assert cov.default_binning is cov.bin_annuli


@pytest.mark.parametrize("i", [0, 1, 2])
def test_gaussian_cov_against_reference(golden, i):
    g = golden
    gc = cov.GaussianCov(g[f"e{i}_edges"])
    gc.add_cls("k", "k", g["ells"], g["cls_kk"], g["ellsn"], g["ncls_kk"])
    gc.add_cls("g", "g", g["ells"], g["cls_gg"], g["ellsn"], g["ncls_gg"])
    gc.add_cls("k", "g", g["ells"], g["cls_kg"])
    assert same(gc.ells, g[f"e{i}_ells"]) and same(gc.ls, g[f"e{i}_ls"]) and same(gc.dls, g[f"e{i}_dls"])
    for pair in ("kk", "gg", "kg", "gk"):
        assert same(gc.get_scls(*pair), g[f"e{i}_scls_{pair}"]), pair
        assert same(gc.get_ncls(*pair), g[f"e{i}_ncls_{pair}"]), pair
        assert same(gc.get_tcls(*pair), g[f"e{i}_tcls_{pair}"]), pair
    # the quirk: stored as k_g, asked for as g_k -> 0; no noise was given for k_g -> 0
    assert gc.get_scls("g", "k") == 0 and gc.get_ncls("k", "g") == 0 and np.all(gc.get_scls("k", "g") > 0)
    for o in g["orders"]:
        assert same(gc.get_cov(*str(o), float(g["fsky"])), g[f"e{i}_cov_{o}"]), o
    # ... which get_cov inherits: Cov(kk, gg) = 2 C_kg^2 / ..., Cov(gg, kk) looks k_g up as g_k and is 0
    assert np.all(g[f"e{i}_cov_kkgg"] > 0) and np.all(g[f"e{i}_cov_ggkk"] == 0)
    assert np.all(gc.get_cov("g", "g", "k", "k", 0.4) == 0)
    with pytest.raises(AssertionError):
        gc.add_cls("g", "k", g["ells"], g["cls_kg"])                         # the other order of a stored pair
    with pytest.raises(AssertionError):
        gc.add_cls("k_1", "g", g["ells"], g["cls_kg"])


# ---------------------------------------------------------------- declared, bound, exported
def test_entry_point_is_declared_and_bound():
    with open(os.path.join(HERE, "..", "include", "hmgrid.h")) as f:
        header = f.read()
    m = re.search(r"int hmg_trispectrum_1h\((.*?)\);", header, re.S)
    assert m, "hmg_trispectrum_1h is not declared in include/hmgrid.h"
    args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")
    sig = nat.SIGNATURES["hmg_trispectrum_1h"]
    assert len(args) == len(sig) == 19
    for a, t in zip(args, sig):
        a = a.strip()
        if "*" in a:
            assert t is C.c_void_p or issubclass(t, C._Pointer), a
        else:
            assert t is (C.c_double if a.startswith("double") else C.c_int), a
    assert "#define HMG_ABI_VERSION 10" in header and nat.ABI_VERSION == 10


def test_exports():
    for name in ("GaussianCov", "bin_annuli", "shot_noise", "lensing_shape_noise", "cl_cov_1halo", "limber_samples"):
        assert getattr(hmvec_amd, name) is getattr(cov, name) and name in hmvec_amd.__all__
    assert not hasattr(cov, "KnoxCov")
    for name in ("get_trispectrum_1halo", "trispectrum_device"):
        assert callable(getattr(hmvec_amd.HaloModel, name))
