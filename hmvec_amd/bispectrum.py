"""Halo-model bispectrum of three tracers.

``HaloModel.bispectrum_device`` / ``get_bispectrum`` contract the 1-halo, 2-halo and 3-halo terms on the GPU over the
resident tensors.  This module holds the host side of the contract - the pieces that are plain arithmetic on a few
numbers and that the device follows operation for operation: the sample wavenumbers, the damping factor, the triangle
closure rule, the tree-level kernel ``F2`` and ``tree_bispectrum`` - and ``cl_bispectrum``, the Limber projection.
Linear halo bias only: there is no b_2 term.
"""
import numpy as np

from .cov import limber_samples
from .quadrature import trapz_weights

__all__ = ["F2", "tree_bispectrum", "cl_bispectrum"]

TERMS = ("1h", "2h", "3h", "total")
MAX_SAMPLES = 256
MAX_TRIANGLES = 1 << 20
CLOSURE_SLACK = 1.0 + 2.0 ** -40

_LOG2E = 1.4426950408889634
_LN2_HI = 6.93147180369123816490e-01          # 32 significant bits: n * _LN2_HI is exact for n < 2^20
_LN2_LO = 1.90821492927058770002e-10
_TAYLOR = [1.0 / 479001600.0, 1.0 / 39916800.0, 1.0 / 3628800.0, 1.0 / 362880.0, 1.0 / 40320.0, 1.0 / 5040.0, 1.0 / 720.0,
           1.0 / 120.0, 1.0 / 24.0, 1.0 / 6.0, 0.5, 1.0, 1.0]


def sample_wavenumbers(ks, idx, frac):
    """k_s of the contract: ks[idx] where frac == 0, else (1 - f) ks[idx] + f ks[idx + 1] as three rounded operations
    (node idx + 1 is not read where frac == 0).  The device forms the same bits."""
    ks = np.asarray(ks, dtype=np.float64)
    idx, frac = np.asarray(idx), np.asarray(frac, dtype=np.float64)
    k0, k1 = ks[idx], ks[np.minimum(idx + 1, ks.size - 1)]
    return np.where(frac == 0.0, k0, (1.0 - frac) * k0 + frac * k1)


def damping(k, kstar):
    """D = 1 - exp(-(k / kstar)^2) as the device evaluates it: a fixed sequence of separately rounded IEEE operations
    (bis_damping in kernels/bispectrum.hpp is the same sequence), so host and device agree to the bit.  (k/kstar)^2 > 40
    gives exactly 1; else exp(-x) = 2^-n exp(t), n = rint(x log2 e), t = -((x - n ln2_hi) - n ln2_lo), exp(t) by its
    Taylor polynomial of degree 13 in Horner form.  exp(-x) is within 3 ulp of the true value."""
    q = np.asarray(k, dtype=np.float64) / kstar
    x = q * q
    big = ~(x <= 40.0)
    x = np.where(big, 0.0, x)
    n = np.rint(x * _LOG2E)
    t = -((x - n * _LN2_HI) - n * _LN2_LO)
    p = np.full_like(x, 1.0 / 6227020800.0)
    for c in _TAYLOR:
        p = p * t + c
    return np.where(big, 1.0, 1.0 - np.ldexp(p, -n.astype(np.int64)))


def closes(k1, k2, k3):
    """The contract's closure rule: k_max <= (k_mid + k_min)(1 + 2^-40), elementwise."""
    hi = np.maximum(k1, np.maximum(k2, k3))
    lo = np.minimum(k1, np.minimum(k2, k3))
    mid = np.maximum(np.minimum(k1, k2), np.minimum(np.maximum(k1, k2), k3))
    return hi <= (mid + lo) * CLOSURE_SLACK


def F2(p, q, r):
    """The tree-level kernel F2(p, q; r) = 5/7 + mu/2 (p/q + q/p) + 2/7 mu^2 of the sides p, q of a closed triangle
    (p, q, r), mu = clamp(((r - p)(r + p) - q^2) / (2 p q), -1, 1) the cosine between them.  The numerator is factored
    on purpose: with r^2 - p^2 - q^2 the rounding error of a squeezed triangle grows as (k_max / k_min)^2.  F2 is
    symmetric in (p, q) and is evaluated with the longer of the two as p (the device does the same), which keeps mu
    within a few ulp for every order of the sides."""
    p, q, r = (np.asarray(v, dtype=np.float64) for v in (p, q, r))
    p, q = np.maximum(p, q), np.minimum(p, q)
    mu = np.clip(((r - p) * (r + p) - q * q) / (2.0 * p * q), -1.0, 1.0)
    return 5.0 / 7.0 + 0.5 * mu * (p / q + q / p) + (2.0 / 7.0) * mu * mu


def tree_bispectrum(k1, k2, k3, P1, P2, P3):
    """B_tree = 2 [F2(k1,k2;k3) P1 P2 + F2(k2,k3;k1) P2 P3 + F2(k3,k1;k2) P3 P1], P_i the linear spectrum at k_i."""
    return 2.0 * (F2(k1, k2, k3) * P1 * P2 + F2(k2, k3, k1) * P2 * P3 + F2(k3, k1, k2) * P3 * P1)


def default_triangles(ksamp):
    """All (i, j, l), i <= j <= l, of the n samples that close at every redshift; ksamp (nz, n)."""
    n = ksamp.shape[1]
    out = []
    for i in range(n):
        j, l = np.triu_indices(n - i)
        j, l = j + i, l + i
        ok = np.all(closes(ksamp[:, i:i + 1], ksamp[:, j], ksamp[:, l]), axis=0)
        out.append(np.stack([np.full(int(ok.sum()), i), j[ok], l[ok]], axis=1))
    return np.concatenate(out, axis=0).astype(np.int32)


def check_triangles(triangles, ksamp, zs):
    """The checked (nt, 3) int32 triangles of a request over the samples ksamp (nz, n); None: default_triangles.
    Everything that can be refused is, here, on the host."""
    n = ksamp.shape[1]
    if triangles is None:
        tri = default_triangles(ksamp)
        if tri.shape[0] < 1:
            raise ValueError("no triangle of the samples closes")
    else:
        tri = np.asarray(triangles)
        if tri.ndim != 2 or tri.shape[1] != 3 or not np.issubdtype(tri.dtype, np.integer):
            raise ValueError("triangles must be an (nt, 3) integer array of sample indices")
        if tri.shape[0] < 1:
            raise ValueError("triangles is empty: the bispectrum needs at least one triangle")
    if tri.shape[0] > MAX_TRIANGLES:
        raise ValueError(f"{tri.shape[0]} triangles; at most 2^20 = {MAX_TRIANGLES} are taken in one call: pass fewer "
                         f"triangles or samples")
    if tri.min() < 0 or tri.max() > n - 1:
        t = int(np.argwhere((tri < 0) | (tri > n - 1))[0][0])
        raise ValueError(f"triangle t = {t} names sample {tuple(int(v) for v in tri[t])}: indices must lie in "
                         f"0 .. n - 1 = {n - 1}")
    bad = ~closes(ksamp[:, tri[:, 0]], ksamp[:, tri[:, 1]], ksamp[:, tri[:, 2]])
    if bad.any():
        z, t = (int(v) for v in np.argwhere(bad)[0])
        k = [float(ksamp[z, s]) for s in tri[t]]
        raise ValueError(f"triangle t = {t} does not close at z = {float(np.asarray(zs).reshape(-1)[z])!r}: "
                         f"k = {k!r} has k_max > k_mid + k_min")
    return np.ascontiguousarray(tri, dtype=np.int32)


def limber_tables(model, ell_triangles, W1=1, W2=1, W3=1):
    """The host tables of cl_bispectrum: (tri, idx, frac, g).  The samples are the distinct multipoles of
    ell_triangles (nt, 3) through cov.limber_samples - tri (nt, 3) indexes them -, idx / frac (nz, n_distinct), and
    g[z] = trapz weight H W1 W2 W3 / chi^4 are the z weights of the device's sum.  A multipole whose Limber wavenumber
    leaves the model's grid at some redshift raises ValueError naming it."""
    ell = np.asarray(ell_triangles, dtype=np.float64)
    if ell.ndim != 2 or ell.shape[1] != 3 or ell.shape[0] < 1:
        raise ValueError("ell_triangles must be an (nt, 3) array of multipoles, nt >= 1")
    zs = np.asarray(model.zs, dtype=np.float64).reshape(-1)
    if zs.size < 2:
        raise ValueError("cl_bispectrum integrates over the model's redshifts: it needs at least two")
    ells, inv = np.unique(ell.reshape(-1), return_inverse=True)
    chis = np.asarray(model.comoving_radial_distance(zs), dtype=np.float64).reshape(-1)
    hzs = np.asarray(model.h_of_z(zs), dtype=np.float64).reshape(-1)
    idx, frac = limber_samples(ells, chis, model.ks, zs=zs)
    g = trapz_weights(zs) * hzs / chis ** 4
    for W in (W1, W2, W3):
        g = g * np.broadcast_to(np.asarray(W, dtype=np.float64), zs.shape)
    return inv.reshape(-1, 3).astype(np.int32), idx, frac, g


def pick_term(B, term):
    """A term of B (3, ...) = (1h, 2h, 3h); "total" is their sum in that order."""
    if term not in TERMS:
        raise ValueError(f"term must be one of {TERMS}, got {term!r}")
    return B[0] + B[1] + B[2] if term == "total" else B[TERMS.index(term)]


def cl_bispectrum(model, ell_triangles, name, name2=None, name3=None, W1=1, W2=1, W3=1, term="total", damping=True):
    """The Limber-projected bispectrum of three tracers at the multipole triangles ell_triangles (nt, 3), shape (nt,):

        B_l1l2l3 = trapz_z[ H(z) W1 W2 W3 / chi^4  B(z; (l1 + 1/2)/chi, (l2 + 1/2)/chi, (l3 + 1/2)/chi) ]

    on the model's own zs (at least two), H in 1/Mpc and chi in Mpc as in cov.cl_cov_1halo; the windows are scalars or
    (nz,) arrays.  B at the Limber wavenumbers is HaloModel.bispectrum_device's at interpolated samples (the distinct
    multipoles); a wavenumber outside the model's grid raises ValueError.  term: "1h", "2h", "3h" or "total".  The z sum
    is taken on the device, in z order."""
    if term not in TERMS:
        raise ValueError(f"term must be one of {TERMS}, got {term!r}")
    tri, idx, frac, g = limber_tables(model, ell_triangles, W1, W2, W3)
    _, Bz = model.bispectrum_device(name, name2, name3, triangles=tri, damping=damping, idx=idx, frac=frac, zweights=g,
                                    per_z=False)
    return pick_term(Bz.numpy(), term)
