"""Numpy restatement of the 1-halo trispectrum from a HaloModel's host arrays alone:
uk_profiles / pk_profiles / hods entries, nzm, ms and the trapezoid weights in ms.  The tensors it reads are produced by
code the trispectrum does not touch and that is gated against the reference elsewhere; what a comparison with this
tests is the device contraction and its loader.

    T[z,i,j] = sum_m wm[m] nzm[z,m] s_ab[z,m,i] s_cd[z,m,j]
    s_ab[z,m,i] = scale[z,i] ((1 - f) S_ab(z,m,k_idx) + f S_ab(z,m,k_idx+1))        (node idx + 1 not read where f == 0)

and A[z,i,j], the same sum over absolute values, which scales the gate

    |T_got - T_ref| <= (nm + 32) 2^-52 A:

each side adds nm terms in some order, and each term carries at most about two dozen roundings (the two linear forms,
the interpolation, the scale, the weight and the products), so each side is within (nm + 32) 2^-53 A of the exact sum."""
import numpy as np

from hmvec_amd.quadrature import trapz_weights

EPS = 2.0 ** -52


def _kind(h, name):
    """What the 1-halo lookup finds (hmvec/hmvec.py:516-523): hods, then matter profiles, then pressure profiles."""
    if name in h.hods:
        return "h"
    if name in h.uk_profiles:
        return "m"
    if name in h.pk_profiles:
        return "p"
    raise ValueError(name)


def _hod_parts(h, name):
    hod = h.hods[name]
    uc = 1.0 if hod["central_profile"] is None else h.uk_profiles[hod["central_profile"]]
    return hod, uc, h.uk_profiles[hod["satellite_profile"]]


def _weight(h, name):
    kind = _kind(h, name)
    if kind == "h":
        hod, uc, us = _hod_parts(h, name)
        return (uc * hod["Nc"][..., None] + us * hod["Ns"][..., None]) / hod["ngal"][..., None, None]
    if kind == "m":
        return h.ms[None, :, None] * h.uk_profiles[name] / float(h.rho_matter_z(0)[0])
    return h.pk_profiles[name]


def square_term(h, a, b):
    """S_ab[z,m,k]: what get_power_1halo(a, b) integrates, first-name-only rules included."""
    ka, kb = _kind(h, a), _kind(h, b)
    if ka == "h" and kb == "h":
        hod, uc, us = _hod_parts(h, a)
        return ((2.0 * uc * us * hod["NcNs"][..., None] + hod["NsNsm1"][..., None] * us ** 2.0)
                / hod["ngal"][..., None, None] ** 2.0)
    if ka == "p" and kb == "p":
        return h.pk_profiles[a] ** 2.0
    return _weight(h, a) * _weight(h, b)


def sampled(S, idx, frac, scale):
    """s[z,m,i] of S[z,m,k] at the (nz, n) tables."""
    nz, nm, nk = S.shape
    zi = np.arange(nz)[:, None, None]
    mi = np.arange(nm)[None, :, None]
    left = S[zi, mi, idx[:, None, :]]
    right = S[zi, mi, np.minimum(idx + 1, nk - 1)[:, None, :]]
    f = frac[:, None, :]
    s = np.where(f == 0.0, left, (1.0 - f) * left + f * np.where(f == 0.0, 0.0, right))
    return scale[:, None, :] * s


def tables(h, kindex=None, idx=None, frac=None, scale=None, damping=True):
    """The (nz, n) tables HaloModel.trispectrum_device makes of the same arguments."""
    nz, nk = h.zs.size, h.ks.size
    if idx is None:
        idx = np.arange(nk) if kindex is None else np.asarray(kindex)
    idx = np.broadcast_to(np.atleast_2d(np.asarray(idx)), (nz, np.asarray(idx).shape[-1]))
    n = idx.shape[1]
    frac = np.zeros((nz, n)) if frac is None else np.broadcast_to(np.asarray(frac, dtype=float), (nz, n))
    scale = np.ones((nz, n)) if scale is None else np.broadcast_to(np.asarray(scale, dtype=float), (nz, n))
    if damping:
        k = np.where(frac == 0.0, h.ks[idx], (1.0 - frac) * h.ks[idx] + frac * h.ks[np.minimum(idx + 1, nk - 1)])
        scale = scale * (1.0 - np.exp(-(k / h.p["kstar_damping"]) ** 2.0))
    return idx, frac, scale


def trispectrum(h, a, b=None, c=None, d=None, **kw):
    """(T, A), each (nz, n, n); arguments as HaloModel.trispectrum_device's."""
    b = a if b is None else b
    c, d = (a if c is None else c), (b if d is None else d)
    idx, frac, scale = tables(h, **kw)
    return contract(h.nzm, h.ms, sampled(square_term(h, a, b), idx, frac, scale),
                    sampled(square_term(h, c, d), idx, frac, scale))


def contract(nzm, ms, s_ab, s_cd):
    w = trapz_weights(ms)[None, :] * nzm
    T = np.einsum("zm,zmi,zmj->zij", w, s_ab, s_cd, optimize=True)
    A = np.einsum("zm,zmi,zmj->zij", np.abs(w), np.abs(s_ab), np.abs(s_cd), optimize=True)
    return T, A


def gate(A, nm):
    return (nm + 32) * EPS * A


def zsum(g, T, A, nm):
    """(Tz, its gate): sum_z g[z] T[z] and the bound of the definition - the gate of T summed with |g|, plus
    nz 2^-53 of the absolute sum."""
    g = np.asarray(g, dtype=float)
    absum = np.einsum("z,zij->ij", np.abs(g), A)
    return np.einsum("z,zij->ij", g, T), (nm + 32) * EPS * absum + g.size * 0.5 * EPS * absum
