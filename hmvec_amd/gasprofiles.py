"""Projected gas and pressure profiles on the GPU: the batched function of plain arrays behind
HaloModel.gas_sigma_1h_profiles, gas_delta_sigma_1h_profiles, tau_1h_profiles and y_1h_profiles.

``projected_gnfw`` works in the scaled units of the generalised NFW family f(x) = x^gamma (1 + x^alpha)^(-eta), truncated
at xcut: the line-of-sight projection F(s), its mean G(s) inside a disc of radius s, the excess G - F, and F convolved with
a circular Gaussian (a telescope beam, or Rayleigh-distributed miscentring).  The Battaglia gas density and pressure
profiles are members of the family.  The kernels are in hmvec_amd/csrc/kernels/gasproj.hpp.
"""
import ctypes as C

import numpy as np

from . import _native as nat
from ._native import as_device as _dev, context_or_default as _context

__all__ = ["projected_gnfw", "quadrature_table"]

_KINDS = {"sigma": nat.GNFW_SIGMA, "mean": nat.GNFW_MEAN, "excess": nat.GNFW_EXCESS}
# testing: alpha == 1 rows through the general evaluation instead of their shorter one
_force_general = False


def _per_row(name, a, n, positive):
    a = np.atleast_1d(np.asarray(a, dtype=np.float64)).ravel()
    if not np.all(np.isfinite(a)) or (positive and np.any(a <= 0)):
        raise ValueError(f"{name} must be finite" + (" and positive" if positive else ""))
    if a.size == 1 and n > 1:
        a = np.full(n, a[0])
    if a.size != n:
        raise ValueError(f"{name} must be a scalar or have one entry per row ({n}), got {a.size}")
    return a


def projected_gnfw(x, alpha, gamma, eta, xcut, kind="sigma", smooth=None, *, ctx=None):
    """Projected profile out[i, j] of row i, f(x) = x^gamma (1 + x^alpha[i])^(-eta[i]) for x <= xcut[i] and 0 beyond, at
    the projected radius x[i, j] (or x[j]) in the same scaled units.

    kind "sigma": F(s) = 2 int_0^sqrt(xcut^2 - s^2) f(sqrt(s^2 + l^2)) dl, exactly 0 for s >= xcut;
    kind "mean":  G(s) = (2/s^2) int_0^s F(s') s' ds', the mass inside the cylinder of radius s over pi s^2;
    kind "excess": G(s) - F(s).
    alpha, eta, xcut: length-N arrays (a scalar is broadcast); gamma: one number for the call; x: (N, nR) or (nR,).
    smooth: None, or a non-negative scalar or length-N array of Gaussian widths in the same units (kind "sigma" only):
    F convolved with a circular Gaussian of that width; rows with width 0 take the unsmoothed route, bit for bit.
    Requires alpha > 0, gamma > -1, alpha eta - gamma > 1, xcut > 0.  Returns an (N, nR) float64 array."""
    n, nr, per_row, x, alpha, gamma, eta, xcut, sig = _checked(x, alpha, gamma, eta, xcut, kind, smooth)
    if n == 0 or nr == 0:
        return np.empty((n, nr))
    ctx = _context(ctx)
    out, plain = None, None
    if sig is None or not np.all(sig > 0):
        out = _launch(ctx, n, nr, per_row, x, alpha, gamma, eta, xcut, kind, sig, True)
        if sig is None:
            return out.numpy()
        plain = out.numpy()
    res = _launch(ctx, n, nr, per_row, x, alpha, gamma, eta, xcut, kind, sig, False, out).numpy()
    if plain is not None:
        res = np.where((sig > 0)[:, None], res, plain)
    return res


def projected_gnfw_device(x, alpha, gamma, eta, xcut, smooth=None, *, ctx):
    """projected_gnfw(kind="sigma") left on the device: the (N, nR) DeviceArray of the context, for a caller that
    contracts the profiles there (HaloModel.get_y_char_exponent).  Same checks; smooth must be None or positive in every
    row (no mixing of the two routes, which the host function does with a copy of each)."""
    n, nr, per_row, x, alpha, gamma, eta, xcut, sig = _checked(x, alpha, gamma, eta, xcut, "sigma", smooth)
    if n == 0 or nr == 0:
        raise ValueError("no rows or no radii")
    if sig is not None and not np.all(sig > 0):
        raise ValueError("smooth must be positive in every row, or None")
    return _launch(ctx, n, nr, per_row, x, alpha, gamma, eta, xcut, "sigma", sig, sig is None)


def _launch(ctx, n, nr, per_row, x, alpha, gamma, eta, xcut, kind, sig, plain, out=None):
    """One launch: the unsmoothed kernel (plain) or the smoothed one with the widths sig, where a row without a width gets
    one (the quadrature needs a positive width; the caller takes that row's unsmoothed values)."""
    flag = nat.GNFW_GENERAL if _force_general else 0
    d_al, d_et, d_xc, d_x = (_dev(ctx, a) for a in (alpha, eta, xcut, x))
    out = ctx.empty((n, nr)) if out is None else out
    if plain:
        ctx.call("hmg_gnfw_projected", n, nr, per_row, _KINDS[kind] | flag, d_al.ptr, d_et.ptr, d_xc.ptr, gamma, d_x.ptr,
                 out.ptr)
    else:
        d_sig = _dev(ctx, np.where(sig > 0, sig, 1.0))
        ctx.call("hmg_gnfw_projected_smooth", n, nr, per_row, _KINDS[kind] | flag, d_al.ptr, d_et.ptr, d_xc.ptr, gamma,
                 d_x.ptr, d_sig.ptr, out.ptr)
    return out


def _checked(x, alpha, gamma, eta, xcut, kind, smooth):
    """The checks of projected_gnfw: (n, nr, per_row, x, alpha, gamma, eta, xcut, sig), sig None or the widths per row."""
    if kind not in _KINDS:
        raise ValueError(f"kind must be one of {sorted(_KINDS)}, got {kind!r}")
    sizes = [np.size(a) for a in (alpha, eta, xcut)]
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0] if x.ndim == 2 else max(sizes + [1 if smooth is None else np.size(smooth)])
    alpha = _per_row("alpha", alpha, n, True)
    eta = _per_row("eta", eta, n, False)
    xcut = _per_row("xcut", xcut, n, True)
    gamma = float(gamma)
    if not np.isfinite(gamma) or gamma <= -1:
        raise ValueError("gamma must be finite and above -1")
    if np.any(alpha * eta - gamma <= 1):
        raise ValueError("the profile must fall faster than 1/x: alpha * eta - gamma > 1")
    if not np.all(np.isfinite(x)) or np.any(x <= 0):
        raise ValueError("x must be finite and positive")
    if x.ndim == 1:
        per_row = 0
    elif x.ndim == 2 and x.shape[0] == n:
        per_row = 1
    else:
        raise ValueError(f"x must be (nR,) or ({n}, nR), got {x.shape}")
    sig = None
    if smooth is not None:
        sig = np.atleast_1d(np.asarray(smooth, dtype=np.float64)).ravel()
        if sig.size == 1 and n > 1:
            sig = np.full(n, sig[0])
        if sig.size != n or not np.all(np.isfinite(sig)) or np.any(sig < 0):
            raise ValueError("smooth must be non-negative, a scalar or one entry per row")
        if not np.any(sig > 0):
            sig = None
    if sig is not None and kind != "sigma":
        raise NotImplementedError("smoothing is implemented for kind='sigma' only: the disc average of a convolved "
                                  "profile needs a further level of quadrature")
    return n, x.shape[-1], per_row, x, alpha, gamma, eta, xcut, sig


def quadrature_table():
    """The node table the kernels read, as the host builds it (no GPU needed): dict of u, w (64 Gauss-Legendre nodes and
    weights on [0, 1]), v2 = u^2, lv2 = 2 ln u, wv = 2 u w (the inner sphere, r = b v^2), and sg, cg, wj of the smoothing
    (32-node rule U, W: sin^2(pi U / 2), cos^2(pi U / 2), W (pi/2) sin(pi U))."""
    buf = (C.c_double * nat.GNFW_TABLE_DOUBLES)()
    nat.check(nat.load().hmg_gnfw_quad_table(buf))
    t = np.array(buf)
    out, at = {}, 0
    for name, size in (("u", 64), ("w", 64), ("v2", 64), ("lv2", 64), ("wv", 64), ("sg", 32), ("cg", 32), ("wj", 32)):
        out[name] = t[at:at + size].copy()
        at += size
    return out
