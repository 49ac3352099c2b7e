"""Configuration-space statistics of halo-model spectra on the GPU.

``xi_from_power`` is the correlation function of a tabulated spectrum, defined exactly rather than by a quadrature in
k r: with f_i = k_i P_i and f~ the piecewise-linear interpolant of f on [ks[0], ks[-1]] (zero outside),

    xi(r) = 1/(2 pi^2 r) int f~(k) sin(k r) dk,

the integral taken in closed form panel by panel.  It stands behind ``HaloModel.get_xi`` and ``HaloModel.get_xi_all``.

``projected_from_power`` gives the Hankel transforms of orders 0 and 2, defined in the same way:
with P~ the interpolant of P that is linear in k^2 on each panel of [ks[0], ks[-1]] (zero outside),

    W_0(R) = 1/(2 pi) int k P~(k) J0(k R) dk,      W_2(R) = 1/(2 pi) int k P~(k) J2(k R) dk,

again exact panel by panel.  W_0 of P_gg is w_p(r_p) with pi_max -> infinity; rho_m0 W_0 and rho_m0 W_2 of P_gm are
Sigma(R) and Delta Sigma(R).  It stands behind ``HaloModel.get_wp``, ``get_surface_density``,
``get_excess_surface_density`` and their ``_all`` forms.  The kernels are in hmvec_amd/csrc/kernels/realspace.hpp.
"""
import numpy as np

from . import _native as nat
from ._native import as_device as _dev, context_or_default as _context

__all__ = ["xi_from_power", "projected_from_power"]


def check_ks(ks):
    """The k grid of a transform as a float64 vector: at least two finite, positive, strictly increasing values."""
    ks = np.asarray(ks, dtype=np.float64)
    if ks.ndim != 1 or ks.size < 2:
        raise ValueError("ks must be a vector of at least two wavenumbers")
    if not np.all(np.isfinite(ks)) or np.any(ks <= 0) or not np.all(np.diff(ks) > 0):
        raise ValueError("ks must be finite, positive and strictly increasing")
    return ks


def check_rs(rs, what="rs"):
    """The radii (`what`: their name in a message) of a transform as a float64 vector of finite, positive values (may
    be empty)."""
    rs = np.atleast_1d(np.asarray(rs, dtype=np.float64))
    if rs.ndim != 1:
        raise ValueError(f"{what} must be a scalar or a vector")
    if not np.all(np.isfinite(rs)) or np.any(rs <= 0):
        raise ValueError(f"{what} must be finite and positive")
    return rs


def transform_rows(ctx, d_ks, d_P, rows, nk, rs):
    """xi of `rows` device-resident rows of nk values at the checked radii rs (non-empty): one launch, a (rows, nr)
    host array."""
    out = ctx.empty((rows, rs.size))
    d_rs = ctx.upload(rs)
    ctx.call("hmg_xi_transform", rows, nk, rs.size, d_ks.ptr, d_P.ptr, d_rs.ptr, out.ptr)
    return out.numpy()


def check_order(order):
    """The orders of a Hankel-transform request as a tuple: 0, 2 or (0, 2)."""
    orders = tuple(order) if isinstance(order, (tuple, list)) else (order,)
    if orders not in ((0,), (2,), (0, 2)) or any(isinstance(o, bool) or not isinstance(o, (int, np.integer)) for o in orders):
        raise ValueError(f"order must be 0, 2 or (0, 2), got {order!r}")
    return orders


def hankel_rows(ctx, d_ks, d_P, rows, nk, rs, orders):
    """W_n, n in `orders` ((0,), (2,) or (0, 2)), of `rows` device-resident rows of nk values at the checked radii rs
    (non-empty): one launch, a tuple of (rows, nr) host arrays in the order of `orders`."""
    outs = {n: ctx.empty((rows, rs.size)) for n in orders}
    d_rs = ctx.upload(rs)
    ctx.call("hmg_hankel_transform", rows, nk, rs.size, d_ks.ptr, d_P.ptr, d_rs.ptr,
             outs[0].ptr if 0 in outs else None, outs[2].ptr if 2 in outs else None)
    return tuple(outs[n].numpy() for n in orders)


def _request(ks, P, rs, what="rs"):
    """The checks xi_from_power, projected_from_power and angular_from_power (whose radii are angles: `what`) share,
    all before any launch: (ks, P, rs, lead, rows) with
    ks and rs checked, P a DeviceArray or a finite float64 host array of nk values per row, lead its leading shape."""
    ks = check_ks(ks)
    nk = ks.size
    if isinstance(P, nat.DeviceArray):
        shape = P.shape
    else:
        P = np.asarray(P, dtype=np.float64)
        shape = P.shape
    if not 1 <= len(shape) <= 3 or shape[-1] != nk:
        raise ValueError(f"P must have shape ({nk},), (nz, {nk}) or (n, nz, {nk}), got {tuple(shape)}")
    if not isinstance(P, nat.DeviceArray) and not np.all(np.isfinite(P)):
        raise ValueError("P must be finite")
    rs = check_rs(rs, what)
    lead = tuple(shape[:-1])
    return ks, P, rs, lead, int(np.prod(lead, dtype=np.int64))


def _resident(ks, P, ctx):
    """The context of a checked request and its k grid and rows on that context's device."""
    ctx = P.ctx if ctx is None and isinstance(P, nat.DeviceArray) else _context(ctx)
    return ctx, ctx.upload(ks), _dev(ctx, P)


def xi_from_power(ks, P, rs, *, ctx=None):
    """Correlation function xi[..., j] at radius rs[j] of the spectra P[..., :] tabulated on ks.

    ks: (nk,) with nk >= 2, finite, positive, strictly increasing.  P: (nk,), (nz, nk) or (n, nz, nk), finite, as a
    host array or a DeviceArray (a resident spectrum is taken as it is: its shape is checked, its values stay on the
    device).  rs: radii, finite and positive; the units are the inverse of those of ks.  Returns a float64 array of
    P's leading shape with len(rs) last.  Anything else raises ValueError before a launch."""
    ks, P, rs, lead, rows = _request(ks, P, rs)
    if rs.size == 0 or rows == 0:
        return np.empty(lead + (rs.size,))
    ctx, d_ks, d_P = _resident(ks, P, ctx)
    return transform_rows(ctx, d_ks, d_P, rows, ks.size, rs).reshape(lead + (rs.size,))


def projected_from_power(ks, P, rs, order=0, *, ctx=None):
    """Hankel transform W_order[..., j] at radius rs[j] of the spectra P[..., :] tabulated on ks:
    W_n(R) = 1/(2 pi) int k P~(k) Jn(k R) dk with P~ linear in k^2 between the grid points and zero outside the grid.

    ks, P, rs and ctx as for xi_from_power, with the same checks.  order: 0 (w_p for pi_max -> infinity, Sigma / rho_m0),
    2 (Delta Sigma / rho_m0) or (0, 2) (both from one launch; each is bit for bit the single-order result).  Returns a
    float64 array of P's leading shape with len(rs) last, or a pair of them for (0, 2)."""
    orders = check_order(order)
    ks, P, rs, lead, rows = _request(ks, P, rs)
    if rs.size == 0 or rows == 0:
        outs = tuple(np.empty(lead + (rs.size,)) for _ in orders)
    else:
        ctx, d_ks, d_P = _resident(ks, P, ctx)
        outs = tuple(o.reshape(lead + (rs.size,)) for o in hankel_rows(ctx, d_ks, d_P, rows, ks.size, rs, orders))
    return outs if len(orders) == 2 else outs[0]
