"""Angular correlation functions of halo-model spectra on the GPU: w(theta) of P_gg,
gamma_t(theta) of P_gm, xi+(theta) and xi-(theta) of P_mm - the real-space 3x2pt data vector.

Under the flat-sky Limber approximation with k = l / chi the chi^2 of the Limber measure cancels and

    zeta_n(theta) = int l dl/(2 pi) C_l J_n(l theta) = sum_z zw[z] W_n^(z)(R = chis[z] theta),      n = 0, 2, 4,

with W_n^(z)(R) = 1/(2 pi) int k P~(k, z) J_n(k R) dk the exact panel-by-panel transform of the row at z
(``projected_from_power``'s P~, linear in k^2 between the grid points and zero outside the grid) and zw the z measure
times the two windows (``Cosmology.angular_weights``).  n = 0 gives w(theta) and xi+, n = 2 gamma_t, n = 4 xi-.
``angular_from_power`` stands behind ``HaloModel.get_angular``, ``get_w_theta``, ``get_gamma_t``, ``get_xi_pm`` and
``get_angular_all``.  The kernels are in hmvec_amd/csrc/kernels/angular.hpp.
"""
import numpy as np

from . import realspace

__all__ = ["angular_from_power"]

ORDERS = (0, 2, 4)


def check_order(order):
    """The orders of an angular request as a tuple: 0, 2, 4 or a strictly increasing tuple of them."""
    orders = tuple(order) if isinstance(order, (tuple, list)) else (order,)
    ok = len(orders) >= 1 and all(not isinstance(o, bool) and isinstance(o, (int, np.integer)) and o in ORDERS
                                  for o in orders)
    if not ok or any(b <= a for a, b in zip(orders, orders[1:])):
        raise ValueError(f"order must be 0, 2, 4 or a strictly increasing tuple of them, got {order!r}")
    return tuple(int(o) for o in orders)


def check_chis(chis, nz):
    """The comoving distances of the nz rows as a float64 vector of finite, positive values."""
    chis = np.asarray(chis, dtype=np.float64)
    if chis.shape != (nz,):
        raise ValueError(f"chis must have shape ({nz},), got {chis.shape}")
    if not np.all(np.isfinite(chis)) or np.any(chis <= 0):
        raise ValueError("chis must be finite and positive")
    return chis


def check_zweights(zweights, nz):
    """The z weights of a request as a finite float64 (nw, nz) array, and whether they were given with the nw axis."""
    zw = np.asarray(zweights, dtype=np.float64)
    if zw.ndim not in (1, 2) or zw.shape[-1] != nz or zw.size == 0:
        raise ValueError(f"zweights must have shape ({nz},) or (nw, {nz}) with nw >= 1, got {zw.shape}")
    if not np.all(np.isfinite(zw)):
        raise ValueError("zweights must be finite")
    return np.ascontiguousarray(zw.reshape(-1, nz)), zw.ndim == 2


def angular_rows(ctx, d_ks, d_P, n, nz, nk, thetas, chis, zw, orders):
    """zeta_n, n in `orders`, of n blocks of nz device-resident rows of nk values at the checked angles (non-empty),
    distances and (nw, nz) weights: ONE transform launch of n nz rows for all orders and ONE contraction over z, a
    tuple of (n, nw, nt) host arrays in the order of `orders`."""
    nt, nw, no, rows = thetas.size, zw.shape[0], len(orders), n * nz
    W = ctx.empty((no * rows, nt))                      # the orders' (rows, nt) blocks one after the other
    w = {o: W.view(i * rows * nt, (rows, nt)) for i, o in enumerate(orders)}
    d_th, d_chi, d_zw = ctx.upload(thetas), ctx.upload(chis), ctx.upload(zw)
    ctx.call("hmg_angular_transform", n, nz, nk, nt, d_ks.ptr, d_P.ptr, d_chi.ptr, d_th.ptr,
             *(w[o].ptr if o in w else None for o in ORDERS))
    out = ctx.empty((no * n, nw, nt))
    ctx.call("hmg_angular_zsum", no * n, nz, nt, nw, d_zw.ptr, W.ptr, out.ptr)
    res = out.numpy().reshape(no, n, nw, nt)
    return tuple(res[i] for i in range(no))


def angular_from_power(ks, P, thetas, chis, zweights, order=0, *, ctx=None):
    """zeta_order[..., j] = sum_z zweights[..., z] W_order^(z)(chis[z] thetas[j]) of the spectra P[..., z, :] tabulated
    on ks, W_n(R) = 1/(2 pi) int k P~(k) Jn(k R) dk as for projected_from_power.

    ks: (nk,) with nk >= 2, finite, positive, strictly increasing.  P: (nz, nk) or (n, nz, nk), finite, as a host
    array or a DeviceArray.  thetas: angles in radians, finite and positive.  chis: (nz,) comoving distances of the
    rows, finite and positive, in the inverse units of ks.  zweights: (nz,) or (nw, nz), finite, any sign - the z
    measure times the two windows (Cosmology.angular_weights); several rows of weights (tomographic bin pairs) share
    the transform.  order: 0 (w(theta), xi+), 2 (gamma_t), 4 (xi-) or a strictly increasing tuple of them (all from
    one launch; each is bit for bit the single-order result).  Returns a float64 array of P's leading shape without
    z, then nw if zweights is two-dimensional, then len(thetas); a tuple of them, in order, for a tuple of orders.
    Anything else raises ValueError before a launch."""
    orders = check_order(order)
    ks, P, thetas, lead, rows = realspace._request(ks, P, thetas, "thetas")
    if len(lead) < 1:
        raise ValueError(f"P must have shape (nz, {ks.size}) or (n, nz, {ks.size}), got {tuple(lead) + (ks.size,)}")
    nz = int(lead[-1])
    if nz == 0:
        raise ValueError("P must hold at least one redshift")
    chis = check_chis(chis, nz)
    zw, stacked = check_zweights(zweights, nz)
    n = rows // nz
    shape = tuple(lead[:-1]) + ((zw.shape[0],) if stacked else ()) + (thetas.size,)
    if thetas.size == 0 or n == 0:
        outs = tuple(np.empty(shape) for _ in orders)
    else:
        ctx, d_ks, d_P = realspace._resident(ks, P, ctx)
        outs = tuple(o.reshape(shape) for o in angular_rows(ctx, d_ks, d_P, n, nz, ks.size, thetas, chis, zw, orders))
    return outs if isinstance(order, (tuple, list)) else outs[0]
