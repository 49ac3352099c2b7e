"""Angular correlation functions of halo-model spectra on the GPU: w(theta) of P_gg,
gamma_t(theta) of P_gm, xi+(theta) and xi-(theta) of P_mm - the real-space 3x2pt data vector.

Under the flat-sky Limber approximation with k = l / chi the chi^2 of the Limber measure cancels and

    zeta_n(theta) = int l dl/(2 pi) C_l J_n(l theta) = sum_z zw[z] W_n^(z)(R = chis[z] theta),      n = 0, 2, 4,

with W_n^(z)(R) = 1/(2 pi) int k P~(k, z) J_n(k R) dk the exact panel-by-panel transform of the row at z
(``projected_from_power``'s P~, linear in k^2 between the grid points and zero outside the grid) and zw the z measure
times the two windows (``Cosmology.angular_weights``).  n = 0 gives w(theta) and xi+, n = 2 gamma_t, n = 4 xi-.
``angular_from_power`` stands behind ``HaloModel.get_angular``, ``get_w_theta``, ``get_gamma_t``, ``get_xi_pm`` and
``get_angular_all``.  The kernels are in hmvec_amd/csrc/kernels/hankel.hpp.
"""
import numpy as np

from . import realspace, spectra

__all__ = ["angular_from_power"]

ORDERS = (0, 2, 4)
_trapz = getattr(np, "trapezoid", None) or np.trapz


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


class AngularMixin:
    """HaloModel's w(theta), gamma_t(theta), xi+-(theta): the rows are transformed at chi(z) theta
    and summed over z on the device (RealspaceMixin's _realspace_pair, _realspace_all); only (nw, ntheta) results cross."""

    def _angular_request(self, zweights, order, term):
        """(zsum, orders, stacked) of an angular request: the distances of self.zs, the checked (nw, nz) weights
        (None: the z measure alone, both windows 1) and orders, and whether the weights came with the nw axis."""
        spectra.check_term(term, self._XI_TERMS)
        orders = check_order(order)
        nz = np.size(self.zs)
        if zweights is None:
            zweights = self.angular_weights(self.zs, 1.0, 1.0)
        zw, stacked = check_zweights(zweights, nz)
        chis = check_chis(np.reshape(self.comoving_radial_distance(self.zs), -1), nz)
        return (chis, zw), orders, stacked

    def get_angular(self, thetas, name, name2=None, zweights=None, order=0, term="total"):
        """Angular correlation function zeta_order(theta) = sum_z zweights[z] W_order^(z)(chi(z) theta) of the spectrum
        of (name, name2) - term as for get_xi - on the model's redshifts self.zs, chi = comoving_radial_distance(zs)
        (every z must be positive): bit for bit angular.angular_from_power(ks, get_power(name, name2), thetas, chi,
        zweights, order).  thetas in radians.  zweights: (nz,) or (nw, nz), the z measure times the two windows
        (angular_weights(zs, W1, W2)); None is the measure alone.  order: 0, 2, 4 or a strictly increasing tuple of
        them.  Returns (ntheta,), or (nw, ntheta) for two-dimensional weights; a tuple of them for a tuple of
        orders."""
        zsum, orders, stacked = self._angular_request(zweights, order, term)
        outs = self._realspace_pair(thetas, name, name2, term, orders, zsum)
        outs = tuple(o[0] if stacked else o[0, 0] for o in outs)
        return outs if isinstance(order, (tuple, list)) else outs[0]

    def _dndz_window(self, dndz, what):
        """dndz / int dndz dz on self.zs (C_gg's convention); None is a uniform distribution over the range of zs."""
        zs = np.reshape(self.zs, -1)
        if zs.size < 2:
            raise ValueError(f"{what} needs at least two redshifts in the model")
        dndz = np.ones(zs.size) if dndz is None else np.asarray(dndz, dtype=np.float64)
        if dndz.shape != zs.shape or not np.all(np.isfinite(dndz)):
            raise ValueError(f"{what} must be a finite vector of {zs.size} values on the model's redshifts")
        norm = _trapz(dndz, zs)
        if not norm > 0:
            raise ValueError(f"{what} must have a positive integral over the model's redshifts")
        return dndz / norm

    def _source_window(self, zsource, sdndz, what):
        """lensing_window on self.zs of a source plane (zsource a scalar) or of sources sdndz on the grid zsource."""
        if zsource is None:
            raise ValueError(f"{what} is required: a source redshift, or the grid of a source distribution")
        zsource = np.asarray(zsource, dtype=np.float64).reshape(-1)
        if (zsource.size == 1) != (sdndz is None) or (sdndz is not None and np.shape(sdndz) != zsource.shape):
            raise ValueError(f"{what}: one source redshift without a distribution, or a grid with its distribution")
        return self.lensing_window(np.reshape(self.zs, -1), zsource, sdndz)

    def get_w_theta(self, thetas, name, name2=None, dndz=None, dndz2=None, term="total"):
        """Angular clustering w(theta), shape (ntheta,): order 0 with the windows dndz / int dndz dz of the two samples
        on self.zs (C_gg's convention; dndz None: uniform over the range of zs, dndz2 None: the first sample's) -
        bit for bit get_angular(thetas, name, name2, angular_weights(zs, W1, W2), 0, term)."""
        spectra.check_term(term, self._XI_TERMS)
        W1 = self._dndz_window(dndz, "dndz")
        W2 = W1 if dndz2 is None else self._dndz_window(dndz2, "dndz2")
        return self.get_angular(thetas, name, name2, self.angular_weights(self.zs, W1, W2), 0, term)

    def get_gamma_t(self, thetas, name, name2="nfw", dndz=None, zsource=None, sdndz=None, term="total"):
        """Tangential shear gamma_t(theta), shape (ntheta,), of the lenses `name` (window dndz / int dndz dz as for
        get_w_theta) about sources at zsource (a single redshift, or a grid with the distribution sdndz: the arguments
        of lensing_window): order 2 of the lens-matter spectrum - bit for bit
        get_angular(thetas, name, name2, angular_weights(zs, W_lens, lensing_window(zs, zsource, sdndz)), 2, term)."""
        spectra.check_term(term, self._XI_TERMS)
        W1 = self._dndz_window(dndz, "dndz")
        W2 = self._source_window(zsource, sdndz, "zsource")
        return self.get_angular(thetas, name, name2, self.angular_weights(self.zs, W1, W2), 2, term)

    def get_xi_pm(self, thetas, name="nfw", name2=None, zsource=None, sdndz=None, zsource2=None, sdndz2=None,
                  term="total"):
        """Shear correlation functions (xi+(theta), xi-(theta)), each (ntheta,), of sources at zsource (and zsource2,
        default the same; arguments as for get_gamma_t): orders 0 and 4 of the matter spectrum from ONE launch - bit
        for bit get_angular(thetas, name, name2, angular_weights(zs, W_kappa1, W_kappa2), (0, 4), term)."""
        spectra.check_term(term, self._XI_TERMS)
        W1 = self._source_window(zsource, sdndz, "zsource")
        W2 = W1 if zsource2 is None else self._source_window(zsource2, sdndz2, "zsource2")
        return self.get_angular(thetas, name, name2, self.angular_weights(self.zs, W1, W2), (0, 4), term)

    def get_angular_all(self, pairs, thetas, zweights, order=0, term="total"):
        """{(name, name2): zeta_order(theta)} for several pairs: their spectra from one pass over the profile tensors
        (get_power_all's), ONE transform launch of len(pairs) * nz rows and one contraction over z.  zweights: (nz,)
        or (nw, nz) shared by all pairs, or a dict {pair: weights}.  Each entry is bit for bit get_angular of that
        pair with its weights."""
        pairs = [tuple(p) for p in pairs]
        if isinstance(zweights, dict):
            missing = [p for p in pairs if p not in zweights]
            if missing:
                raise ValueError(f"zweights has no entry for {missing}")
            per = [check_zweights(zweights[p], np.size(self.zs)) for p in pairs]
        else:
            per = [check_zweights(zweights, np.size(self.zs))] * len(pairs)
        # every pair's rows of weights go stacked into the one contraction and the pair keeps its own: an output's
        # chain reads its row of weights alone, so its bits are those of the pair's own call
        shared = not isinstance(zweights, dict)
        stack = None if not per else per[0][0] if shared else np.concatenate([zw for zw, _ in per])
        zsum, orders, _ = self._angular_request(stack, order, term)
        pairs, outs = self._realspace_all(pairs, thetas, term, orders, zsum)
        res, lo = {}, 0
        for i, (p, (zw, stacked)) in enumerate(zip(pairs, per)):
            ent = tuple(o[i, lo:lo + zw.shape[0]] if stacked else o[i, lo] for o in outs)
            res[p] = ent if isinstance(order, (tuple, list)) else ent[0]
            lo += 0 if shared else zw.shape[0]
        return res
