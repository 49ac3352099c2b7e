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
``get_excess_surface_density`` and their ``_all`` forms.  The kernels are in hmvec_amd/csrc/kernels/realspace.hpp
(xi) and hmvec_amd/csrc/kernels/hankel.hpp (the projected statistics).
"""
import numpy as np

from . import _native as nat
from . import spectra
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


class RealspaceMixin:
    """HaloModel's xi(r), w_p(r_p), Sigma(R) and Delta Sigma(R) (DESIGN.md sections 13, 14): the rows stay on the device
    from the mass integrals to the transform; only the (nz, nr) results cross to the host."""
    _XI_TERMS = ("total", "1h", "2h")

    def _xi_request(self, rs, term, what="rs"):
        """The checked radii (or angles: `what`) of a transform request (everything that can be refused is, before any
        launch)."""
        spectra.check_term(term, self._XI_TERMS)
        check_ks(self.ks)
        return check_rs(rs, what)

    def _xi_rows(self, d1, d2, term):
        """The device rows a term transforms; "total" is the device sum get_power brings to the host."""
        return d1 if term == "1h" else d2 if term == "2h" else self._sum_device(d1, d2)

    def _transform_rows(self, rows, nrows, rs, orders, zsum=None):
        """The transforms of nrows device rows at the radii rs as a tuple of (nrows, nr) host arrays: (xi,) for
        orders=None, else (W_n for n in orders), one launch either way.  With zsum = (chis, zw) rs are angles, the row
        at z is transformed at chis[z] rs and the rows of a block are summed with the (nw, nz) weights zw (section
        22): a tuple of (nrows / nz, nw, nr) arrays from one transform launch and one contraction."""
        if orders is None:
            return (transform_rows(self._ctx(), self._d_ks(), rows, nrows, self._nk, rs),)
        if zsum is not None:
            from .angular import angular_rows          # (angular.py imports this module)
            return angular_rows(self._ctx(), self._d_ks(), rows, nrows // self._nz, self._nz, self._nk, rs, *zsum, orders)
        return hankel_rows(self._ctx(), self._d_ks(), rows, nrows, self._nk, rs, orders)

    def _realspace_pair(self, rs, name, name2, term, orders, zsum=None):
        """What get_xi, the projected and the angular statistics of one pair share: the request's checks, the tSZ
        notice, the pair's cached device spectra and one transform launch.  A tuple of (nz, nr) arrays, with zsum of
        (1, nw, nr) arrays (see _transform_rows)."""
        rs = self._xi_request(rs, term, "rs" if zsum is None else "thetas")
        ra, rb = self._resolve(name, name if name2 is None else name2)
        if term != "1h":          # (get_power and get_power_2halo print it, get_power_1halo does not)
            self._tsz_notice(ra, rb)
        if rs.size == 0:
            shape = (self._nz, 0) if zsum is None else (1, zsum[1].shape[0], 0)
            return tuple(np.empty(shape) for _ in (orders or (None,)))
        ent = self._power_cached(ra, rb)
        return self._transform_rows(self._xi_rows(ent.p1h, ent.p2h, term), self._nz, rs, orders, zsum)

    def _realspace_all(self, pairs, rs, term, orders, zsum=None):
        """The same for several pairs: their spectra from one pass over the profile tensors (get_power_all's) into one
        block and all of them through ONE transform launch of len(pairs) * nz rows.  (pairs, tuple of (n, nz, nr)
        arrays, with zsum of (n, nw, nr) arrays); every [i] is bit for bit what _realspace_pair gives for pairs[i]."""
        rs = self._xi_request(rs, term, "rs" if zsum is None else "thetas")
        pairs = [tuple(p) for p in pairs]
        rpairs = self._resolve_pairs(pairs)
        if term != "1h":
            self._tsz_notice(*dict.fromkeys(r for rp in rpairs for r in rp))
        n, nz, nk = len(pairs), self._nz, self._nk
        if rs.size == 0 or n == 0:
            shape = (n, nz, rs.size) if zsum is None else (n, zsum[1].shape[0], rs.size)
            return pairs, tuple(np.empty(shape) for _ in (orders or (None,)))
        ctx = self._ctx()
        blk = ctx.empty((2 * n, nz, nk))
        o1 = [blk.view(i * nz * nk, (nz, nk)) for i in range(n)]
        o2 = [blk.view((n + i) * nz * nk, (nz, nk)) for i in range(n)]
        if spectra.batchable(spectra.pair_plan(rpairs)[0], rpairs):
            self._power_batch(rpairs, o1, o2)
        else:
            # one pair the batch cannot express sends all of them to the one-pair kernel there (another summation
            # order): take each pair's spectra as the one-pair call does, so that the entries keep its bits
            for (ra, rb), d1, d2 in zip(rpairs, o1, o2):
                ent = self._power_cached(ra, rb)
                ctx.call("hmg_memcpy_d2d", d1.ptr, ent.p1h.ptr, d1.nbytes)
                ctx.call("hmg_memcpy_d2d", d2.ptr, ent.p2h.ptr, d2.nbytes)
        rows = self._xi_rows(blk.view(0, (n * nz, nk)), blk.view(n * nz * nk, (n * nz, nk)), term)
        outs = self._transform_rows(rows, n * nz, rs, orders, zsum)
        return pairs, tuple(o.reshape(n, -1, rs.size) for o in outs)

    def get_xi(self, rs, name="nfw", name2=None, term="total"):
        """Correlation function xi(z, r), shape (nz, nr), of the spectrum of (name, name2) - of P_1h + P_2h
        (term="total"), P_1h ("1h") or P_2h ("2h") - by the exact transform of realspace.xi_from_power: bit for bit
        xi_from_power(ks, get_power(name, name2), rs) and its get_power_1halo / get_power_2halo counterparts."""
        return self._realspace_pair(rs, name, name2, term, None)[0]

    def get_xi_all(self, pairs, rs, term="total"):
        """{(name, name2): xi(z, r)} for several pairs: their spectra from one pass over the profile tensors
        (get_power_all's) and all of them through ONE transform launch of len(pairs) * nz rows.  Each entry is bit for
        bit get_xi of that pair."""
        pairs, (xi,) = self._realspace_all(pairs, rs, term, None)
        return {p: xi[i] for i, p in enumerate(pairs)}

    def get_wp(self, rps, name, name2=None, term="total"):
        """Projected correlation function w_p(z, r_p), shape (nz, nr), of the spectrum of (name, name2) - term as for
        get_xi - integrated along the whole line of sight (pi_max -> infinity): W_0 of
        realspace.projected_from_power, bit for bit projected_from_power(ks, get_power(name, name2), rps).  r_p is
        comoving, in the inverse units of ks; w_p has the units of P times those of ks squared (a length for a
        three-dimensional spectrum)."""
        return self._realspace_pair(rps, name, name2, term, (0,))[0]

    def get_surface_density(self, Rs, name, name2=None, term="total"):
        """Surface density Sigma(z, R) = rho_m0 W_0(R), shape (nz, nr), of the spectrum of (name, name2), e.g. P_gm -
        term as for get_xi; W_0 of realspace.projected_from_power.  Comoving units: rho_m0 = rho_matter_z(0) is the
        comoving matter density, R a comoving transverse distance in the inverse units of ks, Sigma a mass per comoving
        area with the mean density's contribution left out (the line-of-sight integral of rho_m0 xi).  The physical
        convention of sigma_2h_profiles (physical radius R_phys = R / (1 + z), mass per
        physical area, at the angle theta = R_phys / d_A(z) = R / chi(z)) is
        Sigma_phys(R_phys) = (1 + z)^2 Sigma(R_phys (1 + z))."""
        w0 = self._realspace_pair(Rs, name, name2, term, (0,))[0]          # (the request is checked first)
        return self._rho_m0() * w0

    def get_excess_surface_density(self, Rs, name, name2=None, term="total"):
        """Excess surface density Delta Sigma(z, R) = mean Sigma(< R) - Sigma(R) = rho_m0 W_2(R), shape (nz, nr), of
        the spectrum of (name, name2); units and the conversion to the physical convention of
        delta_sigma_2h_profiles as for get_surface_density: Delta Sigma_phys(R_phys) = (1 + z)^2 Delta Sigma(R_phys (1 + z))."""
        w2 = self._realspace_pair(Rs, name, name2, term, (2,))[0]
        return self._rho_m0() * w2

    def get_wp_all(self, pairs, rps, term="total"):
        """{(name, name2): w_p(z, r_p)} for several pairs, spectra and launches as for get_xi_all.  Each entry is bit
        for bit get_wp of that pair."""
        pairs, (wp,) = self._realspace_all(pairs, rps, term, (0,))
        return {p: wp[i] for i, p in enumerate(pairs)}

    def get_surface_density_all(self, pairs, Rs, term="total"):
        """{(name, name2): (Sigma(z, R), Delta Sigma(z, R))} for several pairs, spectra as for get_xi_all and both
        statistics from ONE transform launch.  Each entry is bit for bit get_surface_density and
        get_excess_surface_density of that pair."""
        pairs, (w0, w2) = self._realspace_all(pairs, Rs, term, (0, 2))
        rho = self._rho_m0()
        return {p: (rho * w0[i], rho * w2[i]) for i, p in enumerate(pairs)}
