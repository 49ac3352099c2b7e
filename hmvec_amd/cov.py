"""Covariances of halo-model spectra (DESIGN.md sections 15 and 17).

Three parts.  The Gaussian covariance between bandpowers mirrors the reference's ``hmvec/cov.py`` under the same names
(``bin_annuli``, ``shot_noise``, ``lensing_shape_noise``, ``GaussianCov``): host arithmetic on a few hundred numbers.
The connected part is what a halo model supplies: ``cl_cov_1halo`` is the Limber projection of the 1-halo trispectrum
``HaloModel.trispectrum_device`` contracts on the GPU; ``limber_samples`` builds its sample tables on the host.  The
super-sample covariance ``cl_cov_ssc`` is the Limber projection of the products of two responses to a background mode
(``HaloModel.response_device`` / ``ssc_device``) weighted with the variance of that mode in the survey window,
``sigma_b_disc``.  The three parts are not summed anywhere: the Limber measures of ``cl_cov_1halo`` and ``cl_cov_ssc``
differ.
"""
import warnings

import numpy as np
from scipy.interpolate import interp1d

from .quadrature import simpson_weights, trapz_weights

__all__ = ["bin_annuli", "default_binning", "shot_noise", "lensing_shape_noise", "GaussianCov", "limber_samples",
           "cl_cov_1halo", "sigma_b_disc", "cl_cov_ssc"]


# ---------------------------------------------------------------------------------------- Gaussian part (hmvec/cov.py)
def bin_annuli(ells, cls, bin_edges):
    """Bandpowers of cls weighted by ell: mean(ell * C_ell) / mean(ell) over the multipoles of each bin, NaNs of
    ell * C_ell left out of the numerator's mean (hmvec/cov.py:11-14).  Bins are [edge_i, edge_i+1), the last one closed
    on the right; multipoles outside the edges are dropped, an empty bin gives NaN."""
    ells, cls = np.asarray(ells, dtype=np.float64), np.asarray(cls, dtype=np.float64)
    edges = np.asarray(bin_edges, dtype=np.float64)
    which = np.searchsorted(edges, ells, side="right") - 1
    which[ells == edges[-1]] = edges.size - 2
    out = np.full(edges.size - 1, np.nan)
    prod = ells * cls
    with np.errstate(invalid="ignore", divide="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)          # (a bin of NaNs only: NaN, quietly)
        for b in range(edges.size - 1):
            sel = which == b
            if sel.any():
                out[b] = np.nanmean(prod[sel]) / np.nanmean(ells[sel])
    return out


default_binning = bin_annuli


def shot_noise(ngal):
    """1 / (ngal * 1.18e7): ngal per square arcminute to a white noise level per steradian (hmvec/cov.py:19-20)."""
    return 1.0 / (ngal * 1.18e7)


def lensing_shape_noise(ngal, shape_noise=0.3):
    """shape_noise^2 / 2 / shot_noise(ngal), as the reference has it (hmvec/cov.py:22-23: it divides by the shot
    noise where the usual expression multiplies; kept)."""
    return (shape_noise ** 2.0) / 2.0 / shot_noise(ngal)


def _lookup(table, x, y):
    """The reference's get_avail_cls: the entry stored as "x_y", else 0.  A pair stored in the OTHER name order is not
    found - the reference's fallback names an undefined variable and its bare except turns that into 0.  Kept."""
    try:
        return table[x + "_" + y]
    except Exception:
        return 0


class GaussianCov(object):
    """Gaussian covariance between bandpowers (hmvec/cov.py:33-63).  Spectra are stored binned under "name1_name2";
    get_cov(x, y, w, z, fsky) = (C_xw C_yz + C_xz C_yw) / (2 l + 1) / dl / fsky with the total (signal + noise) spectra.

    Quirk kept from the reference: a lookup in the other name order than the one a spectrum was added in returns 0 (see
    _lookup), so get_cov("k", "g", "g", "k", ...) misses the cross terms that were added as ("k", "g")."""

    def __init__(self, bin_edges, binning_func=default_binning):
        """bin_edges: ascending multipole edges (an array).  binning_func is accepted and, as in the reference, not
        used: spectra are always binned with bin_annuli."""
        edges = np.asarray(bin_edges)
        self.bin_edges = bin_edges
        self.cls, self.nls = {}, {}                              # binned signal and noise spectra by "name1_name2"
        self.ells = np.arange(edges[0], edges[-1] + 1, 1)        # every multipole from the first edge to the last
        self.ls = 0.5 * (edges[1:] + edges[:-1])                 # bin centres
        self.dls = np.diff(edges)                                # bin widths

    def _binned(self, ells, cls):
        """A spectrum tabulated at ells, interpolated linearly to every multipole of the range (a multipole outside
        the table raises ValueError, as interp1d does) and binned."""
        return bin_annuli(self.ells, interp1d(ells, cls)(self.ells), self.bin_edges)

    def add_cls(self, name1, name2, ells, cls, ellsn=None, ncls=None):
        """Store the spectrum of (name1, name2) and, if both ellsn and ncls are given, its noise.  Names must not
        contain "_", and a pair already stored in the other order is refused (AssertionError, as in the reference)."""
        key = f"{name1}_{name2}"
        assert "_" not in name1 and "_" not in name2
        assert f"{name2}_{name1}" not in self.cls
        self.cls[key] = self._binned(ells, cls)
        if ellsn is not None and ncls is not None:
            self.nls[key] = self._binned(ellsn, ncls)

    def get_scls(self, x, y):
        return _lookup(self.cls, x, y)

    def get_ncls(self, x, y):
        return _lookup(self.nls, x, y)

    def get_tcls(self, x, y):
        return self.get_scls(x, y) + self.get_ncls(x, y)

    def get_cov(self, x, y, w, z, fsky):
        """Cov(C^xy, C^wz) per bin: (C_xw C_yz + C_xz C_yw) / ((2 l + 1) dl fsky), total spectra, l the bin centre."""
        t = self.get_tcls
        modes = (2 * self.ls + 1.0) * self.dls * fsky
        return (t(x, w) * t(y, z) + t(x, z) * t(y, w)) / modes


# ---------------------------------------------------------------------------------------- connected part, 1-halo term
def limber_samples(ells, chis, ks, zs=None):
    """Where the Limber wavenumbers k = (ell + 1/2) / chi(z) lie in the grid ks: (idx, frac), each (nz, n_ell), with
    k = (1 - frac) ks[idx] + frac ks[idx + 1], 0 <= frac < 1.  A k on a grid point has frac = 0 at that point - the last
    one included (idx = nk - 1, frac = 0: node idx + 1 is never read there).  A k outside [ks[0], ks[-1]] raises
    ValueError naming the multipole and the redshift (zs, if given, else its index), as the reference's Limber code does
    for C_ell (interp2d(bounds_error=True)); chi = 0 therefore raises."""
    ells = np.asarray(ells, dtype=np.float64).reshape(-1)
    chis = np.asarray(chis, dtype=np.float64).reshape(-1)
    ks = np.asarray(ks, dtype=np.float64).reshape(-1)
    if ks.size < 2 or np.any(np.diff(ks) <= 0):
        raise ValueError("ks must be strictly increasing, at least two points")
    with np.errstate(divide="ignore", invalid="ignore"):
        k = (ells[None, :] + 0.5) / chis[:, None]
    bad = ~((k >= ks[0]) & (k <= ks[-1]))
    if bad.any():
        iz, il = np.argwhere(bad)[0]
        where = f"z = {float(np.asarray(zs).reshape(-1)[iz])!r}" if zs is not None else f"redshift index {iz}"
        raise ValueError(f"ell = {float(ells[il])!r} at {where}: k = (ell + 1/2) / chi = {float(k[iz, il])!r} is outside "
                         f"the grid [{float(ks[0])!r}, {float(ks[-1])!r}]")
    idx = np.searchsorted(ks, k, side="right") - 1              # ks[idx] <= k, and k == ks[-1] gives nk - 1
    last = idx == ks.size - 1
    lo = ks[idx]
    hi = ks[np.minimum(idx + 1, ks.size - 1)]
    frac = np.where(last, 0.0, (k - lo) / np.where(last, 1.0, hi - lo))
    frac = np.clip(frac, 0.0, 1.0)
    return idx.astype(np.int32), frac


def cl_cov_1halo(model, ells, name, name2=None, name3=None, name4=None, W1=1, W2=1, W3=1, W4=1, fsky=1.0, damping=True):
    """The 1-halo part of the connected covariance of two Limber spectra C_ell^{ab} and C_ell'^{cd}, (n_ell, n_ell):

        Cov(l, l') = 1 / (4 pi fsky) trapz_z[ H(z) W1 W2 W3 W4 / chi^6  T_1h^{ab,cd}(z; (l + 1/2)/chi, (l' + 1/2)/chi) ]

    on the model's own zs (at least two), H in 1/Mpc and chi in Mpc as in limber_integral / C_kk / C_yy; the windows are
    scalars or (nz,) arrays of those functions' conventions.  T at the Limber wavenumbers is the bilinear interpolant of
    T at the nodes of the model's ks (limber_samples); a wavenumber outside the grid raises ValueError, so z = 0 in zs
    does.  name3 / name4 default to the first pair; damping as in HaloModel.get_trispectrum_1halo.  The z sum is taken on
    the device, in z order."""
    ells = np.asarray(ells, dtype=np.float64).reshape(-1)
    zs = np.asarray(model.zs, dtype=np.float64).reshape(-1)
    if zs.size < 2:
        raise ValueError("cl_cov_1halo integrates over the model's redshifts: it needs at least two")
    if not fsky > 0:
        raise ValueError(f"fsky must be positive, got {fsky!r}")
    chis = np.asarray(model.comoving_radial_distance(zs), dtype=np.float64).reshape(-1)
    hzs = np.asarray(model.h_of_z(zs), dtype=np.float64).reshape(-1)
    idx, frac = limber_samples(ells, chis, model.ks, zs=zs)
    g = trapz_weights(zs) * hzs / chis ** 6 / (4.0 * np.pi * fsky)
    for W in (W1, W2, W3, W4):
        g = g * np.broadcast_to(np.asarray(W, dtype=np.float64), zs.shape)
    if ells.size == 0:
        return np.empty((0, 0))
    _, Tz = model.trispectrum_device(name, name2, name3, name4, damping=damping, idx=idx, frac=frac, zweights=g,
                                     per_z=False)
    return Tz.numpy()


# ---------------------------------------------------------------------------------------- super-sample covariance
def dlnp_table(ks, Pzk):
    """dlnP[z,k] = d ln P_lin / d ln k on the model's grid: np.gradient(log Pzk, log ks, axis=-1).  The table is
    uploaded as it is, so the device and a restatement interpolate the same numbers."""
    return np.gradient(np.log(np.asarray(Pzk, dtype=np.float64)), np.log(np.asarray(ks, dtype=np.float64)), axis=-1)


def sigma_b_disc(ks, Pzk, chis, fsky=None, theta_s=None):
    """The variance of the background density mode in a disc-shaped survey per unit radial length, (nz,), in Mpc:

        sigma_b(z) = 1 / (2 pi) sum_j w_j k_j P[z,j] (2 J1(x) / x)^2,    x = k_j chi(z) theta_s,

    w the Simpson weights of ks (quadrature.simpson_weights, the rule of the sigma^2 integral), P (nz, nq) the linear
    spectrum on ks, chi in Mpc.  The disc is the cap of area 4 pi fsky, theta_s = arccos(1 - 2 fsky), if fsky is given;
    exactly one of fsky (in (0, 1]) and theta_s (radians, >= 0) must be.  x == 0 gives a window of 1."""
    from scipy.special import j1
    if (fsky is None) == (theta_s is None):
        raise ValueError("give exactly one of fsky and theta_s")
    if fsky is not None:
        fsky = float(fsky)
        if not (0.0 < fsky <= 1.0):
            raise ValueError(f"fsky must lie in (0, 1], got {fsky!r}")
        theta_s = np.arccos(1.0 - 2.0 * fsky)
    theta_s = float(theta_s)
    if not (np.isfinite(theta_s) and theta_s >= 0.0):
        raise ValueError(f"theta_s must be finite and not negative, got {theta_s!r}")
    ks = np.asarray(ks, dtype=np.float64).reshape(-1)
    P = np.atleast_2d(np.asarray(Pzk, dtype=np.float64))
    chis = np.asarray(chis, dtype=np.float64).reshape(-1)
    if P.shape != (chis.size, ks.size):
        raise ValueError(f"Pzk must have shape (nz, nq) = {(chis.size, ks.size)}, got {P.shape}")
    x = ks[None, :] * chis[:, None] * theta_s
    zero = x == 0.0
    win = np.where(zero, 1.0, 2.0 * j1(x) / np.where(zero, 1.0, x))
    return np.sum((simpson_weights(ks) * ks)[None, :] * P * win * win, axis=1) / (2.0 * np.pi)


def ssc_limber_tables(model, ells, npairs, windows=None, fsky=None, sigma_b=None):
    """The host tables of cl_cov_ssc: (idx, frac, g, zscale) - the Limber samples of the multipoles, the z weights
    g = trapz weight H^3 sigma_b / chi^4 and zscale (npairs, nz) = W1 W2 of each pair.  Everything that can be refused
    is, here."""
    ells = np.asarray(ells, dtype=np.float64).reshape(-1)
    zs = np.asarray(model.zs, dtype=np.float64).reshape(-1)
    if zs.size < 2:
        raise ValueError("cl_cov_ssc integrates over the model's redshifts: it needs at least two")
    chis = np.asarray(model.comoving_radial_distance(zs), dtype=np.float64).reshape(-1)
    hzs = np.asarray(model.h_of_z(zs), dtype=np.float64).reshape(-1)
    if sigma_b is None:
        if fsky is None:
            raise ValueError("give sigma_b (nz,) or fsky")
        from .cosmology import sigma2_kgrid
        kq = sigma2_kgrid(model.p["sigma2_kmin"], model.p["sigma2_kmax"], model.p["sigma2_numks"])
        sigma_b = sigma_b_disc(kq, model.sPzk, chis, fsky=fsky)
    else:
        sigma_b = np.asarray(sigma_b, dtype=np.float64)
        if sigma_b.shape != zs.shape:
            raise ValueError(f"sigma_b must have one entry per redshift ({zs.size}), got shape {sigma_b.shape}")
    if windows is None:
        windows = [(1, 1)] * npairs
    if len(windows) != npairs:
        raise ValueError(f"windows must have one (W1, W2) per pair ({npairs}), got {len(windows)}")
    zscale = np.empty((npairs, zs.size))
    for p, (W1, W2) in enumerate(windows):
        zscale[p] = (np.broadcast_to(np.asarray(W1, dtype=np.float64), zs.shape)
                     * np.broadcast_to(np.asarray(W2, dtype=np.float64), zs.shape))
    idx, frac = limber_samples(ells, chis, model.ks, zs=zs)
    g = trapz_weights(zs) * hzs ** 3 * sigma_b / chis ** 4
    return idx, frac, g, zscale


def cl_cov_ssc(model, ells, pairs, windows=None, fsky=None, sigma_b=None, damping=True):
    """The super-sample covariance of the Limber spectra C_ell^{p} of the pairs p = (a, b), (np, n_ell, np, n_ell):

        Cov[p,l,q,l'] = trapz_z[ H^3 sigma_b / chi^4  (W_p1 W_p2 R_p(z, (l + 1/2)/chi)) (W_q1 W_q2 R_q(z, (l' + 1/2)/chi)) ]

    on the model's own zs (at least two), H in 1/Mpc and chi in Mpc as in limber_integral; R = dP / d delta_b is
    HaloModel.response_device's at the Limber samples (limber_samples: a wavenumber outside the model's grid raises
    ValueError).  windows[p] = (W1, W2), scalars or (nz,) arrays of limber_integral's conventions (default 1).
    sigma_b (nz,) is the variance of the background mode per unit radial length, in Mpc; None: sigma_b_disc on the
    model's sigma^2 grid and spectrum at fsky.  The measure is H^3 and not H: with C_ell = int dz H W1 W2 P / chi^2 the
    kernel per d chi is H W, and <delta_b(z) delta_b(z')> = H delta_D(z - z') sigma_b.  The z sum is taken on the device,
    in z order.  The result is not to be added to cl_cov_1halo's, whose measure differs."""
    pairs = list(pairs)
    idx, frac, g, zscale = ssc_limber_tables(model, ells, len(pairs), windows, fsky, sigma_b)
    if idx.shape[1] == 0:
        return np.empty((len(pairs), 0, len(pairs), 0))
    return model.ssc_device(pairs, g, zscale=zscale, idx=idx, frac=frac, damping=damping).numpy()
