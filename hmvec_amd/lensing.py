"""Cluster-lensing profiles on the GPU: batched functions of plain arrays behind HaloModel.sigma_1h_profiles,
kappa_1h_profiles and kappa_2h_profiles (hmvec/hmvec.py:574-625) and behind their excess
surface density and tangential shear counterparts.

``sigma_nfw`` is the batched counterpart of clusterlensing's ``SurfaceMassDensity(rs, delta_c, rho_crit, rbins,
offsets).sigma_nfw()`` - the product the reference's sigma_1h_profiles forms - as a plain float64 array in the units
of its inputs (Msun/Mpc^2 from Mpc and Msun/Mpc^3); ``delta_sigma_nfw`` is the counterpart of its ``deltasigma_nfw()``.
The kernels are in hmvec_amd/csrc/kernels/lensing.hpp.
"""
import numpy as np

from . import _native as nat
from ._native import as_device as _dev, context_or_default as _context
from .utils import _R_from_M

__all__ = ["sigma_nfw", "delta_sigma_nfw", "kappa_2h_integral", "gamma_t_2h_integral"]


def _positive(name, a):
    a = np.asarray(a, dtype=np.float64)
    if not np.all(np.isfinite(a)) or np.any(a <= 0):
        raise ValueError(f"{name} must be finite and positive")
    return a


def sigma_nfw(rs, delta_c, rho_crit, rbins, offsets=None, *, ctx=None):
    """Projected NFW surface density Sigma[i, j] of halo i at projected radius rbins[i, j] (or rbins[j]).

    rs, delta_c, rho_crit: length-N per-halo arrays (scale radius, characteristic overdensity, critical density).
    rbins: (N, nR) or (nR,).  offsets: None, or a length-N array of Rayleigh miscentring widths; halos with offset 0
    take the centred profile (bit for bit the values of offsets=None).  Returns an (N, nR) float64 array."""
    return _nfw_profile("hmg_lensing_sigma_nfw", rs, delta_c, rho_crit, rbins, offsets, ctx)


def delta_sigma_nfw(rs, delta_c, rho_crit, rbins, offsets=None, *, ctx=None):
    """Excess surface density Delta Sigma[i, j] = Sigmabar(<R) - Sigma(R) of NFW halo i at R = rbins[i, j] (or
    rbins[j]); with offsets, Sigmabar_off(<R) - Sigma_off(R) of the Rayleigh-miscentred profile.  Arguments, checks
    and shapes as sigma_nfw (halos with offset 0 take the centred profile, bit for bit)."""
    return _nfw_profile("hmg_lensing_delta_sigma_nfw", rs, delta_c, rho_crit, rbins, offsets, ctx)


def _nfw_profile(entry, rs, delta_c, rho_crit, rbins, offsets, ctx):
    """sigma_nfw / delta_sigma_nfw: `entry` is the centred C entry point, entry + "_off" the miscentred one."""
    rs = _positive("rs", np.atleast_1d(rs)).ravel()
    n = rs.size
    delta_c = _positive("delta_c", np.atleast_1d(delta_c)).ravel()
    rho_crit = _positive("rho_crit", np.atleast_1d(rho_crit)).ravel()
    if delta_c.size != n or rho_crit.size != n:
        raise ValueError("rs, delta_c and rho_crit must have the same length")
    rbins = _positive("rbins", rbins)
    if rbins.ndim == 1:
        per_halo = 0
    elif rbins.ndim == 2 and rbins.shape[0] == n:
        per_halo = 1
    else:
        raise ValueError(f"rbins must be (nR,) or ({n}, nR), got {rbins.shape}")
    nr = rbins.shape[-1]
    if n == 0 or nr == 0:
        return np.empty((n, nr))
    off = None
    if offsets is not None:
        off = np.asarray(offsets, dtype=np.float64).ravel()
        if off.size == 1 and n > 1:
            off = np.full(n, off[0])
        if off.size != n or not np.all(np.isfinite(off)) or np.any(off < 0):
            raise ValueError("offsets must be a non-negative array with one entry per halo")
        if not np.any(off > 0):
            off = None
    ctx = _context(ctx)
    d_rs, d_dc, d_rho, d_r = (_dev(ctx, a) for a in (rs, delta_c, rho_crit, rbins))
    out = ctx.empty((n, nr))
    if off is None or not np.all(off > 0):
        ctx.call(entry, n, nr, per_halo, d_rs.ptr, d_dc.ptr, d_rho.ptr, d_r.ptr, out.ptr)
    if off is None:
        return out.numpy()
    centred = out.numpy() if not np.all(off > 0) else None
    # halos without an offset: the quadrature needs a positive width, so give them one and take the centred values
    d_off = _dev(ctx, np.where(off > 0, off, 1.0))
    ctx.call(entry + "_off", n, nr, per_halo, d_rs.ptr, d_dc.ptr, d_rho.ptr, d_r.ptr, d_off.ptr, out.ptr)
    res = out.numpy()
    if centred is not None:
        res = np.where((off > 0)[:, None], res, centred)
    return res


def kappa_2h_integral(ks, chi, pre, Pzk, thetas, lmin, lmax, ms, bh, Ms, *, ctx=None):
    """Two-halo convergence out[z, t, m] = b(z, Ms[m]) pre[z] trapz_l[P(z,k) J0(l thetas[t]) l / 2 pi] over the
    l = ks chi[z] with lmin < l < lmax (hmvec/hmvec.py:598-625, per lens redshift).

    ks (nk,) increasing, chi and pre (nz,), Pzk (nz, nk), thetas (nt,) in radians, ms (nm,) increasing, bh (nz, nm),
    Ms (nM,) inside [ms[0], ms[-1]].  Pzk and bh may be DeviceArrays (a model's resident arrays).  Returns an
    (nz, nt, nM) float64 array."""
    return _two_halo("hmg_lensing_kappa_2h", ks, chi, pre, Pzk, thetas, lmin, lmax, ms, bh, Ms, ctx)


def gamma_t_2h_integral(ks, chi, pre, Pzk, thetas, lmin, lmax, ms, bh, Ms, *, ctx=None):
    """Two-halo tangential shear out[z, t, m] = b(z, Ms[m]) pre[z] trapz_l[P(z,k) J2(l thetas[t]) l / 2 pi]: the
    kappa_2h_integral with J0 replaced by J2 (Oguri & Takada 2011), same arguments, checks and shape.  With pre
    without its 1/Sigma_crit it is the two-halo Delta Sigma."""
    return _two_halo("hmg_lensing_gamma_t_2h", ks, chi, pre, Pzk, thetas, lmin, lmax, ms, bh, Ms, ctx)


def _two_halo(entry, ks, chi, pre, Pzk, thetas, lmin, lmax, ms, bh, Ms, ctx):
    ks = np.asarray(ks, dtype=np.float64).ravel()
    chi = np.asarray(chi, dtype=np.float64).ravel()
    pre = np.asarray(pre, dtype=np.float64).ravel()
    thetas = _positive("thetas", np.atleast_1d(thetas)).ravel()
    Ms = _positive("Ms", np.atleast_1d(Ms)).ravel()
    nz, nk, nt, nM = chi.size, ks.size, thetas.size, Ms.size
    if pre.size != nz or nz == 0 or nk == 0:
        raise ValueError("chi and pre need one entry per lens redshift, ks at least one wavenumber")
    if nk > 1 and not np.all(np.diff(ks) > 0):
        raise ValueError("ks must be strictly increasing")
    ms = np.asarray(ms, dtype=np.float64).ravel()
    nm = ms.size
    if nm < 2 or not np.all(np.diff(ms) > 0):
        raise ValueError("ms must be strictly increasing with at least two masses")
    if np.any(Ms < ms[0]) or np.any(Ms > ms[-1]):
        raise ValueError("A value in x_new is outside the interpolation range of the mass grid")
    for name, a, shape in (("Pzk", Pzk, (nz, nk)), ("bh", bh, (nz, nm))):
        if tuple(np.shape(a) if not isinstance(a, nat.DeviceArray) else a.shape) != shape:
            raise ValueError(f"{name} must have shape {shape}")
    if nt == 0 or nM == 0:
        return np.empty((nz, nt, nM))
    ctx = _context(ctx)
    d = [_dev(ctx, a) for a in (ks, chi, pre, Pzk, thetas, ms, bh, Ms)]
    out = ctx.empty((nz, nt, nM))
    ctx.call(entry, nz, nk, nt, nm, nM, d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr, d[4].ptr,
             float(lmin), float(lmax), d[5].ptr, d[6].ptr, d[7].ptr, out.ptr)
    return out.numpy()


class ClusterLensingMixin:
    """HaloModel's cluster-lensing profiles (DESIGN.md sections 10, 12).  The per-halo scalars are formed on the host one
    lens redshift at a time (a few values per halo), so that a z slice of a model with several redshifts is the same
    computation as a model of that redshift alone.  With one redshift the results have the reference's shapes; with
    nz > 1 a leading z axis is added."""

    @staticmethod
    def _lensing_thetas(thetas):
        th = np.atleast_1d(np.asarray(thetas, dtype=np.float64)).ravel()
        if not np.all(np.isfinite(th)) or np.any(th <= 0):
            raise ValueError("thetas must be finite and positive")
        return th

    def _lensing_halos(self, Ms, concs, delta, rho, rho_at_z):
        """(Ms, concs, [(D_A, r_s, delta_c, rho_crit) per z]) of sigma_1h_profiles (hmvec/hmvec.py:574-589)."""
        Ms = np.atleast_1d(np.asarray(Ms, dtype=np.float64)).ravel()
        concs = np.atleast_1d(np.asarray(concs, dtype=np.float64)).ravel()
        if Ms.size != concs.size:
            raise ValueError("Ms and concs must have the same length")
        if not (np.all(np.isfinite(Ms)) and np.all(Ms > 0) and np.all(np.isfinite(concs)) and np.all(concs > 0)):
            raise ValueError("masses and concentrations must be finite and positive")
        if rho == "critical":
            rhofunc = self.rho_critical_z
        elif rho == "mean":
            rhofunc = self.rho_matter_z
        else:
            raise ValueError(f"rho must be 'mean' or 'critical', got {rho!r}")
        fcon = np.log(1.0 + concs) - (concs / (1.0 + concs))      # Fcon (hmvec/hmvec.py:737)
        rows = []
        for z in self.zs:
            zz = np.array([z])
            rhoz = zz if rho_at_z else zz * 0
            rs = _R_from_M(Ms, rhofunc(rhoz), delta=delta) / concs
            rhoc = self.rho_critical_z(zz)
            delta_c = Ms / 4 / np.pi / rs ** 3 / rhoc / fcon
            rows.append((float(self.angular_diameter_distance(zz)[0]), rs, delta_c, float(rhoc[0])))
        return Ms, concs, rows

    def sigma_1h_profiles(self, thetas, Ms, concs, sig_theta=None, delta=200, rho="mean", rho_at_z=True):
        """One-halo surface density Sigma [Msun/Mpc^2] of NFW halos (masses Ms, concentrations concs) at angles
        thetas [rad] (hmvec/hmvec.py:574-590): (nM, ntheta), or (nz, nM, ntheta) with several lens redshifts.
        sig_theta [rad] averages over Rayleigh-distributed miscentring of width D_A(z) sig_theta; 0 is the centred
        profile."""
        return self._lensing_1h(sigma_nfw, thetas, Ms, concs, sig_theta, delta, rho, rho_at_z)

    def delta_sigma_1h_profiles(self, thetas, Ms, concs, sig_theta=None, delta=200, rho="mean", rho_at_z=True):
        """One-halo excess surface density Delta Sigma = Sigmabar(<R) - Sigma(R) [Msun/Mpc^2],
        with the arguments, conventions and shapes of sigma_1h_profiles: (nM, ntheta), or (nz, nM, ntheta)."""
        return self._lensing_1h(delta_sigma_nfw, thetas, Ms, concs, sig_theta, delta, rho, rho_at_z)

    def gamma_t_1h_profiles(self, thetas, Ms, concs, zsource, sig_theta=None, delta=200, rho="mean", rho_at_z=True):
        """One-halo tangential shear: delta_sigma_1h_profiles / Sigma_crit(z, zsource)."""
        dsigma = self.delta_sigma_1h_profiles(thetas, Ms, concs, sig_theta=sig_theta, delta=delta, rho=rho,
                                              rho_at_z=rho_at_z)
        return self._over_sigma_crit(dsigma, zsource)

    def _lensing_1h(self, profile, thetas, Ms, concs, sig_theta, delta, rho, rho_at_z):
        """sigma_1h_profiles / delta_sigma_1h_profiles: `profile` is lensing.sigma_nfw or lensing.delta_sigma_nfw."""
        th = self._lensing_thetas(thetas)
        Ms, _, rows = self._lensing_halos(Ms, concs, delta, rho, rho_at_z)
        if sig_theta is not None and (not np.isfinite(sig_theta) or sig_theta < 0):
            raise ValueError("sig_theta must be finite and non-negative")
        nz, nM, nt = self._nz, Ms.size, th.size
        rs = np.concatenate([r[1] for r in rows])
        dc = np.concatenate([r[2] for r in rows])
        rhoc = np.repeat([r[3] for r in rows], nM)
        rbins = np.repeat(np.stack([r[0] * th for r in rows]), nM, axis=0)           # (nz nM, ntheta)
        offsets = None
        if sig_theta is not None and sig_theta > 0:
            offsets = np.repeat([r[0] * float(sig_theta) for r in rows], nM)
        prof = profile(rs, dc, rhoc, rbins, offsets=offsets, ctx=self._main()).reshape(nz, nM, nt)
        return prof[0] if nz == 1 else prof

    def kappa_1h_profiles(self, thetas, Ms, concs, zsource, sig_theta=None, delta=200, rho="mean", rho_at_z=True):
        """sigma_1h_profiles / Sigma_crit(z, zsource) (hmvec/hmvec.py:592-595)."""
        sigma = self.sigma_1h_profiles(thetas, Ms, concs, sig_theta=sig_theta, delta=delta, rho=rho,
                                       rho_at_z=rho_at_z)
        return self._over_sigma_crit(sigma, zsource)

    def _over_sigma_crit(self, prof, zsource):
        """A one-halo profile ((nM, ntheta), or (nz, nM, ntheta)) over Sigma_crit(z, zsource) of its lens redshift."""
        sigmac = np.concatenate([np.atleast_1d(self.sigma_crit(np.array([z]), zsource)) for z in self.zs])
        return prof / sigmac[0] if self._nz == 1 else prof / sigmac[:, None, None]

    def kappa_2h_profiles(self, thetas, Ms, zsource, delta=200, rho="mean", rho_at_z=True, lmin=100, lmax=10000,
                          verbose=True):
        """Two-halo convergence (hmvec/hmvec.py:597-625) at angles thetas [rad] for halo masses Ms: (ntheta, nM), or
        (nz, ntheta, nM) with several lens redshifts.  delta, rho and rho_at_z are accepted and unused, as in the
        reference.  Ms outside the model's mass grid raise ValueError (the reference's interp1d does)."""
        return self._lensing_2h(kappa_2h_integral, thetas, Ms, zsource, lmin, lmax, verbose)

    def gamma_t_2h_profiles(self, thetas, Ms, zsource, delta=200, rho="mean", rho_at_z=True, lmin=100, lmax=10000,
                            verbose=True):
        """Two-halo tangential shear: kappa_2h_profiles with J0(l theta) replaced by J2(l theta)
        (Oguri & Takada 2011), same arguments, conventions and shapes: (ntheta, nM), or (nz, ntheta, nM)."""
        return self._lensing_2h(gamma_t_2h_integral, thetas, Ms, zsource, lmin, lmax, verbose)

    def delta_sigma_2h_profiles(self, thetas, Ms, delta=200, rho="mean", rho_at_z=True, lmin=100, lmax=10000,
                                verbose=True):
        """Two-halo excess surface density Sigma_crit(z, zsource) gamma_t^2h [Msun/Mpc^2]: gamma_t_2h_profiles without
        its 1/Sigma_crit, so no source redshift.  Shapes and keywords as kappa_2h_profiles; verbose prints the bias."""
        return self._lensing_2h(gamma_t_2h_integral, thetas, Ms, None, lmin, lmax, verbose)

    def sigma_2h_profiles(self, thetas, Ms, delta=200, rho="mean", rho_at_z=True, lmin=100, lmax=10000,
                          verbose=True):
        """Two-halo surface density Sigma_crit(z, zsource) kappa_2h [Msun/Mpc^2]: kappa_2h_profiles without its
        1/Sigma_crit, so no source redshift.  Shapes and keywords as kappa_2h_profiles; verbose prints the bias."""
        return self._lensing_2h(kappa_2h_integral, thetas, Ms, None, lmin, lmax, verbose)

    def _lensing_2h(self, integral, thetas, Ms, zsource, lmin, lmax, verbose):
        """The two-halo profiles: `integral` is lensing.kappa_2h_integral (J0) or gamma_t_2h_integral (J2); pre(z)
        carries 1/Sigma_crit(z, zsource) unless zsource is None."""
        th = self._lensing_thetas(thetas)
        Ms = np.atleast_1d(np.asarray(Ms, dtype=np.float64)).ravel()       # (finite and positive: `integral` checks)
        if np.any(Ms < self.ms[0]) or np.any(Ms > self.ms[-1]):
            raise ValueError("A value in x_new is outside the interpolation range of the model's mass grid")
        chi, pre, sigmac = [], [], []
        for z in self.zs:
            zz = np.array([z])
            dA = self.angular_diameter_distance(zz)
            if zsource is None:
                pre.append((self.rho_matter_z(zz) / (1 + zz) ** 3.0 / dA ** 2)[0])
            else:
                sc = np.atleast_1d(self.sigma_crit(zz, zsource))
                pre.append((self.rho_matter_z(zz) / (1 + zz) ** 3.0 / sc / dA ** 2)[0])
                sigmac.append(sc[0])
            chi.append(np.atleast_1d(self.comoving_radial_distance(zz))[0])
        ctx = self._main(needs_aux=True)
        out = integral(self.ks, np.array(chi), np.array(pre), self._d_Pzk(), th, lmin, lmax, self.ms, self._d_bh, Ms,
                       ctx=ctx)
        if verbose:
            bhs = np.stack([np.interp(Ms, self.ms, b) for b in self.bh])
            print("bias ", bhs)
            if zsource is not None:
                print("sigmacr ", np.array(sigmac))
        return out[0] if self._nz == 1 else out
