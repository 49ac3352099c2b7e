"""Projected gas and pressure profiles on the GPU: the batched function of plain arrays behind
HaloModel.gas_sigma_1h_profiles, gas_delta_sigma_1h_profiles, tau_1h_profiles and y_1h_profiles.

``projected_gnfw`` works in the scaled units of the generalised NFW family f(x) = x^gamma (1 + x^alpha)^(-eta), truncated
at xcut: the line-of-sight projection F(s), its mean G(s) inside a disc of radius s, the excess G - F, and F convolved with
a circular Gaussian (a telescope beam, or Rayleigh-distributed miscentring).  The Battaglia gas density and pressure
profiles are members of the family.  The kernels are in hmvec_amd/csrc/kernels/gasproj.hpp.
"""
import ctypes as C

import numpy as np
import scipy.constants as constants

from . import _native as nat
from ._native import as_device as _dev, context_or_default as _context
from .params import default_params
from .utils import _R_from_M

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


_X_H = 0.76      # hydrogen mass fraction of the Battaglia profiles (hmvec/hmvec.py:922)


def _battaglia_fit(m200c, z, A0, alpham, alphaz):
    """A0 (M200c / 1e14)^alpha_m (1+z)^alpha_z on the host (hmvec/hmvec.py:800-802)."""
    return A0 * (m200c / 1.0e14) ** alpham * (1.0 + z) ** alphaz


def _mdelta_host(M1, c1, drho1, drho2):
    """Mass in the definition Delta rho = drho2 of NFW halos of mass M1 and concentration c1 in the definition drho1
    (hmvec/hmvec.py:770-798) on the host: equal r_s and rho_s give M2 / F(c2) = M1 / F(c1) with
    c2 = c1 (M2 drho1 / (M1 drho2))^(1/3), F(c) = ln(1+c) - c/(1+c); Newton in ln(M2/M1) to machine precision."""
    def F(c):
        return np.log1p(c) - c / (1.0 + c)
    lnF1 = np.log(F(c1))
    lq = np.zeros_like(M1)
    for _ in range(60):
        c2 = c1 * (np.exp(lq) * drho1 / drho2) ** (1.0 / 3.0)
        F2 = F(c2)
        resid = lq - np.log(F2) + lnF1
        dlnF = c2 * c2 / (1.0 + c2) ** 2 / F2           # d ln F / d ln c
        step = resid / (1.0 - dlnF / 3.0)
        lq = lq - step
        if np.all(np.abs(step) < 1e-15):
            break
    return M1 * np.exp(lq)


def halo_rings(halos, rowfn, truncate, angles):
    """The per-redshift loop over the rows of _gas_halos that the projected profiles and the rings of the one-point PDF
    share; angles[z]: the angles [rad] of redshift z, (1, ntheta) or one row per halo.  Yields per redshift
    (x, alpha, eta, xcut, pref, r, gamma): the arguments of the projection in scaled units, the prefactor and the scale
    radius of every halo, and the family's gamma.  The beam width in scaled units is left to the caller: the two do not
    form it with the same operations."""
    for (z, da, rhoc, rvir, m200c, r200c), ang in zip(halos, angles):
        r, al, gamma, et, pf = rowfn(z, rhoc, m200c, r200c)
        yield da * ang / r[:, None], al + 0.0 * r, et, truncate * rvir / r, pf, r, gamma


class GasProjectionMixin:
    """HaloModel's projected gas and pressure profiles.  Per-halo scalars on the host, one redshift
    at a time, as for the cluster-lensing profiles: a z slice of a batch is bit for bit a single-z model's result."""

    def _gas_halos(self, Ms, concs, truncate):
        """(Ms, [(z, D_A, rho_crit, r_vir, M200c, R200c) per z]) with the mass conversion of add_battaglia_profile
        (hmvec/hmvec.py:215-225): the model's mass definition -> 200 rho_crit(z), concs=None the Duffy concentration."""
        Ms = np.atleast_1d(np.asarray(Ms, dtype=np.float64)).ravel()
        if not np.all(np.isfinite(Ms)) or np.any(Ms <= 0):
            raise ValueError("Ms must be finite and positive")
        if concs is not None:
            concs = np.atleast_1d(np.asarray(concs, dtype=np.float64)).ravel()
            if concs.size != Ms.size:
                raise ValueError("Ms and concs must have the same length")
            if not np.all(np.isfinite(concs)) or np.any(concs <= 0):
                raise ValueError("concs must be finite and positive")
        if not np.isfinite(truncate) or truncate <= 0:
            raise ValueError("truncate must be finite and positive")
        A, al, be = (float(self.p[f"duffy_{k}_{self.mdef}"]) for k in ("A", "alpha", "beta"))
        rows = []
        for z in self.zs:
            zz = np.array([z])
            rhoc = float(self.rho_critical_z(zz)[0])
            if self.mdef == "vir":
                drho1 = rhoc * float(self.deltav(zz)[0])
            elif self.mdef == "mean":
                drho1 = float(self.rho_matter_z(zz)[0]) * 200.0
            else:
                raise NotImplementedError(self.mdef)
            cs = A * (self.h * Ms / 2.0e12) ** al * (1.0 + z) ** be if concs is None else concs
            m200c = _mdelta_host(Ms, cs, drho1, 200.0 * rhoc)
            rows.append((float(z), float(self.angular_diameter_distance(zz)[0]), rhoc,
                         _R_from_M(Ms, drho1, delta=1.0), m200c, _R_from_M(m200c, rhoc, delta=200.0)))
        return Ms, rows

    def _projected_profile(self, kind, thetas, Ms, concs, truncate, fwhm, rowfn, norm="fit"):
        """prefactor x projected_gnfw(kind) for every (z, M, theta).  rowfn(z, rho_crit, M200c, R200c) returns the halo's
        (scale radius, alpha, gamma, eta, prefactor) with gamma one number.  norm="mass": the prefactor is M / (N r^2)
        instead, N = 4 pi int_0^xcut x^2 f dx from the "mean" kind at s = xcut."""
        th = self._lensing_thetas(thetas)
        if norm not in ("fit", "mass"):
            raise ValueError(f"norm must be 'fit' or 'mass', got {norm!r}")
        if fwhm is not None and (not np.isfinite(fwhm) or fwhm < 0):
            raise ValueError("fwhm must be finite and non-negative")
        Ms, halos = self._gas_halos(Ms, concs, truncate)
        x, alpha, eta, xcut, pref, rscale, (*_, gamma) = zip(*halo_rings(halos, rowfn, truncate, [th[None, :]] * len(halos)))
        smooth = [da * float(fwhm or 0.0) / np.sqrt(8.0 * np.log(2.0)) / r for (_, da, *_), r in zip(halos, rscale)]
        x, alpha, eta, xcut, pref, smooth, rscale = (np.concatenate(a) for a in (x, alpha, eta, xcut, pref, smooth, rscale))
        ctx = self._main()
        if norm == "mass":
            N = projected_gnfw(xcut[:, None], alpha, gamma, eta, xcut, kind="mean", ctx=ctx)[:, 0] * np.pi * xcut ** 2
            pref = np.tile(Ms, self._nz) / (N * rscale ** 2)
        prof = projected_gnfw(x, alpha, gamma, eta, xcut, kind=kind, smooth=smooth if fwhm else None, ctx=ctx)
        prof = (pref[:, None] * prof).reshape(self._nz, Ms.size, th.size)
        return prof[0] if self._nz == 1 else prof

    def _gas_rowfn(self, family, param_override):
        """Battaglia gas density (hmvec/hmvec.py:844-860) as a member of the family: x = r / (R200c / 2),
        eta = (beta + gamma) / alpha, amplitude (Omega_b / Omega_m) rho_crit(z) rho0 times the scale radius."""
        pp = self._battaglia_gas_pparams(family, param_override)
        gamma = float(pp["battaglia_gas_gamma"])
        fb = self.p["ombh2"] / self.h ** 2.0 / self.omm0

        def rowfn(z, rhoc, m200c, r200c):
            rho0, alpha, beta = (_battaglia_fit(m200c, z, *(pp[q + s] for s in ("A0", "alpham", "alphaz")))
                                 for q in ("rho0_", "alpha_", "beta_"))
            rg = 0.5 * r200c
            return rg, alpha, gamma, (beta + gamma) / alpha, fb * rhoc * rho0 * rg
        return rowfn

    def gas_sigma_1h_profiles(self, thetas, Ms, concs=None, family=None, param_override=None, truncate=1.0, norm="fit",
                              fwhm=None):
        """Projected gas surface density Sigma_gas [Msun/Mpc^2] of the Battaglia gas profile (the profile of
        add_battaglia_profile) around halos of mass Ms (the model's mass definition; concs=None: Duffy) at angles thetas
        [rad]: (nM, ntheta), or (nz, nM, ntheta) with several redshifts.  The profile is cut at truncate r_vir.
        norm="fit": the amplitude of the fit, (Omega_b / Omega_m) rho_crit(z) rho0; norm="mass": the same shape holding
        the halo mass Ms inside the cut (the profile whose transform uk_profiles approximates).  fwhm [rad]: convolved
        with a circular Gaussian beam of that full width at half maximum.  family and param_override as in
        add_battaglia_profile."""
        return self._projected_profile("sigma", thetas, Ms, concs, truncate, fwhm,
                                       self._gas_rowfn(family, param_override), norm)

    def gas_delta_sigma_1h_profiles(self, thetas, Ms, concs=None, family=None, param_override=None, truncate=1.0,
                                    norm="fit"):
        """Excess gas surface density Sigmabar_gas(<R) - Sigma_gas(R) [Msun/Mpc^2]; arguments, conventions and shapes of
        gas_sigma_1h_profiles (no beam)."""
        return self._projected_profile("excess", thetas, Ms, concs, truncate, None,
                                       self._gas_rowfn(family, param_override), norm)

    def tau_1h_profiles(self, thetas, Ms, concs=None, family=None, param_override=None, truncate=1.0, fwhm=None):
        """Thomson optical depth tau(theta) = sigma_T (1 + X_H) / (2 m_p) Sigma_gas of fully ionised gas with hydrogen
        mass fraction X_H = 0.76 (norm="fit"); dimensionless.  Arguments and shapes of gas_sigma_1h_profiles."""
        sigma_gas = self.gas_sigma_1h_profiles(thetas, Ms, concs=concs, family=family, param_override=param_override,
                                               truncate=truncate, norm="fit", fwhm=fwhm)
        sigmaT = constants.physical_constants["Thomson cross section"][0] / (default_params["parsec"] * 1e6) ** 2
        m_p = constants.physical_constants["proton mass"][0] / default_params["mSun"]
        return sigmaT * (1.0 + _X_H) / (2.0 * m_p) * sigma_gas

    def y_1h_profiles(self, thetas, Ms, concs=None, family=None, param_override=None, truncate=1.0, fwhm=None):
        """Compton-y profile y(theta) = sigma_T / (m_e c^2) int P_e dl of the Battaglia pressure profile (the profile of
        add_battaglia_pres_profile; hmvec/hmvec.py:906-927, units of 313-316), dimensionless: (nM, ntheta), or
        (nz, nM, ntheta).  Arguments as gas_sigma_1h_profiles; family and param_override as in
        add_battaglia_pres_profile."""
        return self._projected_profile("sigma", thetas, Ms, concs, truncate, fwhm, self._pres_rowfn(family, param_override))

    def _pres_rowfn(self, family, param_override):
        """Battaglia pressure profile as a member of the family, in Compton-y units: x = r / (xc R200c), eta = beta,
        amplitude sigma_T / (m_e c^2) A_P times the scale radius."""
        pp = self._battaglia_pres_pparams(family, param_override)
        gamma, alpha = float(pp["battaglia_pres_gamma"]), float(pp["battaglia_pres_alpha"])
        eFrac = 2.0 * (_X_H + 1.0) / (5.0 * _X_H + 3.0)
        G_newt = constants.G / (default_params["parsec"] * 1e6) ** 3 * default_params["mSun"]
        sigmaT = constants.physical_constants["Thomson cross section"][0]
        mElect = constants.physical_constants["electron mass"][0] / default_params["mSun"]
        fb = self.p["ombh2"] / self.h ** 2.0 / self.omm0

        def rowfn(z, rhoc, m200c, r200c):
            P0, xc, beta = (_battaglia_fit(m200c, z, *(pp[q + s] for s in ("A0", "alpham", "alphaz")))
                            for q in ("P0_", "xc_", "beta_"))
            rp = xc * r200c
            A_P = eFrac * fb * 200.0 * m200c * G_newt * rhoc / (2.0 * r200c) * P0
            return rp, alpha, gamma, beta, sigmaT / (mElect * constants.c ** 2) * A_P * rp
        return rowfn
