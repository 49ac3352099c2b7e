"""The one-point PDF of a field that is a sum of halo profiles on the sky - P(y) of a Compton-y map, P(kappa) - and its
cumulants: the functions of plain arrays behind HaloModel.get_y_pdf, get_y_cumulants,
get_y_char_exponent and profile_char_exponent.

For Poisson-placed halos the characteristic function of the field is <exp(i lambda s)> = exp A(lambda),

    A(lambda) = sum_z zw[z] sum_m wm[m] n[z, m] sum_t a[z, m, t] (exp(i lambda s[z, m, t]) - 1),

s the profile at ring t of a halo of mass ms[m] at zs[z] and a the ring's solid angle; the cumulants are
kappa_p = sum zw wm n a s^p.  ``char_exponent`` and ``cumulants`` are the two contractions on the GPU
(hmvec_amd/csrc/kernels/onepoint.hpp); ``pdf_from_exponent`` is the transform of the nbins numbers exp A on the host.
Overlapping halos are included (that is what the exponential does); halo clustering is not.
"""
import numpy as np
import scipy.constants as constants

from . import _native as nat
from . import gasprofiles
from ._native import as_device as _dev, context_or_default as _context
from .quadrature import gauss_legendre_unit, trapz_weights

__all__ = ["char_exponent", "cumulants", "pdf_from_exponent", "lambda_grid", "ring_rule", "chain_length",
           "MAX_BINS", "MAX_RINGS", "DEFAULT_RINGS"]

MAX_BINS = 1 << 20          # bins of the PDF in one call: nlambda = MAX_BINS / 2 + 1 values of lambda
MAX_RINGS = 1024            # nodes of the ring rule
DEFAULT_RINGS = 256         # the truncated pressure profile's disc integral to 6e-9 (64 rings: 5e-7)

# the kernels' constants (csrc/kernels/onepoint.hpp)
_THREADS, _WAVES, _RADIX, _SLICE, _MAXSPLIT = 256, 4, 8, 4096, 8


def _ladder(n):
    """Additions on the longest chain of the kernels' ladder of accumulators over n terms."""
    return min(n, _RADIX) + min(n // _RADIX, _RADIX) + min(n // _RADIX ** 2, _RADIX) + n // _RADIX ** 3 + 3


def chain_length(nm_used, nt):
    """The longest chain of floating-point additions behind one output of a row of char_exponent or cumulants (the larger
    of the two) over nm_used masses x nt rings: a plain count from the kernels' constants.  The exponent's samples go to
    split = min(8, ceil(count / 4096)) slices of four wavefronts, each a ladder over its share, then 3 additions for the
    wavefronts and split - 1 for the slices; the moments' to 256 threads, each a ladder, then a tree of 8."""
    count = int(nm_used) * int(nt)
    if nm_used < 1 or nt < 1:
        raise ValueError("nm_used and nt must be at least 1")
    split = min(_MAXSPLIT, max(1, -(-count // _SLICE)))
    exponent = _ladder(-(-count // (_WAVES * split))) + (_WAVES - 1) + (split - 1)
    moments = _ladder(-(-count // _THREADS)) + 8
    return max(exponent, moments)


def lambda_grid(nbins, ds):
    """(nlambda, dlambda) of a PDF of nbins bins of width ds: nlambda = nbins / 2 + 1 values lambda_j = j dlambda,
    dlambda = 2 pi / (nbins ds).  nbins must be even, 4 <= nbins <= MAX_BINS; ds finite and positive."""
    if not isinstance(nbins, (int, np.integer)) or isinstance(nbins, bool) or nbins < 4 or nbins > MAX_BINS or nbins % 2:
        raise ValueError(f"nbins must be an even integer in 4 .. {MAX_BINS}, got {nbins!r}")
    ds = _positive("ds", ds)
    return int(nbins) // 2 + 1, 2.0 * np.pi / (int(nbins) * ds)


def _positive(name, v):
    try:
        v = float(v)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be a finite positive number, got {v!r}") from None
    if not np.isfinite(v) or v <= 0.0:
        raise ValueError(f"{name} must be a finite positive number, got {v!r}")
    return v


def check_rings(ntheta):
    if not isinstance(ntheta, (int, np.integer)) or isinstance(ntheta, bool) or not 2 <= ntheta <= MAX_RINGS:
        raise ValueError(f"ntheta must be an integer in 2 .. {MAX_RINGS}, got {ntheta!r}")
    return int(ntheta)


def ring_rule(ntheta=DEFAULT_RINGS):
    """(u, w): the ntheta-node Gauss-Legendre rule on (0, 1] (quadrature.gauss_legendre_unit), 2 <= ntheta <= MAX_RINGS.
    The rings of a halo whose profile ends at theta_out are at theta_t = theta_out u_t and have the solid angle
    a_t = 2 pi theta_out^2 u_t w_t: sum_t a_t f(theta_t) is the integral of f over the disc."""
    return gauss_legendre_unit(check_rings(ntheta))


def check_noise(noise_sigma):
    try:
        v = float(noise_sigma)
    except (TypeError, ValueError):
        raise ValueError(f"noise_sigma must be a finite number >= 0, got {noise_sigma!r}") from None
    if not np.isfinite(v) or v < 0.0:
        raise ValueError(f"noise_sigma must be a finite number >= 0, got {noise_sigma!r}")
    return v


def check_window(mwindow, nm):
    """(m_lo, m_hi) of a mass index window; None: the whole grid."""
    if mwindow is None:
        return 0, int(nm)
    try:
        lo, hi = mwindow
        ok = all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) for v in (lo, hi))
    except (TypeError, ValueError):
        ok = False
    if not ok or not 0 <= lo < hi <= nm:
        raise ValueError(f"mwindow must be a pair of indices (m_lo, m_hi) with 0 <= m_lo < m_hi <= nm = {nm}, got {mwindow!r}")
    return int(lo), int(hi)


def check_zweights(zw, nz):
    zw = np.ascontiguousarray(zw, dtype=np.float64)
    if zw.shape != (nz,) or not np.all(np.isfinite(zw)):
        raise ValueError(f"zweights must be finite with one entry per redshift, shape ({nz},), got shape {zw.shape}")
    return zw


def _finite(name, a, shape):
    """A host array checked for shape and finiteness; a DeviceArray checked for shape alone (its values stay where they
    are)."""
    if isinstance(a, nat.DeviceArray):
        if a.shape != shape:
            raise ValueError(f"{name} must have shape {shape}, got {a.shape}")
        return a
    a = np.ascontiguousarray(a, dtype=np.float64)
    if a.shape != shape:
        raise ValueError(f"{name} must have shape {shape}, got {a.shape}")
    if not np.all(np.isfinite(a)):
        raise ValueError(f"{name} must be finite")
    return a


def _request(signal, area, nzm, wm, zw, mwindow):
    """The checked inputs of a contraction: every refusal happens here on the host, before a context is touched."""
    shape = signal.shape if isinstance(signal, nat.DeviceArray) else np.shape(signal)
    if len(shape) != 3 or min(shape) < 1:
        raise ValueError(f"signal must have shape (nz, nm, nt), each at least 1, got {tuple(shape)}")
    nz, nm, nt = (int(v) for v in shape)
    signal = _finite("signal", signal, (nz, nm, nt))
    area = _finite("area", area, (nz, nm, nt))
    nzm = _finite("nzm", nzm, (nz, nm))
    wm = _finite("wm", wm, (nm,))
    zw = zw if isinstance(zw, nat.DeviceArray) and zw.shape == (nz,) else check_zweights(zw, nz)
    return (signal, area, nzm, wm, zw), (nz, nm, nt), check_window(mwindow, nm)


def _launch(ctx, entry, arrays, amp, dims, window, extra, width, per_z):
    """One contraction on the device: rows (nz, width) and, unless per_z, their sum over z, fetched to the host."""
    nz, nm, nt = dims
    d_signal, d_area, d_nzm, d_wm, d_zw = (_dev(ctx, a) for a in arrays)
    d_amp = None if amp is None else _dev(ctx, amp)
    rows = ctx.empty((nz, width))
    total = None if per_z else ctx.empty((width,))
    ctx.call(entry, nz=nz, nm=nm, nt=nt, d_signal=d_signal.ptr, d_area=d_area.ptr, d_amp=nat.ptr(d_amp), d_nzm=d_nzm.ptr,
             d_wm=d_wm.ptr, d_zw=d_zw.ptr, m_lo=window[0], m_hi=window[1], **extra, d_rows=rows.ptr, d_total=nat.ptr(total))
    return (rows if per_z else total).numpy()


def _exponent(ctx, arrays, amp, dims, window, nlambda, dlambda, per_z):
    out = _launch(ctx, "hmg_onepoint_exponent", arrays, amp, dims, window, dict(nlambda=nlambda, dlambda=dlambda), 2 * nlambda,
                  per_z)
    out = out.reshape(-1, 2, nlambda)
    A = np.empty((out.shape[0], nlambda), dtype=np.complex128)
    A.real, A.imag = out[:, 0], out[:, 1]
    return A if per_z else A[0]


def _moments(ctx, arrays, amp, dims, window, per_z):
    return _launch(ctx, "hmg_onepoint_moments", arrays, amp, dims, window, {}, 4, per_z)


def check_lambda(nlambda, dlambda):
    if not isinstance(nlambda, (int, np.integer)) or isinstance(nlambda, bool) or not 1 <= nlambda <= MAX_BINS // 2 + 1:
        raise ValueError(f"nlambda must be an integer in 1 .. {MAX_BINS // 2 + 1}, got {nlambda!r}")
    return int(nlambda), _positive("dlambda", dlambda)


def char_exponent(signal, area, nzm, wm, zw, nlambda, dlambda, mwindow=None, per_z=False, ctx=None):
    """A(lambda_j) = sum_z zw[z] sum_m wm[m] nzm[z, m] sum_t area[z, m, t] (exp(i lambda_j signal[z, m, t]) - 1) on the grid
    lambda_j = j dlambda, j < nlambda: complex128 (nlambda,), or with per_z=True its rows (nz, nlambda), each already
    multiplied by zw[z].  signal, area: (nz, nm, nt); nzm: (nz, nm); wm: (nm,); zw: (nz,); host arrays or device buffers.
    mwindow = (m_lo, m_hi): only the masses m_lo <= m < m_hi.  The real part is formed as -2 sin^2(lambda s / 2), so it
    keeps its digits at small phases; A[0] is exactly 0.  A row of a batch has the bits of the call with that redshift
    alone, and a repeated call the bits of the first."""
    arrays, dims, window = _request(signal, area, nzm, wm, zw, mwindow)
    nlambda, dlambda = check_lambda(nlambda, dlambda)
    return _exponent(_context(ctx), arrays, None, dims, window, nlambda, dlambda, bool(per_z))


def cumulants(signal, area, nzm, wm, zw, mwindow=None, per_z=False, ctx=None):
    """kappa_p = sum_z zw[z] sum_m wm[m] nzm[z, m] sum_t area[z, m, t] signal[z, m, t]^p, p = 1 .. 4: the mean, the
    variance and the third and fourth cumulant of the field whose exponent char_exponent gives; (4,), or with per_z=True
    (nz, 4).  Arguments as char_exponent."""
    arrays, dims, window = _request(signal, area, nzm, wm, zw, mwindow)
    return _moments(_context(ctx), arrays, None, dims, window, bool(per_z))


def pdf_from_exponent(A, ds, smin=0.0, noise_sigma=0.0):
    """(s, p): the PDF of the field from its exponent A (nlambda,) on lambda_grid(N, ds), N = 2 (nlambda - 1) bins at
    s_b = smin + b ds; p is the probability per bin (the density times ds) and sums to 1.  With lambda_j = 2 pi j / (N ds)

        p = irfft(conj(exp(A_j - lambda_j^2 noise_sigma^2 / 2) exp(-i lambda_j smin)), n=N):

    noise_sigma is the width of Gaussian noise added to the field (the map's noise).  Host numpy: a transform of N
    numbers.  The result is periodic with period N ds - whatever of the PDF lies outside [smin, smin + N ds) is folded
    back in.  Without noise the PDF has a point mass at 0 (the sky no halo covers) and edge singularities, and the
    result rings: add the map's noise, or keep noise_sigma >~ 2 ds."""
    A = np.asarray(A)
    if A.ndim != 1 or A.size < 3 or not np.all(np.isfinite(A)):
        raise ValueError(f"A must be a finite one-dimensional array of nlambda >= 3 values, got shape {A.shape}")
    ds = _positive("ds", ds)
    sigma = check_noise(noise_sigma)
    smin = float(smin)
    if not np.isfinite(smin):
        raise ValueError("smin must be finite")
    n = 2 * (A.size - 1)
    lam = 2.0 * np.pi * np.arange(A.size) / (n * ds)
    phi = np.exp(A.astype(np.complex128) - 0.5 * (lam * sigma) ** 2) * np.exp(-1j * lam * smin)
    return smin + ds * np.arange(n), np.fft.irfft(np.conj(phi), n=n)


class OnePointMixin:
    """HaloModel's one-point PDF (hmg_onepoint_exponent, hmg_onepoint_moments).  Every refusal happens on the host before
    a context is touched: the *_request methods check and build host arrays (the halos and the pressure profile's rows
    are GasProjectionMixin's _gas_halos, _pres_rowfn), _onepoint_launch is the only one that reaches the device."""

    def _onepoint_request(self, ntheta, mmin, mmax, zweights):
        """(u, w, (m_lo, m_hi), zw) of the shared tail of the one-point methods."""
        u, w = ring_rule(ntheta)
        ms = np.asarray(self.ms, dtype=np.float64)
        for name, v in (("mmin", mmin), ("mmax", mmax)):
            if v is not None and not (np.isscalar(v) and np.isfinite(v) and v > 0):
                raise ValueError(f"{name} must be a finite positive mass or None, got {v!r}")
        keep = np.nonzero((ms >= (ms[0] if mmin is None else mmin)) & (ms <= (ms[-1] if mmax is None else mmax)))[0]
        if keep.size == 0:
            raise ValueError(f"no point of the mass grid lies in mmin .. mmax = {mmin!r} .. {mmax!r}")
        if zweights is None:
            if self._nz < 2:
                raise ValueError("zweights=None needs at least two redshifts (the default is a trapezoid rule over zs times "
                                 "the comoving volume per steradian); give the weight of the one redshift")
            zs = np.asarray(self.zs, dtype=np.float64)
            chi = np.asarray(self.comoving_radial_distance(zs), dtype=np.float64).reshape(-1)
            hz = np.asarray(self.hubble_parameter(zs), dtype=np.float64).reshape(-1)
            zweights = trapz_weights(zs) * (constants.c / 1.0e3) * chi ** 2 / hz       # dz dV/dz/dOmega, comoving Mpc^3/sr
        return u, w, (int(keep[0]), int(keep[-1]) + 1), check_zweights(zweights, self._nz)

    def _profile_request(self, profiles, theta_out, ntheta, mmin, mmax, zweights):
        u, w, window, zw = self._onepoint_request(ntheta, mmin, mmax, zweights)
        shape = (self._nz, self._nm, u.size)
        got = profiles.shape if isinstance(profiles, nat.DeviceArray) else np.shape(profiles)
        if tuple(got) != shape:
            raise ValueError(f"profiles must have shape (nz, nm, ntheta) = {shape}, got {tuple(got)}")
        if not isinstance(profiles, nat.DeviceArray):
            profiles = np.ascontiguousarray(profiles, dtype=np.float64)
            if not np.all(np.isfinite(profiles)):
                raise ValueError("profiles must be finite")
        theta_out = np.asarray(theta_out, dtype=np.float64)
        if theta_out.shape != shape[:2]:
            raise ValueError(f"theta_out must have shape (nz, nm) = {shape[:2]}, got {theta_out.shape}")
        if not np.all(np.isfinite(theta_out)) or np.any(theta_out <= 0):
            raise ValueError("theta_out must be finite and positive")
        area = (2.0 * np.pi * theta_out ** 2)[:, :, None] * (u * w)[None, None, :]
        return dict(signal=profiles, amp=None, area=area, window=window, zw=zw)

    def _y_request(self, truncate, fwhm, family, param_override, ntheta, mmin, mmax, zweights):
        """The rings of every (zs, ms) halo's Compton-y profile: the arguments of the projection in scaled units, the
        amplitudes and the solid angles, all on the host."""
        u, w, window, zw = self._onepoint_request(ntheta, mmin, mmax, zweights)
        if fwhm is not None and not (np.isscalar(fwhm) and np.isfinite(fwhm) and fwhm >= 0):
            raise ValueError("fwhm must be finite and non-negative")
        beam = float(fwhm or 0.0) / np.sqrt(8.0 * np.log(2.0))
        rowfn = self._pres_rowfn(family, param_override)
        Ms, halos = self._gas_halos(self.ms, None, truncate)
        theta_out = [truncate * rvir / da + 5.0 * beam for _, da, _, rvir, _, _ in halos]
        # (the operations of y_1h_profiles at the angles theta_out u)
        x, alpha, eta, xcut, pref, rscale, (*_, gamma) = zip(*gasprofiles.halo_rings(
            halos, rowfn, truncate, [tout[:, None] * u[None, :] for tout in theta_out]))
        smooth = [da * beam / r for (_, da, *_), r in zip(halos, rscale)]
        x, alpha, eta, xcut, smooth = (np.concatenate(a) for a in (x, alpha, eta, xcut, smooth))
        pref, theta_out = np.stack(pref), np.stack(theta_out)
        for name, a in (("the profile's parameters", np.concatenate([alpha, eta, xcut, pref.ravel()])), ("the ring radii", x)):
            if not np.all(np.isfinite(a)):
                raise ValueError(f"{name} are not finite")
        area = (2.0 * np.pi * theta_out ** 2)[:, :, None] * (u * w)[None, None, :]
        return dict(signal=None, proj=(x, alpha, gamma, eta, xcut, smooth if beam > 0 else None), amp=pref, area=area,
                    window=window, zw=zw)

    def _onepoint_launch(self, req, grid, per_z):
        """The contraction of a checked request on the device; grid = (nlambda, dlambda), or None for the cumulants."""
        ctx = self._main(needs_aux=True)
        signal = req["signal"]
        if signal is None:          # the profiles stay on the device
            signal = gasprofiles.projected_gnfw_device(*req["proj"], ctx=ctx)
        arrays = (signal, req["area"], self._d_nzm, self._d_wm(), req["zw"])
        dims = (self._nz, self._nm, req["area"].shape[-1])
        if grid is None:
            out = _moments(ctx, arrays, req["amp"], dims, req["window"], per_z)
        else:
            out = _exponent(ctx, arrays, req["amp"], dims, req["window"], *grid, per_z)
        self._sync_point()
        return out

    def profile_char_exponent(self, profiles, theta_out, nbins, ds, ntheta=DEFAULT_RINGS, mmin=None, mmax=None,
                              zweights=None, per_z=False):
        """The exponent A(lambda_j) of the characteristic function exp A of a field that is the sum of the profiles of
        Poisson-placed halos of the model's mass function, on onepoint.lambda_grid(nbins, ds): complex (nbins / 2 + 1,),
        or with per_z=True its rows (nz, nbins / 2 + 1).  profiles (nz, nm, ntheta), a host array or a device buffer, is
        the profile of a halo of mass ms[m] at zs[z] at the angles theta_out[z, m] u_t [rad], u = onepoint.ring_rule(ntheta)
        [0], and zero beyond theta_out (nz, nm) - built from kappa_1h_profiles, for instance.  zweights (nz,): the weight
        of a redshift, default trapz_weights(zs) c chi^2 / H, the comoving volume per steradian that goes with the comoving
        mass function; mmin, mmax: only the masses of the grid in [mmin, mmax].  onepoint.pdf_from_exponent turns the
        result into the PDF.  Halo clustering is neglected; overlapping halos are not."""
        grid = lambda_grid(nbins, ds)
        req = self._profile_request(profiles, theta_out, ntheta, mmin, mmax, zweights)
        return self._onepoint_launch(req, grid, bool(per_z))

    def get_y_char_exponent(self, nbins, dy, truncate=1.0, fwhm=None, family=None, param_override=None,
                            ntheta=DEFAULT_RINGS, mmin=None, mmax=None, zweights=None, per_z=False):
        """profile_char_exponent of the Compton-y profile of y_1h_profiles (the Battaglia pressure profile cut at
        truncate r_vir, Duffy concentrations; family and param_override as in add_battaglia_pres_profile) of every
        (zs, ms) halo, on lambda_grid(nbins, dy).  The rings end at theta_out = truncate r_vir / D_A, with fwhm [rad] (the
        beam the profile is convolved with) at 5 beam widths sigma = fwhm / sqrt(8 ln 2) beyond.  The profiles are
        evaluated and contracted on the device."""
        grid = lambda_grid(nbins, dy)
        req = self._y_request(truncate, fwhm, family, param_override, ntheta, mmin, mmax, zweights)
        return self._onepoint_launch(req, grid, bool(per_z))

    def get_y_pdf(self, nbins, dy, ymin=0.0, noise_sigma=0.0, truncate=1.0, fwhm=None, family=None, param_override=None,
                  ntheta=DEFAULT_RINGS, mmin=None, mmax=None, zweights=None, per_z=False):
        """(ys, p): the one-point PDF of the Compton-y map in nbins bins of width dy from ymin, p the probability per bin
        (nbins,), with Gaussian map noise of width noise_sigma - onepoint.pdf_from_exponent of get_y_char_exponent; see
        there for the periodicity and for why noise_sigma >~ 2 dy.  per_z=True: p (nz, nbins), the PDF of each redshift's
        halos alone."""
        grid = lambda_grid(nbins, dy)
        noise_sigma = check_noise(noise_sigma)
        if not (np.isscalar(ymin) and np.isfinite(ymin)):
            raise ValueError("ymin must be finite")
        req = self._y_request(truncate, fwhm, family, param_override, ntheta, mmin, mmax, zweights)
        A = self._onepoint_launch(req, grid, bool(per_z))
        if not per_z:
            return pdf_from_exponent(A, dy, ymin, noise_sigma)
        rows = [pdf_from_exponent(a, dy, ymin, noise_sigma) for a in A]
        return rows[0][0], np.stack([p for _, p in rows])

    def get_y_cumulants(self, truncate=1.0, fwhm=None, family=None, param_override=None, ntheta=DEFAULT_RINGS,
                        mmin=None, mmax=None, zweights=None, per_z=False):
        """[<y>, kappa_2, kappa_3, kappa_4]: the mean and the second to fourth cumulant of the Compton-y map of
        get_y_char_exponent (without noise), kappa_p = sum zw wm n a y^p; (4,), or with per_z=True (nz, 4)."""
        req = self._y_request(truncate, fwhm, family, param_override, ntheta, mmin, mmax, zweights)
        return self._onepoint_launch(req, None, bool(per_z))
