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

from . import _native as nat
from ._native import as_device as _dev, context_or_default as _context
from .quadrature import gauss_legendre_unit

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
