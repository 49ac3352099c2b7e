"""Independent numpy model of the one-point contractions, written from the formulas: for samples
(z, m, t) with weight W = zw[z] wm[m] n[z, m] a[z, m, t] and signal s[z, m, t],

    A[z, j] = sum_{m, t} W (exp(i lambda_j s) - 1),   lambda_j = j dlambda,
    K[z, p - 1] = sum_{m, t} W s^p,   p = 1 .. 4,

in np.longdouble: the weights, lambda_j and the phase phi = lambda_j s are formed in long double from the float64 inputs,
and the real part of a term is -2 sin^2(phi / 2).  Shared by tests/test_onepoint_cpu.py and tests/test_gpu_onepoint.py;
nothing here calls the library."""
import numpy as np

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
# Worst relative error of the default ring rule (256 Gauss-Legendre nodes) on the disc integral of the truncated pressure
# profile, as tests/test_onepoint_cpu.py measures it, and the gate of the end-to-end GPU test built on it by the
# convention of tests/test_gpu_gas_profiles.py.
RING_ERROR = 5.91e-9
RING_GATE = min(1e-6, max(1e-10, 100.0 * RING_ERROR))


def weights(area, nzm, wm, zw, window=None, dtype=LD):
    """W (nz, nmw, nt) of the mass window (m_lo, m_hi)."""
    lo, hi = (0, np.shape(nzm)[1]) if window is None else window
    a, n, w, g = (np.asarray(v, dtype=dtype) for v in (area, nzm, wm, zw))
    return g[:, None, None] * w[None, lo:hi, None] * n[:, lo:hi, None] * a[:, lo:hi, :]


def exponent(signal, area, nzm, wm, zw, nlambda, dlambda, window=None, K=None, dtype=LD):
    """(A, bound): A (nz, nlambda) complex128 rounded from the long-double sums, and - where K is given - the gate
    bound[z, j] = eps sum |W| (|phi| + K min(|phi|, 2)) as float64."""
    lo, hi = (0, np.shape(nzm)[1]) if window is None else window
    W = weights(area, nzm, wm, zw, window, dtype).reshape(len(zw), -1)                 # (nz, n)
    s = np.asarray(signal, dtype=dtype)[:, lo:hi, :].reshape(len(zw), -1)
    lam = np.arange(nlambda).astype(dtype) * dtype(dlambda)
    A = np.empty((len(zw), nlambda), dtype=np.complex128)
    bound = None if K is None else np.empty((len(zw), nlambda))
    for z in range(len(zw)):                                                          # (one redshift at a time: memory)
        phi = lam[:, None] * s[z][None, :]                                            # (nl, n)
        A[z].real = np.sum(W[z] * (-2 * np.sin(phi / 2) ** 2), axis=-1).astype(np.float64)
        A[z].imag = np.sum(W[z] * np.sin(phi), axis=-1).astype(np.float64)
        if K is not None:
            bound[z] = EPS * np.sum(np.abs(W[z]) * (np.abs(phi) + K * np.minimum(np.abs(phi), 2)), axis=-1)
    return A, bound


def moments(signal, area, nzm, wm, zw, window=None, dtype=LD):
    """K (nz, 4) float64 rounded from the long-double sums."""
    lo, hi = (0, np.shape(nzm)[1]) if window is None else window
    W = weights(area, nzm, wm, zw, window, dtype).reshape(len(zw), -1)
    s = np.asarray(signal, dtype=dtype)[:, lo:hi, :].reshape(len(zw), -1)
    return np.stack([np.sum(W * s ** p, axis=-1) for p in (1, 2, 3, 4)], axis=-1).astype(np.float64)


def pdf(A, ds, smin=0.0, noise_sigma=0.0):
    """(s, p) from the exponent A (nlambda,) on lambda_j = 2 pi j / (N ds), N = 2 (nlambda - 1), by the direct sum
    p_b = (1/N) [phi_0 + 2 sum_{0<j<N/2} Re(phi_j e^{-i lambda_j s_b}) + Re(phi_{N/2} e^{-i lambda_{N/2} s_b})] of the
    characteristic function phi_j = exp(A_j - lambda_j^2 sigma^2 / 2): no FFT, O(N^2)."""
    A = np.asarray(A, dtype=np.complex128)
    n = 2 * (A.size - 1)
    lam = 2.0 * np.pi * np.arange(A.size) / (n * ds)
    phi = np.exp(A - 0.5 * (lam * noise_sigma) ** 2)
    s = smin + ds * np.arange(n)
    term = np.real(phi[None, :] * np.exp(-1j * lam[None, :] * s[:, None]))
    wgt = np.full(A.size, 2.0)
    wgt[0] = wgt[-1] = 1.0
    return s, term @ wgt / n
