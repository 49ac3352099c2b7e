"""Non-Limber angular power spectra of separable sources on the GPU: the projection that is valid
at the low multipoles where every Limber statistic of the library (limber_integral, C_gg / C_kg / C_kk, the k = l / chi
transforms of section 22) is not, and the only one that can carry linear redshift-space distortions.

A spectrum that is separable between two lines of sight, P(z, z', k) = S_a(z, k) S_b(z', k), projects exactly through
one transfer function per field.  The two-halo term is of that form: P_2h = P_lin L_a L_b with L_a = I_a + b_a - C_a the
bracket of get_power_2halo (two_halo_terms), so S_a = L_a sqrt(P_lin).  In limber_integral's convention (windows per unit
z, c = 1, H in 1/Mpc), on nodes gzs with trapezoid weights wz and distances chi_g:

    src_a[g, i]  = wz_g W_a[g] S_a(z_g, kq_i)
    T_l^a(kq_i)  = sum_g src_a[g, i] j_l(kq_i chi_g)        l = 0 .. lmax                      (nonlimber_transfer)
    C_l^{ab}     = (2/pi) sum_i wk_i kq_i^2 T_l^a(kq_i) T_l^b(kq_i)                            (nonlimber_cl)

These are functions of plain arrays: the caller forms the sources.  A lensing field has its source divided by
(kq_i chi_g)^2 and T_l multiplied by l (l + 1) (its Limber limit carries l (l + 1) / (l + 1/2)^2); the Kaiser term of a
density field is - sum_g wz W f_g S_m j_l''(kq chi_g) with j_l'' = c- j_{l-2} - c0 j_l + c+ j_{l+2} - one more column of
the same transfer, taken to lmax + 2 and combined over l by the caller.  refine_gzs and nonlimber_k_rule give the two
quadrature rules.  The kernels are in hmvec_amd/csrc/kernels/nonlimber.hpp and hmvec_amd/csrc/sphbessel.hpp.
"""
import ctypes as C_

import numpy as np

from . import _native as nat
from .cosmology import z_of_chi
from .quadrature import trapz_weights

__all__ = ["spherical_bessel", "spherical_bessel_device", "nonlimber_transfer", "nonlimber_transfer_device", "nonlimber_cl",
           "nonlimber_cl_device", "refine_gzs", "nonlimber_k_rule"]

XMIN = 1e-100                      # the smallest argument of the spherical Bessel walk (sphbessel.hpp's SB_XMIN)


def fmax():
    """Fields per launch of the transfer kernel (HMG_NONLIMBER_FMAX); larger requests are split."""
    return nat.DEFINES["HMG_NONLIMBER_FMAX"]


def check_lmax(lmax):
    top = nat.DEFINES["HMG_NONLIMBER_LMAX"]
    if isinstance(lmax, bool) or not isinstance(lmax, (int, np.integer)) or not 0 <= lmax <= top:
        raise ValueError(f"lmax must be an integer in 0 .. {top}, got {lmax!r}")
    return int(lmax)


def _increasing(a, what):
    a = np.asarray(a, dtype=np.float64)
    if a.ndim != 1 or a.size < 1 or not np.all(np.isfinite(a)) or np.any(a <= 0) or np.any(np.diff(a) <= 0):
        raise ValueError(f"{what} must be a finite, positive, strictly increasing vector")
    return np.ascontiguousarray(a)


def check_rule(kq, chis):
    """The k nodes and the chi nodes of a transfer as float64 vectors: finite, positive, strictly increasing, kq chi not
    below 1e-100, and the chi rule not below Nyquist for the largest k: kq[-1] max(diff(chis)) <= pi."""
    kq, chis = _increasing(kq, "kq"), _increasing(chis, "chis")
    if kq[0] * chis[0] < XMIN:
        raise ValueError(f"kq chi must be at least {XMIN}")
    if chis.size > 1 and kq[-1] * np.max(np.diff(chis)) > np.pi:
        raise ValueError(f"the chi rule is below Nyquist: kq[-1] max(dchi) = {kq[-1] * np.max(np.diff(chis)):.3g} > pi; "
                         "refine_gzs returns nodes that resolve a given kmax")
    return kq, chis


def _array(ctx, a, shape, what):
    """A host array (checked finite, of the given shape) uploaded, or a DeviceArray of that shape as it is."""
    if isinstance(a, nat.DeviceArray):
        if tuple(a.shape) != tuple(shape):
            raise ValueError(f"{what} must have shape {tuple(shape)}, got {tuple(a.shape)}")
        return a
    a = np.asarray(a, dtype=np.float64)
    if a.shape != tuple(shape) or not np.all(np.isfinite(a)):
        raise ValueError(f"{what} must be finite and of shape {tuple(shape)}, got {a.shape}")
    return ctx.upload(a)


# ---------------------------------------------------------------- plain arrays
def spherical_bessel_device(lmax, xs, *, ctx=None):
    """spherical_bessel with the result left on the device: a DeviceArray (lmax + 1, nx)."""
    lmax = check_lmax(lmax)
    xs = np.asarray(xs, dtype=np.float64).reshape(-1)
    if not np.all(np.isfinite(xs)) or np.any(xs < XMIN):
        raise ValueError(f"xs must be finite and at least {XMIN}")
    ctx = nat.context_or_default(ctx)
    out = ctx.empty((lmax + 1, xs.size))
    if xs.size:
        d_xs = ctx.upload(xs)
        ctx.call("hmg_sph_bessel", lmax, xs.size, d_xs.ptr, out.ptr)
    return out


def spherical_bessel(lmax, xs, *, ctx=None):
    """j_l(x) for l = 0 .. lmax at the arguments xs (finite, >= 1e-100), shape (lmax + 1, nx), in fp64: upward recurrence
    for x >= lmax, Miller's downward recurrence from a start order that depends on lmax alone otherwise (sphbessel.hpp).
    A value below the fp64 range is 0, never NaN.  A value depends on its x and on lmax."""
    out = spherical_bessel_device(lmax, xs, ctx=ctx)
    return out.numpy() if out.size else np.empty(out.shape)


def nonlimber_transfer_device(kq, chis, sources, lmax, *, ctx=None):
    """nonlimber_transfer with the result left on the device: a DeviceArray (F, lmax + 1, nkq).  sources may be a
    DeviceArray (F, ngz, nkq)."""
    lmax = check_lmax(lmax)
    kq, chis = check_rule(kq, chis)
    shape = tuple(sources.shape) if isinstance(sources, nat.DeviceArray) else np.shape(sources)
    if len(shape) != 3 or shape[0] < 1 or shape[1:] != (chis.size, kq.size):
        raise ValueError(f"sources must have shape (F, {chis.size}, {kq.size}) with F >= 1, got {shape}")
    ctx = nat.context_or_default(ctx)
    src = _array(ctx, sources, shape, "sources")
    F, ngz, nkq = shape
    out = ctx.empty((F, lmax + 1, nkq))
    d_kq, d_chis = ctx.upload(kq), ctx.upload(chis)
    for f0 in range(0, F, fmax()):                     # the walk at a point serves the fields of one launch
        n = min(fmax(), F - f0)
        ctx.call("hmg_nonlimber_transfer", n, ngz, nkq, lmax, d_kq.ptr, d_chis.ptr,
                 src.view(f0 * ngz * nkq, (n, ngz, nkq)).ptr, out.view(f0 * (lmax + 1) * nkq, (n, lmax + 1, nkq)).ptr)
    return out


def nonlimber_transfer(kq, chis, sources, lmax, *, ctx=None):
    """T[f, l, i] = sum_g sources[f, g, i] j_l(kq[i] chis[g]) for l = 0 .. lmax, shape (F, lmax + 1, nkq).

    kq (nkq,), chis (ngz,): finite, positive, strictly increasing, kq chi >= 1e-100 and kq[-1] max(diff(chis)) <= pi (a
    chi rule below Nyquist for the largest k is refused: see refine_gzs).  sources (F, ngz, nkq), finite: the sources
    times the weights of the chi rule.  fp64, the sum over g in a fixed order, bit-identical on repeat; an element depends
    on its field's column, its k node, chis and lmax alone (not on the other fields or k nodes - requests of more than 16
    fields are split into launches - but on lmax: the recurrence branches on x >= lmax).  Anything else raises
    ValueError before a launch."""
    return nonlimber_transfer_device(kq, chis, sources, lmax, ctx=ctx).numpy()


def check_pairs(pairs, F):
    out = []
    for p in pairs:
        if len(p) != 2 or any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= v < F for v in p):
            raise ValueError(f"pair {p!r} must be two field indices in 0 .. {F - 1}")
        out.append((int(p[0]), int(p[1])))
    if not out:
        raise ValueError("at least one pair is needed")
    return np.ascontiguousarray(out, dtype=np.int32)


def _cl_device(ctx, d_kq, d_wk, T, F, nkq, lmax, pr):
    out = ctx.empty((pr.shape[0], lmax + 1))
    chunk = 65535
    for p0 in range(0, pr.shape[0], chunk):
        part = np.ascontiguousarray(pr[p0:p0 + chunk])
        d_part = ctx.upload_int32(part)
        ctx.call("hmg_nonlimber_cl", F, nkq, lmax, part.shape[0], part.ctypes.data_as(C_.POINTER(C_.c_int)), d_part.ptr,
                 d_kq.ptr, d_wk.ptr, T.ptr, out.view(p0 * (lmax + 1), (part.shape[0], lmax + 1)).ptr)
    return out


def nonlimber_cl_device(kq, kweights, transfers, pairs, *, ctx=None):
    """nonlimber_cl with the result left on the device: a DeviceArray (npairs, lmax + 1).  transfers may be a
    DeviceArray (F, lmax + 1, nkq)."""
    kq = _increasing(kq, "kq")
    wk = np.asarray(kweights, dtype=np.float64)
    if wk.shape != kq.shape or not np.all(np.isfinite(wk)):
        raise ValueError(f"kweights must be finite and of shape {kq.shape}")
    shape = tuple(transfers.shape) if isinstance(transfers, nat.DeviceArray) else np.shape(transfers)
    if len(shape) != 3 or shape[0] < 1 or shape[1] < 1 or shape[2] != kq.size:
        raise ValueError(f"transfers must have shape (F, lmax + 1, {kq.size}), got {shape}")
    lmax = check_lmax(shape[1] - 1)
    pr = check_pairs(pairs, shape[0])
    ctx = nat.context_or_default(ctx)
    T = _array(ctx, transfers, shape, "transfers")
    return _cl_device(ctx, ctx.upload(kq), ctx.upload(wk), T, shape[0], kq.size, lmax, pr)


def nonlimber_cl(kq, kweights, transfers, pairs, *, ctx=None):
    """C[p, l] = (2/pi) sum_i kweights[i] kq[i]^2 T[a, l, i] T[b, l, i] for the pairs p = (a, b) of field indices,
    shape (npairs, lmax + 1) for transfers (F, lmax + 1, nkq).  A fixed order of summation: bit-identical on repeat, C[p]
    independent of the other pairs, (a, b) and (b, a) the same bits."""
    return nonlimber_cl_device(kq, kweights, transfers, pairs, ctx=ctx).numpy()


# ---------------------------------------------------------------- quadrature rules
def refine_gzs(model, zlo, zhi, kmax, phase=0.5):
    """Redshift nodes from zlo to zhi, uniform in comoving distance, with kmax dchi <= phase: the chi rule that resolves
    j_l(k chi) up to k = kmax (Nyquist is phase = pi; 0.5 leaves the trapezoid rule its accuracy).  model: anything with
    comoving_radial_distance and h_of_z (a HaloModel, a Cosmology); z from the existing cosmology.z_of_chi."""
    if not (np.isfinite(zlo) and np.isfinite(zhi) and 0 < zlo < zhi) or not kmax > 0 or not phase > 0:
        raise ValueError("refine_gzs needs 0 < zlo < zhi, kmax > 0 and phase > 0")
    lo, hi = (float(v) for v in np.reshape(model.comoving_radial_distance(np.array([zlo, zhi], dtype=np.float64)), -1))
    n = max(2, int(np.ceil((hi - lo) * kmax / phase)) + 1)
    zs = np.asarray(z_of_chi(model, np.linspace(lo, hi, n)), dtype=np.float64).reshape(-1)
    zs[0], zs[-1] = zlo, zhi
    return zs


def nonlimber_k_rule(lmax, chi_min, chi_max, depth, kmin=1e-4, per_period=8, nsigma=8.0, kmax=None):
    """The default k rule (kq, kweights): nodes linear in k from kmin to kmax with trapezoid weights.

    Spacing: T_l(k)^2 oscillates in k with period about pi / chi (the window sits at chi, not at 0), so the spacing is
    pi / (chi_max per_period) - per_period nodes per oscillation, set by the far edge of the windows; it does not depend
    on lmax.  Range: the integrand is cut off by the window's transform, not by j_l: beyond k = (lmax + 1/2) / chi_min
    the line-of-sight wavenumber sqrt(k^2 - ((l + 1/2)/chi)^2) grows and a window of depth `depth` (the r.m.s. width in
    chi of the narrowest feature) suppresses T_l like its transform, exp(-(k_par depth)^2 / 2) for a Gaussian, so
    kmax = sqrt(((lmax + 1/2) / chi_min)^2 + (nsigma / depth)^2) unless one is given.  Below kmin the integrand is
    k^2 P(k) times a bounded factor; kmin = 1e-4 / Mpc leaves out less than 1e-9 of C_0 of a 60 Mpc deep bin."""
    lmax = check_lmax(lmax)
    if not (0 < chi_min <= chi_max) or not depth > 0 or not kmin > 0 or per_period < 2 or not nsigma > 0:
        raise ValueError("nonlimber_k_rule needs 0 < chi_min <= chi_max, depth > 0, kmin > 0, per_period >= 2, nsigma > 0")
    if kmax is None:
        kmax = float(np.hypot((lmax + 0.5) / chi_min, nsigma / depth))
    if not kmax > kmin:
        raise ValueError(f"kmax = {kmax} must exceed kmin = {kmin}")
    n = int(np.ceil((kmax - kmin) * chi_max * per_period / np.pi)) + 1
    kq = np.linspace(kmin, kmax, max(n, 2))
    return kq, trapz_weights(kq)
