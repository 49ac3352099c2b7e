"""Redshift-space spectra of the dispersion halo model.

``HaloModel.rsd_device`` / ``get_power_rsd`` give the wedges P^s(k, mu) and ``multipoles_device`` /
``get_power_multipoles`` the multipoles P_0, P_2, P_4 of a pair of tracers, contracted on the GPU over the resident
tensors.  This module holds the host side of the contract - plain arithmetic on a few numbers that is uploaded, so that
host and device read the same bits: the default line-of-sight dispersion of a halo's members, the Gauss-Legendre rule in
mu of the two-halo multipoles and its Legendre weights - and the checks of a request, all of which refuse on the host
before anything is launched.
"""
import numpy as np

__all__ = ["virial_dispersion", "mu_rule", "legendre_weights"]

G_NEWTON = 4.30091e-9         # Mpc (km/s)^2 / M_sun
ELLS = (0, 2, 4)
MAX_MU = 32
DEFAULT_NMU = 16
TERMS = ("1h", "2h", "total")


def virial_dispersion(model, scale=1.0):
    """sigma_s[z, m] = scale sqrt(G m / (2 r_vir)) (1 + z) / H(z), shape (nz, nm): the one-dimensional velocity
    dispersion of an isothermal halo of the model's mass definition as a comoving line-of-sight displacement in Mpc.
    r_vir = model.rvir(m, z) is a physical length (its density argument is the physical density at z) and H is in
    km/s/Mpc."""
    zs = np.asarray(model.zs, dtype=np.float64).reshape(-1)
    ms = np.asarray(model.ms, dtype=np.float64).reshape(-1)
    rvir = np.asarray(model.rvir(ms[None, :], zs[:, None]), dtype=np.float64)
    hz = np.asarray(model.hubble_parameter(zs), dtype=np.float64).reshape(-1)
    return float(scale) * np.sqrt(G_NEWTON * ms[None, :] / (2.0 * rvir)) * ((1.0 + zs) / hz)[:, None]


def _check_nmu(nmu):
    if not isinstance(nmu, (int, np.integer)) or isinstance(nmu, bool) or not 1 <= nmu <= MAX_MU:
        raise ValueError(f"nmu must be an integer in 1 .. {MAX_MU}, got {nmu!r}")
    return int(nmu)


def mu_rule(nmu=DEFAULT_NMU):
    """(mu, w): the nmu-node Gauss-Legendre rule on [0, 1] - numpy.polynomial.legendre.leggauss mapped from [-1, 1] -
    nodes ascending, 1 <= nmu <= 32."""
    x, w = np.polynomial.legendre.leggauss(_check_nmu(nmu))
    return 0.5 * (x + 1.0), 0.5 * w


def legendre(ell, mu):
    """L_0, L_2 or L_4 at mu."""
    mu = np.asarray(mu, dtype=np.float64)
    m2 = mu * mu
    if ell == 0:
        return np.ones_like(mu)
    if ell == 2:
        return 0.5 * (3.0 * m2 - 1.0)
    if ell == 4:
        return 0.125 * ((35.0 * m2 - 30.0) * m2 + 3.0)
    raise ValueError(f"ell must be one of {ELLS}, got {ell!r}")


def legendre_weights(nmu=DEFAULT_NMU):
    """(3, nmu): (2 l + 1) w_q L_l(mu_q), l = 0, 2, 4, over mu_rule(nmu): the weights with which the rule turns a wedge
    into its multipoles, P_l = sum_q weights[l/2, q] P(mu_q)."""
    mu, w = mu_rule(nmu)
    return np.stack([(2 * ell + 1) * w * legendre(ell, mu) for ell in ELLS])


# ---------------------------------------------------------------- the checks of a request
def check_mus(mus):
    mus = np.ascontiguousarray(np.atleast_1d(np.asarray(mus, dtype=np.float64)))
    if mus.ndim != 1 or mus.size < 1:
        raise ValueError("mus is empty: the wedges need at least one value of mu (a one-dimensional array)")
    if mus.size > MAX_MU:
        raise ValueError(f"{mus.size} values of mu; at most {MAX_MU} are taken in one call")
    if not np.all((mus >= 0.0) & (mus <= 1.0)):
        raise ValueError("mus must lie in [0, 1]")
    return mus


def check_kindex(kindex, nk):
    kindex = np.arange(nk) if kindex is None else np.asarray(kindex)
    if kindex.ndim != 1 or not np.issubdtype(kindex.dtype, np.integer):
        raise ValueError("kindex must be a one-dimensional integer array of indices into ks")
    if kindex.size < 1:
        raise ValueError("kindex is empty: at least one node is needed")
    if kindex.size > nk:
        raise ValueError(f"kindex names {kindex.size} samples; at most nk = {nk} are taken")
    if kindex.min() < 0 or kindex.max() > nk - 1:
        raise ValueError(f"kindex must lie in 0 .. nk - 1 = {nk - 1}, got {kindex.min()} .. {kindex.max()}")
    return np.ascontiguousarray(kindex, dtype=np.int32)


def check_sigma(sigma_s, nz, nm):
    sigma_s = np.ascontiguousarray(sigma_s, dtype=np.float64)
    if sigma_s.shape != (nz, nm):
        raise ValueError(f"sigma_s must have shape (nz, nm) = {(nz, nm)}, got {sigma_s.shape}")
    if not np.all(np.isfinite(sigma_s)) or np.any(sigma_s < 0.0):
        raise ValueError("sigma_s must be finite and >= 0")
    return sigma_s


def check_f(f, nz):
    f = np.ascontiguousarray(f, dtype=np.float64)
    if f.shape != (nz,) or not np.all(np.isfinite(f)):
        raise ValueError(f"f must be finite with one entry per redshift, shape ({nz},), got shape {f.shape}")
    return f


def check_alphas(alphas):
    a = np.asarray(alphas, dtype=np.float64)
    if a.shape != (3,) or not np.all(np.isfinite(a)):
        raise ValueError(f"alphas must be three finite numbers (alpha_m, alpha_c, alpha_s), got {alphas!r}")
    return tuple(float(v) for v in a)


def check_ells(ells):
    ells = tuple(int(e) if float(e) == int(e) else e for e in np.atleast_1d(ells).tolist())
    for e in ells:
        if e not in ELLS:
            raise ValueError(f"ell must be one of {ELLS}, got {e!r}")
    return ells


def pick_term(out, term):
    """A term of out (2, ...) = (1h, 2h); "total" is their sum."""
    if term not in TERMS:
        raise ValueError(f"term must be one of {TERMS}, got {term!r}")
    return out[0] + out[1] if term == "total" else out[TERMS.index(term)]
