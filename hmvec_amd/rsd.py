"""Redshift-space spectra of the dispersion halo model.

``HaloModel.rsd_device`` / ``get_power_rsd`` give the wedges P^s(k, mu) and ``multipoles_device`` /
``get_power_multipoles`` the multipoles P_0, P_2, P_4 of a pair of tracers, contracted on the GPU over the resident
tensors.  This module holds the host side of the contract - plain arithmetic on a few numbers that is uploaded, so that
host and device read the same bits: the default line-of-sight dispersion of a halo's members, the Gauss-Legendre rule in
mu of the two-halo multipoles and its Legendre weights - and the checks of a request, all of which refuse on the host
before anything is launched.
"""
import ctypes as C

import numpy as np

from . import _native as nat
from . import bispectrum as bispec
from .spectra import _same_lookups, check_term

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


class RsdMixin:
    """HaloModel's wedges and multipoles of one pair at nodes of the k grid (hmg_rsd_wedges, hmg_rsd_multipoles): a mass
    integral with a Gaussian of the bin's line-of-sight dispersion inside it."""

    def _rsd_request(self, name, name2, kindex, sigma_s, f, alphas, damping):
        """(records, uploaded tables, alphas) of a redshift-space request.  Every refusal happens here on the host,
        before any launch."""
        pair = (name, name if name2 is None else name2)
        recs = self._resolve(*pair)
        for r in recs:
            if r.kind1 == "p" or r.kind2 == "p":
                raise ValueError(f"redshift-space spectrum of {pair!r}: {r.name!r} is a pressure profile, which has no "
                                 f"line-of-sight velocity in this model")
        _same_lookups(recs, f"redshift-space spectrum of {pair!r}")
        nz, nm, nk = self._nz, self._nm, self._nk
        kindex = check_kindex(kindex, nk)
        sigma_s = check_sigma(virial_dispersion(self) if sigma_s is None else sigma_s, nz, nm)
        f = check_f(self.get_growth_rate_f(self.zs) if f is None else f, nz)
        alphas = check_alphas(alphas)
        damp = bispec.damping(self.ks[kindex], self.p["kstar_damping"]) if damping else np.ones(kindex.size)
        return recs, (kindex, np.ascontiguousarray(damp, dtype=np.float64), sigma_s, f), alphas

    def _rsd_launch(self, entry, recs, tables, alphas, mus, wl, out_last, parts_shape):
        nz, nm, nk, n, nmu = self._nz, self._nm, self._nk, tables[0].size, mus.size
        ctx = self._main(needs_aux=True)
        # (another reader of the tensors than the batched mass integrals: a deferred left fill is written first)
        ta, tb = (self._tracer(r, 1) for r in recs)
        d_k, d_damp, d_sig, d_f = ctx.upload_int32(tables[0]), ctx.upload(tables[1]), ctx.upload(tables[2]), ctx.upload(tables[3])
        d_mus = ctx.upload(mus)
        d_wl = None if wl is None else ctx.upload(np.ascontiguousarray(wl, dtype=np.float64))
        out = ctx.empty((2, nz, n, out_last))
        parts = ctx.empty(parts_shape(nz, n)) if parts_shape else None
        own = dict(d_parts=nat.ptr(parts)) if wl is None else dict(d_wl=d_wl.ptr, d_Q=nat.ptr(parts))
        ctx.call(entry, nz=nz, nm=nm, nk=nk, n=n, nmu=nmu, h_a=C.byref(ta), h_b=C.byref(tb), **self._model_block(entry),
                 d_kindex=d_k.ptr, d_damp=d_damp.ptr, d_mus=d_mus.ptr, d_sigma=d_sig.ptr, d_f=d_f.ptr, alpha_m=alphas[0],
                 alpha_c=alphas[1], alpha_s=alphas[2], d_out=out.ptr, **own)
        self._sync_point()
        return out, parts      # (the tables go back to the free list: whatever reads them was enqueued before)

    def rsd_device(self, name, name2=None, mus=None, kindex=None, sigma_s=None, f=None, alphas=(1, 0, 1), damping=True,
                   parts=False):
        """The redshift-space wedges of the pair (name, name2; default name) on the device, (2, nz, n, nmu) = (P1h, P2h),
        at the nodes ks[kindex] (default: all) and the values mus of mu in [0, 1] (default: rsd.mu_rule(16)'s nodes; at
        most 32).  Dispersion halo model: a halo's members of species i are displaced along the line of sight with the
        Gaussian dispersion alphas[i] sigma_s[z, m] - alphas = (alpha_m, alpha_c, alpha_s) for matter, centrals and
        satellites; sigma_s (nz, nm) in comoving Mpc, default rsd.virial_dispersion(self) - so every product of two species
        in a mass integral carries exp(-(alpha_i^2 + alpha_j^2) (k sigma_s mu)^2 / 2), and the 2-halo term is

            P2h = P_lin (J_a + f mu^2 K_a) (J_b + f mu^2 K_b),

        J the bracket of get_power_2halo with the damped weights, K the same bracket without the halo bias (the Kaiser
        term of the tracer's own velocity) and f (nz,) the growth rate, default get_growth_rate_f(zs).  The square term
        of P1h is get_power_1halo's, first-name-only rule for two HOD names included; damping=True multiplies P1h by
        1 - exp(-(k / kstar)^2) as get_power_1halo does.  A matter or an HOD name is taken, a pressure name refused.
        parts=True: (out, parts), parts (4, nz, n, nmu) = (I_a, V_a, I_b, V_b), the damped mass sums of the brackets."""
        mus = mu_rule(DEFAULT_NMU)[0] if mus is None else mus
        mus = check_mus(mus)
        recs, tables, alphas = self._rsd_request(name, name2, kindex, sigma_s, f, alphas, damping)
        out, P = self._rsd_launch("hmg_rsd_wedges", recs, tables, alphas, mus, None, mus.size,
                                  (lambda nz, n: (4, nz, n, mus.size)) if parts else None)
        return (out, P) if parts else out

    def get_power_rsd(self, name, name2=None, mus=None, kindex=None, sigma_s=None, f=None, alphas=(1, 0, 1), damping=True):
        """{"1h", "2h", "total"}: the redshift-space wedges P^s(z, k, mu) of the pair on the host, each (nz, n, nmu); see
        rsd_device."""
        out = self.rsd_device(name, name2, mus=mus, kindex=kindex, sigma_s=sigma_s, f=f, alphas=alphas,
                              damping=damping).numpy()
        return {"1h": out[0], "2h": out[1], "total": out[0] + out[1]}

    def multipoles_device(self, name, name2=None, nmu=16, kindex=None, sigma_s=None, f=None, alphas=(1, 0, 1), damping=True,
                          parts=False):
        """The multipoles P_l = (2l + 1) int_0^1 L_l(mu) P^s dmu, l = 0, 2, 4, of rsd_device's wedges on the device,
        (2, nz, n, 3) = (1-halo, 2-halo).  The 1-halo multipoles are exact in mu (the moments of the Gaussians in closed
        form inside the mass integral); the 2-halo ones are defined as the nmu-node Gauss-Legendre rule on [0, 1]
        (rsd.mu_rule, rsd.legendre_weights; 1 <= nmu <= 32) of the 2-halo wedge.  parts=True: (out, Q), Q (3, nz, n) the
        moment sums Q_0, Q_1, Q_2 of the 1-halo term (undamped by get_power_1halo's factor)."""
        mus, _ = mu_rule(nmu)
        wl = legendre_weights(nmu)
        recs, tables, alphas = self._rsd_request(name, name2, kindex, sigma_s, f, alphas, damping)
        out, Q = self._rsd_launch("hmg_rsd_multipoles", recs, tables, alphas, np.ascontiguousarray(mus), wl, 3,
                                  (lambda nz, n: (3, nz, n)) if parts else None)
        return (out, Q) if parts else out

    def get_power_multipoles(self, name, name2=None, ells=(0, 2, 4), term="total", nmu=16, kindex=None, sigma_s=None,
                             f=None, alphas=(1, 0, 1), damping=True):
        """The multipoles ells (of 0, 2, 4) of the redshift-space spectrum of the pair at the nodes ks[kindex], shape
        (len(ells), nz, n); term: "1h", "2h" or "total".  See multipoles_device."""
        ells = check_ells(ells)
        check_term(term, TERMS)
        out = self.multipoles_device(name, name2, nmu=nmu, kindex=kindex, sigma_s=sigma_s, f=f, alphas=alphas,
                                     damping=damping).numpy()
        picked = pick_term(out, term)
        return np.stack([picked[..., ELLS.index(e)] for e in ells])
