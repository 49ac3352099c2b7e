"""Numpy restatement of the CIB halo model from host arrays alone, and the 40-digit mpmath
reference of its integrand.

``luminosities`` follows csrc/kernels/cib.hpp operation by operation (the header of that file states the order); the
spectra follow hmg_emission_power's definitions with numpy sums.  Every spectrum is a pair (value, tol): tol bounds
|device - restatement| when both follow the contract, and is derived from rounding counts, never from a device result
(EPS = 2^-52):

* a luminosity: (nsub + C_DEVICE) EPS sum_g |w_g f_g| - each side adds nsub terms (half an EPS of the absolute sum per
  addition and side) and a term carries the integrand's error, at most C_DEVICE EPS |f_g|.  C_DEVICE is twice
  C_DEVICE_MEASURED, the device's worst error of one integrand value (w_g hw) N L / 4 pi against mpmath at 40 digits
  (tests/test_gpu_cib.py::test_integrand_constant_of_the_device measures it with one-node rules; the exact inputs are the
  fp64 numbers z, nu, chi, M, t_g, the parameters, x0 and the fp64 quotient M / M_min).  A central is one such value
  without N and without the sum: (1 + C_DEVICE) EPS |L_c|;
* a mass sum: (nm + TERM_ROUNDINGS) EPS A, A the same sum over absolute values.  Each side adds nm terms in some order
  (half an EPS of A per addition and side).  A term as hmg_emission_power forms it carries six roundings - t = L_s u,
  a = L_c + t, w = wm nzm, w t, and the two fma of the accumulate (the legs and the crosses: w bh or (w c) prof, a, one
  fma: five) - and as numpy forms it nine - w, t_f, t_g, three products, two sums, the product with w: fifteen, counted
  at a full EPS each, and one to spare;
* products and sums propagate with bispectrum_model.prod / add; P_lin at a node and the damping factor are exact (host and
  device hold the same bits); against get_power_1halo, whose kernel evaluates the damping with the device's exp,
  hod_ensemble_model.damping_tol times the undamped sum is added to twice the tol."""
import numpy as np

from hmvec_amd import bispectrum as bs
from hmvec_amd import cib
from hmvec_amd.quadrature import trapz_weights

import bispectrum_model as bm
from hod_ensemble_model import damping_tol  # noqa: F401

EPS = bm.EPS
TERM_ROUNDINGS = 16
C_DEVICE_MEASURED = 185.4   # MI355X: at the last node of the 64-node rule (t = 0.99965), 857 GHz, z = 1.2, the 69th mass
C_DEVICE = 2.0 * C_DEVICE_MEASURED
KH = 20.836619123327576      # k_B / h [GHz / K]
FOURPI, INV4PI = 4.0 * np.pi, 1.0 / (4.0 * np.pi)


# ---------------------------------------------------------------- luminosities, in the kernel's order
def sigma(M, p):
    norm = 1.0 / np.sqrt((2.0 * np.pi) * p["sigma2"])
    inv2s2 = 1.0 / (2.0 * p["sigma2"])
    d = np.log10(M) - p["log10_M_eff"]
    return (M * norm) * np.exp(-((d * d) * inv2s2))


def prefactor(nus, zs, p, x0):
    """A[f, z] = (L0 Phi) Theta, in the kernel's order."""
    nus = np.asarray(nus, dtype=float)
    zp1 = 1.0 + np.asarray(zs, dtype=float).reshape(-1)
    phi = np.minimum(zp1, 1.0 + p["z_p"]) ** p["delta"]
    Td = p["T0"] * zp1 ** p["alpha"]
    nu0 = (x0 * KH) * Td
    r = (zp1[None, :] * nus[:, None]) / nu0[None, :]
    with np.errstate(over="ignore"):
        low = r ** (3.0 + p["beta"]) * (np.expm1(x0) / np.expm1(x0 * r))
    theta = np.where(r < 1.0, low, r ** (-p["gamma"]))
    return (p["L0"] * phi[None, :]) * theta


def luminosities(zs, ms, chis, nus, p, x0, scut, t, w):
    """A dict: Lc, Ls (F, nz, nm); absum (F, nz, nm) = sum_g |term_g| of the kept nodes; central_margin, node_margin: the
    smallest |S / S_cut - 1| over the centrals and the nodes (inf without a cut); central_masked, node_masked: the masked
    shares of the centrals with M >= M_min and of the nodes of the rows with M > M_min."""
    zs, ms, chis = (np.asarray(a, dtype=float).reshape(-1) for a in (zs, ms, chis))
    nus = np.asarray(nus, dtype=float)
    A = prefactor(nus, zs, p, x0)                                          # (F, nz)
    zp1 = 1.0 + zs
    den = (FOURPI * zp1) * (chis * chis)                               # (nz,)
    Mmin = p["M_min"]
    # centrals
    L = A[:, :, None] * sigma(ms, p)[None, None, :]                        # (F, nz, nm)
    alive_c = (ms >= Mmin)[None, None, :]
    if scut is None:
        masked_c = np.zeros(L.shape, dtype=bool)
        cm = np.inf
    else:
        S = L / den[None, :, None]
        masked_c = S > scut[:, None, None]
        cm = float(np.min(np.abs(S / scut[:, None, None] - 1.0)[np.broadcast_to(alive_c, L.shape)]))
    Lc = np.where(alive_c & ~masked_c, L * INV4PI, 0.0)
    # satellites
    hw = np.log(ms / Mmin)                                                 # (nm,)
    x = hw[:, None] * t[None, :]                                           # (nm, nsub)
    msub = Mmin * np.exp(x)
    q = msub / ms[:, None]
    N = (0.3 * q ** (-0.7)) * np.exp(-(9.9 * q ** 2.5))
    sg = sigma(msub, p)
    wg = w[None, :] * hw[:, None]
    Ln = A[:, :, None, None] * sg[None, None]                              # (F, nz, nm, nsub)
    alive_s = (ms > Mmin)[None, None, :, None]
    if scut is None:
        masked_s = np.zeros(Ln.shape, dtype=bool)
        nm_ = np.inf
    else:
        S = Ln / den[None, :, None, None]
        masked_s = S > scut[:, None, None, None]
        nm_ = float(np.min(np.abs(S / scut[:, None, None, None] - 1.0)[np.broadcast_to(alive_s, Ln.shape)]))
    term = np.where(masked_s, 0.0, wg[None, None] * (N[None, None] * (Ln * INV4PI)))
    Ls = np.zeros(term.shape[:-1])
    for g in range(t.size):                                                # the nodes in order
        Ls = Ls + term[..., g]
    Ls = np.where(alive_s[..., 0], Ls, 0.0)
    absum = np.where(alive_s[..., 0], np.abs(term).sum(axis=-1), 0.0)
    n_c = np.broadcast_to(alive_c, L.shape)
    n_s = np.broadcast_to(alive_s, Ln.shape)
    return dict(Lc=Lc, Ls=Ls, absum=absum, central_margin=cm, node_margin=nm_,
                central_masked=float(masked_c[n_c].mean()), node_masked=float(masked_s[n_s].mean()))


def luminosity_tols(ref, nsub):
    """(tol of Lc, tol of Ls), each (F, nz, nm)."""
    return (1.0 + C_DEVICE) * EPS * np.abs(ref["Lc"]), (nsub + C_DEVICE) * EPS * ref["absum"]


# ---------------------------------------------------------------- the integrand at 40 digits
def exact_integrand(zs, ms, nus, p, x0, t):
    """f[f, z, m] = hw N(q) A Sigma(m_s) / 4 pi at the single node t of every row, in mpmath at 40 digits, rounded to
    fp64 at the end; rows with M <= M_min are nan.  The exact inputs are the fp64 numbers handed in and fl(M / M_min)."""
    import mpmath as mp
    mp.mp.dps = 40
    f_ = mp.mpf
    KH_, PI = f_(KH), mp.pi
    A = np.empty((len(nus), len(zs)), dtype=object)
    for j, z in enumerate(zs):
        zp1 = 1 + f_(float(z))
        phi = min(zp1, 1 + f_(p["z_p"])) ** f_(p["delta"])
        Td = f_(p["T0"]) * zp1 ** f_(p["alpha"])
        nu0 = f_(x0) * KH_ * Td
        for i, nu in enumerate(nus):
            r = zp1 * f_(float(nu)) / nu0
            theta = (r ** (3 + f_(p["beta"])) * mp.expm1(f_(x0)) / mp.expm1(f_(x0) * r)) if r < 1 else r ** (-f_(p["gamma"]))
            A[i, j] = f_(p["L0"]) * phi * theta
    s2, lMeff, Mmin = f_(p["sigma2"]), f_(p["log10_M_eff"]), f_(p["M_min"])
    base = np.empty(len(ms), dtype=object)
    for k, M in enumerate(ms):
        if not M > p["M_min"]:
            base[k] = None
            continue
        hw = mp.log(f_(float(M / p["M_min"])))
        msub = Mmin * mp.exp(hw * f_(float(t)))
        q = msub / f_(float(M))
        N = f_("0.3") * q ** f_("-0.7") * mp.exp(f_("-9.9") * q ** f_("2.5"))
        d = mp.log10(msub) - lMeff
        sg = msub / mp.sqrt(2 * PI * s2) * mp.exp(-d * d / (2 * s2))
        base[k] = hw * N * sg / (4 * PI)
    out = np.full((len(nus), len(zs), len(ms)), np.nan)
    for i in range(len(nus)):
        for j in range(len(zs)):
            for k in range(len(ms)):
                if base[k] is not None:
                    out[i, j, k] = float(A[i, j] * base[k])
    return out


def measure_c(got, exact):
    """The worst |got - exact| / (EPS |exact|) over the rows that exist, and where."""
    ok = np.isfinite(exact) & (exact != 0)
    err = np.zeros(exact.shape)
    err[ok] = np.abs(got[ok] - exact[ok]) / (EPS * np.abs(exact[ok]))
    at = np.unravel_index(int(np.argmax(err)), err.shape)
    return float(err[at]), tuple(int(i) for i in at)


# ---------------------------------------------------------------- spectra
def mass_sum(w, term, absterm=None):
    """sum over the mass axis (second to last) of w term and its tol (nm + TERM_ROUNDINGS) EPS A."""
    v = (w * term).sum(axis=-2)
    a = np.abs(w * (term if absterm is None else absterm)).sum(axis=-2)
    return v, (term.shape[-2] + TERM_ROUNDINGS) * EPS * a


def neg(x):
    return -x[0], x[1]


def spectra(nzm, bh, ms, ks, Pzk, rho_m0, us, Lc, Ls, kstar, partners=(), kindex=None, damping=True):
    """A dict of (value, tol) pairs: P1h (npair, nz, n), I (F, nz, n), X1h (NP, F, nz, n), the assembled planes 2h, total,
    cross_2h, cross_total, the undamped sums G (npair, nz, n) and X (NP, F, nz, n), and J (NP, nz, n), the partners'
    brackets.  partners: [(kind "m" | "p", tensor (nz, nm, nk)), ...]."""
    cols = np.arange(ks.size) if kindex is None else np.asarray(kindex)
    F = Lc.shape[0]
    w = (trapz_weights(ms)[None, :] * nzm)[:, :, None]                       # (nz, nm, 1)
    wb = w * bh[:, :, None]
    u = us[:, :, cols]
    t = Ls[..., None] * u[None]                                             # (F, nz, nm, n)
    lc = Lc[..., None]
    a = lc + t
    D = bs.damping(ks[cols], kstar) if damping else np.ones(cols.size)
    De, P = bm.exact(D[None, :]), bm.exact(Pzk[:, cols])
    G, I = [], []
    for f, g in cib.pair_list(F):
        term = lc[f] * t[g] + lc[g] * t[f] + t[f] * t[g]
        G.append(mass_sum(w, term, np.abs(lc[f] * t[g]) + np.abs(lc[g] * t[f]) + np.abs(t[f] * t[g])))
    for f in range(F):
        I.append(mass_sum(wb, a[f], np.abs(lc[f]) + np.abs(t[f])))
    one, two, tot = [], [], []
    for i, (f, g) in enumerate(cib.pair_list(F)):
        one.append(bm.prod(De, G[i]))
        two.append(bm.prod(P, I[f], I[g]))
        tot.append(bm.add(one[-1], two[-1]))
    out = dict(G=G, I=I, P1h=one)
    out["2h"], out["total"] = two, tot
    X, X1, J, x2, xt = [], [], [], [], []
    r = (ms / rho_m0)[None, :, None]
    for kind, prof in partners:
        pr = prof[:, :, cols]
        c = r if kind == "m" else np.ones((1, 1, 1))
        if kind == "m":
            Jp = bm.add(bm.mass_sum(wb[..., 0], r * pr), bm.exact(np.ones(())), neg(bm.mass_sum(wb[..., 0], r * np.ones_like(pr[..., :1]))))
        else:
            Jp = bm.mass_sum(wb[..., 0], pr)
        J.append(Jp)
        Xp = [mass_sum(w, (c * pr) * a[f], np.abs(c * pr) * (np.abs(lc[f]) + np.abs(t[f]))) for f in range(F)]
        X.append(Xp)
        X1.append([bm.prod(De, x) for x in Xp])
        x2.append([bm.prod(P, I[f], Jp) for f in range(F)])
        xt.append([bm.add(X1[-1][f], x2[-1][f]) for f in range(F)])
    out.update(X=X, X1h=X1, J=J, cross_2h=x2, cross_total=xt)
    return {k: _stack(v) for k, v in out.items()}


def _stack(pairs):
    """A (nested) list of (value, tol) pairs as one pair of arrays."""
    if isinstance(pairs, tuple):
        v, t = pairs
        return np.asarray(v), np.broadcast_to(t, np.shape(v)).copy()
    got = [_stack(p) for p in pairs]
    if not got:
        return np.zeros((0,)), np.zeros((0,))
    return np.stack([g[0] for g in got]), np.stack([g[1] for g in got])


def from_model(h, Lc, Ls, partners=(), satellite="nfw", kindex=None, damping=True):
    """spectra() on a HaloModel's own host arrays; partners are names of its matter or pressure profiles."""
    parts = [("m", np.asarray(h.uk_profiles[n])) if n in h.uk_profiles else ("p", np.asarray(h.pk_profiles[n])) for n in partners]
    return spectra(h.nzm, h.bh, h.ms, h.ks, h.Pzk, float(h.rho_matter_z(0)[0]), np.asarray(h.uk_profiles[satellite]), Lc, Ls,
                   h.p["kstar_damping"], partners=parts, kindex=kindex, damping=damping)
