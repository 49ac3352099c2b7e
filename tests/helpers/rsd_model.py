"""Numpy restatement of the redshift-space spectra of the dispersion halo model from a HaloModel's
host arrays alone: uk_profiles / hods entries, nzm, bh, ms, ks, Pzk.  The kinds of the names and the parts of an HOD are
trispectrum_model's, the k -> 0 sums C and b of a leg and the (value, tol) arithmetic are bispectrum_model's; what a
comparison with this tests is the new mass sums with a Gaussian inside, the moments, the epilogues and the rule in mu.

    species of a leg: (p, h) = (m/rho_m0 u, alpha_m^2/2) | (Nc/ngal (u_c or 1), alpha_c^2/2), (Ns/ngal u_s, alpha_s^2/2)
    w^s(mu) = sum_species p exp(-h x^2 mu^2),  x = k sigma_s[z,m]
    P1h = damp sum_m wm nzm S^s;  I^s = sum_m wm nzm bh w^s,  V^s = sum_m wm nzm w^s
    P2h = P_lin (J_a + f mu^2 K_a) (J_b + f mu^2 K_b),  J = (I^s + b) - C,  K = (V^s + 1) - C0
    Q_n = sum_m wm nzm sum_terms v M_n(t);  P_0 = Q_0, P_2 = 5/2 (3 Q_1 - Q_0), P_4 = 9/8 ((35 Q_2 - 30 Q_1) + 3 Q_0)

Every quantity is a pair (value, tol).  tol bounds |device - restatement| when both follow the contract; it is derived
from rounding counts and the measured error of the special functions, not from the device's results (EPS = 2^-52):

* a Gaussian exp(-A), A = h x^2 mu^2: relative (EXP_ERR + ARG_ROUNDINGS A) EPS - the error of exp itself, and the five
  roundings of its argument (x, x^2, alpha^2, h x^2, mu^2 ... each moves exp(-A) by A EPS);
* a species term p exp(-A): three more roundings (the coefficient, the tensor value, the product);
* a moment M_n(t): MOMENT_ERR EPS M_0 for the evaluation, and T_ROUNDINGS roundings of t, each of which moves M_n by at
  most t M_{n+1} EPS <= 5/2 M_0 EPS (t M_{n+1} = ((2n + 1) M_n - exp(-t)) / 2);
* a mass sum of terms with tols: sum_m |w| tol_term + (nm + 3) EPS sum_m |w term| (nm accumulations in some order on
  each side, the weight wm nzm (bh) and the fma);
* products and sums propagate (bispectrum_model.prod / add);
* P_lin at a node, f mu^2, the factor of the 1-halo term and the weights of the rule are exact: host and device hold or
  form the same bits.

EXP_ERR and MOMENT_ERR are twice the worst case tests/test_rsd_cpu.py measures on the host against 40-digit arithmetic
(the factor two is for the device's libm); that test fails if a measurement exceeds half of the constant."""
import numpy as np
from scipy.special import erf

from hmvec_amd import bispectrum as bs
from hmvec_amd import rsd
from hmvec_amd.quadrature import trapz_weights

import bispectrum_model as bm
import trispectrum_model as tm

EPS = tm.EPS
EXP_ERR = 2.0                 # exp, relative: measured 0.52 on the host, rounded up to one
MOMENT_ERR = 6.0              # M_n, in EPS M_0: measured 2.9 (this restatement) and 0.97 (the header's host build)
ARG_ROUNDINGS = 5
T_ROUNDINGS = 5
SERIES_BELOW = 2.0            # this restatement's own switch and series length (the header's are 1 and 20)
SERIES_TERMS = 32


def gauss_moments(t):
    """M_n(t) = int_0^1 mu^2n exp(-t mu^2) dmu, n = 0, 1, 2, stacked on a new first axis."""
    t = np.asarray(t, dtype=float)
    small = t < SERIES_BELOW
    ts = np.where(small, t, 0.0)
    out = np.empty((3,) + t.shape)
    for n in range(3):
        term, acc = np.ones_like(ts), np.full_like(ts, 1.0 / (2 * n + 1))
        for j in range(1, SERIES_TERMS):
            term = term * (-ts) / j
            acc = acc + term / (2 * n + 2 * j + 1)
        out[n] = acc
    tl = np.where(small, 1.0, t)
    e = np.exp(-tl)
    m0 = np.sqrt(np.pi / (4.0 * tl)) * erf(np.sqrt(tl))
    m1 = (m0 - e) / (2.0 * tl)
    m2 = (3.0 * m1 - e) / (2.0 * tl)
    for n, m in enumerate((m0, m1, m2)):
        out[n] = np.where(small, out[n], m)
    return out


def neg(x):
    return -x[0], x[1]


def mass_sum_t(w, term):
    """sum over axis 1 of w[z,m] term[z,m,...] for term = (value, tol): (value, tol)."""
    val, tol = term
    wb = w.reshape(w.shape + (1,) * (val.ndim - 2))
    return (wb * val).sum(axis=1), (np.abs(wb) * tol).sum(axis=1) + (w.shape[1] + 3) * EPS * np.abs(wb * val).sum(axis=1)


def species(h, name, alphas):
    """The species of a leg: a list of (coef (nz, nm), u (nz, nm, nk) or None for 1, h = alpha^2 / 2)."""
    am, ac, as_ = (float(a) for a in alphas)
    kind = tm._kind(h, name)
    if kind == "p":
        raise ValueError(f"{name!r} is a pressure profile")
    if kind == "m":
        rho = float(h.rho_matter_z(0)[0])
        return [(np.broadcast_to(h.ms[None, :] / rho, h.nzm.shape), h.uk_profiles[name], 0.5 * (am * am))]
    hod, uc, us = tm._hod_parts(h, name)
    ng = hod["ngal"][:, None]
    return [(hod["Nc"] / ng, None if np.isscalar(uc) else uc, 0.5 * (ac * ac)), (hod["Ns"] / ng, us, 0.5 * (as_ * as_))]


def _at(u, kindex):
    return 1.0 if u is None else u[:, :, kindex]


def _x2(h, kindex, sigma_s):
    x = h.ks[kindex][None, None, :] * sigma_s[:, :, None]
    return x * x


def damped_species(spec, x2, kindex, mu2):
    """(value, tol) [z, m, s, q] of one species' term p exp(-h x^2 mu^2)."""
    coef, u, hh = spec
    p = (coef[:, :, None] * _at(u, kindex))[..., None]
    if hh == 0.0:
        val = p * np.ones(x2.shape + mu2.shape)
        return val, 3 * EPS * np.abs(val)
    arg = (hh * x2)[..., None] * mu2
    val = p * np.exp(-arg)
    return val, np.abs(val) * EPS * (3 + EXP_ERR + ARG_ROUNDINGS * arg)


def tables(h, kindex, sigma_s, f, damping):
    nz, nm = h.nzm.shape
    kindex = np.arange(h.ks.size) if kindex is None else np.asarray(kindex)
    sigma_s = np.asarray(sigma_s, dtype=float)
    f = np.asarray(f, dtype=float)
    assert sigma_s.shape == (nz, nm) and f.shape == (nz,)
    damp = bs.damping(h.ks[kindex], h.p["kstar_damping"]) if damping else np.ones(kindex.size)
    return kindex, sigma_s, f, damp


def leg_constants(h, name, kindex):
    """(C, C0, b), each (value, tol) of shape (nz,): the k -> 0 sums of the leg and its bias term."""
    nz, nm = h.nzm.shape
    idx = np.broadcast_to(kindex[None, :], (nz, kindex.size))
    _, _, C, b, _ = bm.leg_terms(h, name, idx, np.zeros(idx.shape))
    wn = trapz_weights(h.ms)[None, :] * h.nzm
    if tm._kind(h, name) == "m":
        low = np.broadcast_to(h.ms[None, :] / float(h.rho_matter_z(0)[0]), (nz, nm))
    else:
        hod = h.hods[name]
        low = (hod["Nc"] + hod["Ns"]) / hod["ngal"][:, None]
    return C, bm.mass_sum(wn, low), b


def wedges(h, a, b=None, mus=None, kindex=None, sigma_s=None, f=None, alphas=(1, 0, 1), damping=True):
    """A dict of (value, tol) pairs: P1h, P2h, Ia, Va, Ib, Vb (nz, n, nmu), and the exact damp (n,)."""
    b = a if b is None else b
    mus = np.asarray(mus, dtype=float)
    kindex, sigma_s, f, damp = tables(h, kindex, sigma_s, f, damping)
    mu2 = mus * mus
    x2 = _x2(h, kindex, sigma_s)
    wn = trapz_weights(h.ms)[None, :] * h.nzm
    wnb = wn * h.bh
    out = {}
    w = {}
    for name in dict.fromkeys((a, b)):
        sp = [damped_species(s, x2, kindex, mu2) for s in species(h, name, alphas)]
        w[name] = sp[0] if len(sp) == 1 else bm.add(*sp)
    if tm._kind(h, a) == "h" and tm._kind(h, b) == "h":
        S = _square_hh(h, a, alphas, x2, kindex, mu2)
    else:
        S = bm.prod(w[a], w[b])
    P1 = mass_sum_t(wn, S)
    out["P1h"] = bm.prod(bm.exact(damp[None, :, None]), P1)
    bra = {}
    for name in w:
        I, V = mass_sum_t(wnb, w[name]), mass_sum_t(wn, w[name])
        C, C0, bias = ((v[0][:, None, None], v[1][:, None, None]) for v in leg_constants(h, name, kindex))
        J = bm.add(I, bias, neg(C))
        K = bm.add(V, bm.exact(np.ones(())), neg(C0))
        fm = bm.exact(f[:, None, None] * mu2[None, None, :])
        bra[name] = (I, V, bm.add(J, bm.prod(fm, K)))
    P = bm.exact(h.Pzk[:, kindex][:, :, None])
    out["P2h"] = bm.prod(P, bra[a][2], bra[b][2])
    out["Ia"], out["Va"], out["Ib"], out["Vb"] = bra[a][0], bra[a][1], bra[b][0], bra[b][1]
    out["damp"] = damp
    return out


def _square_hh(h, a, alphas, x2, kindex, mu2):
    """Two HOD names: the first name's 2<NcNs>/ngal^2 u_c u_s E_c E_s + <Ns(Ns-1)>/ngal^2 u_s^2 E_s^2, (value, tol)."""
    hod, uc, us = tm._hod_parts(h, a)
    _, ac, as_ = (float(v) for v in alphas)
    hc, hs = 0.5 * (ac * ac), 0.5 * (as_ * as_)
    ng2 = hod["ngal"][:, None, None] ** 2.0
    ucs = 1.0 if np.isscalar(uc) else uc[:, :, kindex]
    uss = us[:, :, kindex]
    ac_arg, as_arg = (hc * x2)[..., None] * mu2, (hs * x2)[..., None] * mu2
    t0 = (2.0 * hod["NcNs"][..., None] / ng2 * ucs * uss)[..., None] * np.exp(-(ac_arg + as_arg))
    t1 = (hod["NsNsm1"][..., None] / ng2 * uss * uss)[..., None] * np.exp(-2.0 * as_arg)
    tol0 = np.abs(t0) * EPS * (8 + 2 * EXP_ERR + ARG_ROUNDINGS * (ac_arg + as_arg))
    tol1 = np.abs(t1) * EPS * (8 + 2 * EXP_ERR + ARG_ROUNDINGS * 2.0 * as_arg)
    return bm.add((t0, tol0), (t1, tol1))


def moment_terms(h, a, b, alphas, x2, kindex):
    """The products of two species of the 1-halo term: a list of (v (nz, nm, n), t (nz, nm, n))."""
    if tm._kind(h, a) == "h" and tm._kind(h, b) == "h":
        hod, uc, us = tm._hod_parts(h, a)
        _, ac, as_ = (float(v) for v in alphas)
        hc, hs = 0.5 * (ac * ac), 0.5 * (as_ * as_)
        ng2 = hod["ngal"][:, None, None] ** 2.0
        ucs = 1.0 if np.isscalar(uc) else uc[:, :, kindex]
        uss = us[:, :, kindex]
        return [(2.0 * hod["NcNs"][..., None] / ng2 * ucs * uss, (hc + hs) * x2),
                (hod["NsNsm1"][..., None] / ng2 * uss * uss, (hs + hs) * x2)]
    out = []
    for ca, ua, ha in species(h, a, alphas):
        for cb, ub, hb in species(h, b, alphas):
            out.append(((ca[:, :, None] * _at(ua, kindex)) * (cb[:, :, None] * _at(ub, kindex)), (ha + hb) * x2))
    return out


def multipoles(h, a, b=None, nmu=16, kindex=None, sigma_s=None, f=None, alphas=(1, 0, 1), damping=True):
    """A dict of (value, tol) pairs: Q (3, nz, n), P1h and P2h (nz, n, 3), the 2-halo wedge W2h (nz, n, nmu) at the
    rule's nodes, and Q0abs (nz, n), the scale of the tols of the 1-halo term."""
    b = a if b is None else b
    mus, _ = rsd.mu_rule(nmu)
    wl = rsd.legendre_weights(nmu)
    kidx, sig, ff, damp = tables(h, kindex, sigma_s, f, damping)
    x2 = _x2(h, kidx, sig)
    wn = (trapz_weights(h.ms)[None, :] * h.nzm)[:, :, None]
    nm = h.nzm.shape[1]
    Q = np.zeros((3,) + x2.shape[::2])
    Q0abs = np.zeros(x2.shape[::2])
    for v, t in moment_terms(h, a, b, alphas, x2, kidx):
        M = gauss_moments(t)
        Q += (wn * v * M).sum(axis=2)
        Q0abs += np.abs(wn * v * M[0]).sum(axis=1)
    c = 3 + 8 + MOMENT_ERR + 2.5 * T_ROUNDINGS
    Qtol = np.broadcast_to((nm + c) * EPS * Q0abs, Q.shape)
    Qs = [(Q[n], Qtol[n]) for n in range(3)]
    const = lambda v: bm.exact(np.full((), v))  # noqa: E731
    P0 = Qs[0]
    P2 = bm.prod(const(2.5), bm.add(bm.prod(const(3.0), Qs[1]), neg(Qs[0])))
    P4 = bm.prod(const(1.125), bm.add(bm.add(bm.prod(const(35.0), Qs[2]), neg(bm.prod(const(30.0), Qs[1]))),
                                      bm.prod(const(3.0), Qs[0])))
    d = bm.exact(damp[None, :])
    P1h = [bm.prod(d, p) for p in (P0, P2, P4)]
    W = wedges(h, a, b, mus=mus, kindex=kindex, sigma_s=sigma_s, f=f, alphas=alphas, damping=damping)["P2h"]
    P2h = rule(W, wl)
    return dict(Q=(Q, Qtol), P1h=tuple(np.stack([p[j] for p in P1h], axis=-1) for j in (0, 1)), P2h=P2h, W2h=W,
                Q0abs=Q0abs, damp=damp)


def rule(W, wl):
    """(value, tol) (..., 3) of sum_q wl[l, q] W[..., q] for W = (value, tol)."""
    val = np.einsum("lq,...q->...l", wl, W[0])
    absum = np.einsum("lq,...q->...l", np.abs(wl), np.abs(W[0]))
    tol = np.einsum("lq,...q->...l", np.abs(wl), np.broadcast_to(W[1], W[0].shape)) + (wl.shape[1] + 1) * EPS * absum
    return val, tol
