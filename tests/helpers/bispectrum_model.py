"""Numpy restatement of the halo-model bispectrum of three tracers from a HaloModel's host arrays
alone: uk_profiles / pk_profiles / hods entries, nzm, bh, ms, ks, Pzk.  The tensors it reads are produced by code the
bispectrum does not touch and that is gated against the reference elsewhere; what a comparison with this tests is the
device contraction, its loader, the prepass and the assembly of the three terms.

Every quantity is a pair (value, tol).  tol bounds |device - restatement| when both follow the contract; it is derived
from rounding counts, not measured (EPS = 2^-52):

* mass sums (the 1-halo sum, I_xy, I_x, C_x, the HOD bias sum): (nm + 40) EPS A, A the same sum over absolute values.
  Each side adds nm terms in some order, and a term carries at most about thirty roundings - per leg a form of <= 5 fma
  and a 3-rounding interpolation, then two products, the weight wm nzm (bh) and the accumulate;
* P_s: 3 EPS |P|;  J = (I + b) - C: the three sums' tols plus 2 EPS (|I| + |b| + |C|);
* mu: 4 EPS (|(r - p)(r + p)| + q^2) / (2 p q);  F2: dmu/2 (p/q + q/p) + 4/7 |mu| dmu + 6 EPS F2abs,
  F2abs = 5/7 + |mu|/2 (p/q + q/p) + 2/7 mu^2 - with (p, q) in the order F2 is evaluated in, p >= q;
* a product: sum_i tol_i prod_{j != i} |x_j| plus one EPS of prod |x_j| per multiplication; a sum: the sum of the tols
  plus one EPS of the absolute sum per addition;
* the sample wavenumbers, the damping factors (hmvec_amd.bispectrum.damping) and the scales are exact: host and device
  form the same bits."""
import numpy as np

from hmvec_amd import bispectrum as bs
from hmvec_amd.quadrature import trapz_weights

import trispectrum_model as tm

EPS = tm.EPS
MASS_ROUNDINGS = 40


def exact(x):
    x = np.asarray(x, dtype=float)
    return x, np.zeros_like(x)


def prod(*xs):
    """(value, tol) of a product of (value, tol) factors."""
    val = np.ones(())
    for v, _ in xs:
        val = val * v
    tol = np.zeros(())
    for i, (_, t) in enumerate(xs):
        rest = np.ones(())
        for j, (v, _) in enumerate(xs):
            if j != i:
                rest = rest * np.abs(v)
        tol = tol + t * rest
    return val, tol + (len(xs) - 1) * EPS * np.abs(val)


def add(*xs):
    """(value, tol) of a sum of (value, tol) terms."""
    val, tol, absum = np.zeros(()), np.zeros(()), np.zeros(())
    for v, t in xs:
        val, tol, absum = val + v, tol + t, absum + np.abs(v)
    return val, tol + (len(xs) - 1) * EPS * absum


def mass_sum(w, *factors):
    """sum_m w[z,m] prod factors[z,m,...] over axis 1 and its tol (nm + 40) EPS A."""
    term = w.reshape(w.shape + (1,) * (factors[0].ndim - 2))
    for f in factors:
        term = term * f
    return term.sum(axis=1), (w.shape[1] + MASS_ROUNDINGS) * EPS * np.abs(term).sum(axis=1)


def kind(h, name):
    return tm._kind(h, name)


def leg_terms(h, name, idx, frac):
    """Of one leg at the (nz, n) samples: w[z,m,s] and the (value, tol) pairs I[z,s], C[z], b[z], J[z,s]."""
    nz, nm = h.nzm.shape
    one = np.ones(idx.shape)
    w = tm.sampled(np.broadcast_to(tm._weight(h, name), (nz, nm, h.ks.size)), idx, frac, one)
    wnb = trapz_weights(h.ms)[None, :] * h.nzm * h.bh
    I = mass_sum(wnb, w)
    k = kind(h, name)
    if k == "m":
        C = mass_sum(wnb, np.broadcast_to(h.ms[None, :] / float(h.rho_matter_z(0)[0]), (nz, nm)))
        b = exact(np.ones(nz))
    elif k == "p":
        C, b = exact(np.zeros(nz)), exact(np.zeros(nz))
    else:
        hod = h.hods[name]
        low = (hod["Nc"] + hod["Ns"]) / hod["ngal"][:, None]
        C = mass_sum(wnb, low)
        b = mass_sum(wnb, low)
    Jv = (I[0] + b[0][:, None]) - C[0][:, None]
    Jt = I[1] + (b[1] + C[1])[:, None] + 2 * EPS * (np.abs(I[0]) + (np.abs(b[0]) + np.abs(C[0]))[:, None])
    return w, I, C, b, (Jv, Jt)


def F2_tol(p, q, r):
    """(F2, tol) of hmvec_amd.bispectrum.F2 with the bound of the module docstring, at the order of (p, q) F2 is
    evaluated in: the longer of the two first."""
    p, q = np.maximum(p, q), np.minimum(p, q)
    num = (r - p) * (r + p)
    mu = np.clip((num - q * q) / (2.0 * p * q), -1.0, 1.0)
    dmu = 4 * EPS * (np.abs(num) + q * q) / (2.0 * p * q)
    s = p / q + q / p
    f2abs = 5.0 / 7.0 + 0.5 * np.abs(mu) * s + (2.0 / 7.0) * mu * mu
    return bs.F2(p, q, r), 0.5 * dmu * s + (4.0 / 7.0) * np.abs(mu) * dmu + 6 * EPS * f2abs


def tree_tol(k1, k2, k3, P1, P2, P3):
    """(B_tree, tol); P_i are (value, tol) pairs."""
    v, t = add(prod(F2_tol(k1, k2, k3), P1, P2), prod(F2_tol(k2, k3, k1), P2, P3), prod(F2_tol(k3, k1, k2), P3, P1))
    return 2.0 * v, 2.0 * t


def bispectrum(h, names, tri, kindex=None, idx=None, frac=None, scale=None, damping=True):
    """The three terms of the triple `names` at the triangles tri (nt, 3) of the samples: a dict of (value, tol) pairs
    B1h, B2h, B3h (nz, nt), J (3, nz, n), I (3, nz, n), C and b (3, nz), P (nz, n), and the exact k and D (nz, n)."""
    a, b, c = names
    idx, frac, scale = tm.tables(h, kindex=kindex, idx=idx, frac=frac, scale=scale, damping=False)
    tri = np.asarray(tri)
    nz, nm = h.nzm.shape
    z = np.arange(nz)[:, None]
    ksamp = bs.sample_wavenumbers(h.ks, idx, frac)
    D = bs.damping(ksamp, h.p["kstar_damping"]) if damping else np.ones_like(ksamp)
    Pl, Pr = h.Pzk[z, idx], h.Pzk[z, np.minimum(idx + 1, h.ks.size - 1)]
    Pv = np.where(frac == 0.0, Pl, (1.0 - frac) * Pl + frac * np.where(frac == 0.0, 0.0, Pr))
    P = (Pv, 3 * EPS * np.abs(Pv))
    legs = {nm_: leg_terms(h, nm_, idx, frac) for nm_ in dict.fromkeys(names)}
    wn = trapz_weights(h.ms)[None, :] * h.nzm
    wnb = wn * h.bh
    s1, s2, s3 = tri[:, 0], tri[:, 1], tri[:, 2]

    def at(x, s):          # a (value, tol) pair of shape (nz, n) at the samples s of the triangles
        return x[0][:, s], x[1][:, s]

    wa, wb, wc = legs[a][0][:, :, s1], legs[b][0][:, :, s2], legs[c][0][:, :, s3]
    sig = [at(exact(scale), s) for s in (s1, s2, s3)]
    D1, D2, D3 = (at(exact(D), s) for s in (s1, s2, s3))
    P1, P2, P3 = (at(P, s) for s in (s1, s2, s3))
    Ja, Jb, Jc = at(legs[a][4], s1), at(legs[b][4], s2), at(legs[c][4], s3)
    B1h = prod(*sig, D1, D2, D3, mass_sum(wn, wa, wb, wc))
    two = add(prod(D1, D2, mass_sum(wnb, wa, wb), Jc, P3), prod(D2, D3, mass_sum(wnb, wb, wc), Ja, P1),
              prod(D1, D3, mass_sum(wnb, wa, wc), Jb, P2))
    B2h = prod(*sig, two)
    k1, k2, k3 = ksamp[:, s1], ksamp[:, s2], ksamp[:, s3]
    B3h = prod(*sig, Ja, Jb, Jc, tree_tol(k1, k2, k3, P1, P2, P3))

    def stack(i):
        return tuple(np.stack([legs[nm_][i][j] for nm_ in names]) for j in (0, 1))

    return dict(B1h=B1h, B2h=B2h, B3h=B3h, J=stack(4), I=stack(1), C=stack(2), b=stack(3), P=P, k=ksamp, D=D)


def zsum(g, B):
    """(Bz, tol) of Bz[t] = sum_z g[z] B[z,t] for B = (value, tol), each (nz, nt), as trispectrum_model.zsum: the tols
    summed with |g| plus nz 2^-53 of the absolute sum."""
    g = np.asarray(g, dtype=float)
    absum = np.einsum("z,zt->t", np.abs(g), np.abs(B[0]))
    return np.einsum("z,zt->t", g, B[0]), np.einsum("z,zt->t", np.abs(g), B[1]) + g.size * 0.5 * EPS * absum
