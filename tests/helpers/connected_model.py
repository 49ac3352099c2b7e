"""Numpy restatement of the 2-, 3- and 4-halo terms of the trispectrum from a HaloModel's host
arrays alone, and a 40-digit mpmath evaluator of the perturbation-theory quantities and of one element's terms.  The
tensors it reads are produced by code this feature does not touch; what a comparison with this tests is the device's PT
kernel, its mass contraction, its loader and its epilogue.

Every quantity is a pair (value, tol), with the rules of helpers/bispectrum_model.py (EPS = 2^-52: a count of roundings
times 2^-53 on each of the two sides): a product carries sum_i tol_i prod_{j != i} |x_j| plus one EPS of |value| per
multiplication, a sum the sum of the tols plus one EPS of the absolute sum of the addends per addition - so a
cancellation, in F3s or between the F2 pairs, is priced at the size of what cancels.  Beyond those rules:

* mass sums: (nm + 40) EPS A, A the sum over absolute values (section 16);
* 1 -+ mu and the weights of the rule are exact (both sides read the same arrays); k_s, D_s and the scales are exact;
* q-+^2 = d^2 + 2 k_a k_b (1 -+ mu): 4 EPS of the absolute sum; the square root halves the relative tol and adds one EPS;
* plin_at: with C_LOG, C_EXP the device's log and exp in ulp (measured on the device against mpmath through the math
  probe: 0.70 and 0.81 ulp, times the project's factor 4 between two good libraries; numpy's are within 1 ulp),
  ln x carries (C_LOG + 1) u |ln x| + rel(x); t = (lq - x0) / (x1 - x0) and y = y0 + t (y1 - y0) by the product and sum
  rules; P = exp(y) carries |P| (tol_y + (C_EXP + 1) u).  A node of the table that the two sides assign to different panels
  is covered: the interpolant is continuous and both panels' values are within that tol of it;
* F2 (section 16's bound) with the closing side's own tol entering through mu: dmu += (r tol_r + p tol_p) / (p q) ... see
  F2_pair.
"""
import itertools

import numpy as np

from hmvec_amd import bispectrum as bs
from hmvec_amd import connected as cn
from hmvec_amd.quadrature import trapz_weights

import bispectrum_model as bm
import trispectrum_model as tm

EPS = bm.EPS
U = 2.0 ** -53
C_LOG = 4 * 0.70          # ulp: log_fast on an MI355X against mpmath (0.70), times 4
C_EXP = 4 * 0.81          # ulp: exp_fast on an MI355X against mpmath (0.81), times 4
prod, add, exact = bm.prod, bm.add, bm.exact


def scale(x, c):
    """(value, tol) of an exact factor (a power of two, or a constant both sides hold) times x, one rounding."""
    return c * x[0], abs(c) * x[1] + EPS * np.abs(c * x[0])


def neg(x):
    return -x[0], x[1]


def div(x, y):
    """(value, tol) of x / y."""
    v = x[0] / y[0]
    return v, x[1] / np.abs(y[0]) + np.abs(v) * y[1] / np.abs(y[0]) + EPS * np.abs(v)


def sqrt(x):
    v = np.sqrt(x[0])
    return v, 0.5 * x[1] / v + EPS * v


def log(x):
    v = np.log(x[0])
    return v, (C_LOG + 1) * U * np.abs(v) + x[1] / np.abs(x[0])


# ---------------------------------------------------------------------------------------- plin_at
def plin_tol(lnk, lnP, q):
    """(P(q), tol); lnk, lnP are (value, tol) pairs of the row's tables, q a (value, tol) pair."""
    lq = log(q)
    lo = np.clip(np.searchsorted(lnk[0], lq[0], side="right") - 1, 0, lnk[0].size - 2)
    x0, x1 = (lnk[0][lo], lnk[1][lo]), (lnk[0][lo + 1], lnk[1][lo + 1])
    y0, y1 = (lnP[0][lo], lnP[1][lo]), (lnP[0][lo + 1], lnP[1][lo + 1])
    t = div(add(lq, neg(x0)), add(x1, neg(x0)))
    y = add(prod(t, add(y1, neg(y0))), y0)
    v = np.exp(y[0])
    return v, v * (y[1] + (C_EXP + 1) * U)


def row_tables(ks, Pz):
    """The (value, tol) pairs of ln ks and ln Pzk[z]: each side takes the logarithm of the same numbers."""
    return log(exact(ks)), log(exact(Pz))


# ---------------------------------------------------------------------------------------- F2 with inexact sides
def F2_pair(p, q, r):
    """(F2(p, q; r), tol) of (value, tol) sides: section 16's bound (bispectrum_model.F2_tol) plus what the sides' own
    tols move: mu = ((r - a)(r + a) - b^2) / (2 a b) with a >= b the two sides has |dmu/dr| = r / (a b),
    |dmu/da| <= (1 + |mu|) / b ... bounded by (a + |mu| b) / (a b), |dmu/db| <= (b + |mu| a) / (a b); F2 depends on the
    sides through mu and through s = a/b + b/a, |ds| <= (a^2 + b^2) / (a b) (|da|/a + |db|/b)."""
    (pv, pt), (qv, qt), (rv, rt) = p, q, r
    swap = qv > pv
    a, at = np.where(swap, qv, pv), np.where(swap, qt, pt)
    b, bt = np.where(swap, pv, qv), np.where(swap, pt, qt)
    val, tol = bm.F2_tol(a, b, rv)
    mu = np.clip(((rv - a) * (rv + a) - b * b) / (2.0 * a * b), -1.0, 1.0)
    s = a / b + b / a
    dmu = (rv * rt + (a + np.abs(mu) * b) * at + (b + np.abs(mu) * a) * bt) / (a * b)
    ds = s * (at / a + bt / b)
    return val, tol + dmu * (0.5 * s + (4.0 / 7.0) * np.abs(mu)) + 0.5 * np.abs(mu) * ds


# ---------------------------------------------------------------------------------------- F3s
def F3s_tol(k, kp, mu, omm, opm, qm2, qp2):
    """(F3s(k, -k, k'), tol) by the form of hmvec_amd.connected.F3s, term by term; k, kp exact arrays, mu, omm, opm exact
    scalars, qm2, qp2 (value, tol) pairs."""
    K, KP, MU, OMM, OPM = exact(k), exact(kp), exact(mu), exact(omm), exact(opm)
    s = add(div(K, KP), div(KP, K))
    h = scale(prod(MU, s), 0.5)
    m2 = prod(MU, MU)
    e2 = add(scale(m2, 2.0 / 7.0), exact(5.0 / 7.0))
    g2 = add(scale(m2, 4.0 / 7.0), exact(3.0 / 7.0))
    dk = add(KP, neg(K))
    r = div(KP, K)
    a = scale(prod(r, MU), 7.0)
    Am = add(scale(add(prod(K, OMM), dk), 7.0), scale(prod(r, add(dk, neg(prod(KP, OMM)))), 2.0))
    Ap = add(scale(add(prod(K, OPM), dk), 7.0), scale(prod(r, add(prod(KP, OPM), neg(dk))), -2.0))
    tm_ = add(prod(add(g2, neg(h)), div(KP, qm2), Am), prod(a, add(e2, neg(h))))
    tp_ = add(prod(add(g2, h), div(KP, qp2), Ap), neg(prod(a, add(e2, h))))
    return scale(add(tm_, tp_), 1.0 / 54.0)


# ---------------------------------------------------------------------------------------- the PT matrices
def pt_matrices(ks, Pzk, idx, frac, rule):
    """{"Pbar", "Bbar", "Tbar"}: (value, tol) pairs, each (nz, n, n), by the contract's order of operations: each unordered
    pair once, its sides ordered by (k, P), the rule walked in node order, mirrored."""
    ks, Pzk = np.asarray(ks, dtype=float), np.asarray(Pzk, dtype=float)
    nz, n = idx.shape
    ksamp = bs.sample_wavenumbers(ks, idx, frac)
    Ps = cn.sampled_plin(Pzk, idx, frac)
    val, tol = np.zeros((3, nz, n, n)), np.zeros((3, nz, n, n))
    i, j = np.triu_indices(n)
    for z in range(nz):
        lnk, lnP = row_tables(ks, Pzk[z])
        k1, k2, P1, P2 = ksamp[z, i], ksamp[z, j], Ps[z, i], Ps[z, j]
        first = (k1 > k2) | ((k1 == k2) & (P1 >= P2))
        ka, kb = np.where(first, k1, k2), np.where(first, k2, k1)
        Pa = (np.where(first, P1, P2), 3 * EPS * np.where(first, P1, P2))
        Pb = (np.where(first, P2, P1), 3 * EPS * np.where(first, P2, P1))
        KA, KB = exact(ka), exact(kb)
        d = add(KA, neg(KB))
        d2, c2 = prod(d, d), scale(prod(KA, KB), 2.0)
        sums = [[], [], []]
        for mu, omm, opm, w in zip(rule.mu, rule.one_minus_mu, rule.one_plus_mu, rule.weights):
            qm2, qp2 = add(prod(c2, exact(omm)), d2), add(prod(c2, exact(opm)), d2)
            qm, qp = sqrt(qm2), sqrt(qp2)
            Pm, Pp = plin_tol(lnk, lnP, qm), plin_tol(lnk, lnP, qp)
            f1p, f2p = F2_pair(qp, KB, KA), F2_pair(qp, KA, KB)
            f1m, f2m = F2_pair(qm, KB, KA), F2_pair(qm, KA, KB)
            up, um = add(prod(f1p, Pb), prod(f2p, Pa)), add(prod(f1m, Pb), prod(f2m, Pa))
            B = scale(add(prod(F2_pair(KA, KB, qp), Pa, Pb), prod(Pp, up)), 2.0)
            F3 = add(prod(F3s_tol(ka, kb, mu, omm, opm, qm2, qp2), exact(12.0), Pa, Pa, Pb),
                     prod(F3s_tol(kb, ka, mu, omm, opm, qm2, qp2), exact(12.0), Pb, Pb, Pa))
            T = add(prod(exact(4.0), Pp, up, up), prod(exact(4.0), Pm, um, um), F3)
            W = exact(w)
            for q, x in enumerate((Pp, B, T)):
                sums[q].append(prod(W, x))
        for q in range(3):
            v, t = add(*sums[q])
            val[q, z, i, j], tol[q, z, i, j] = v, t
            val[q, z, j, i], tol[q, z, j, i] = v, t
    return {key: (val[q], tol[q]) for q, key in enumerate(("Pbar", "Bbar", "Tbar"))}


# ---------------------------------------------------------------------------------------- the same-halo factors
def hod_sampled(h, name, idx, frac):
    """(u_c, u_s)[z,m,s] of an HOD at the samples (u_c == 1 without a central profile), and <NcNs>/ngal^2,
    <Ns(Ns-1)>/ngal^2 [z,m]."""
    hod, uc, us = tm._hod_parts(h, name)
    nz, nm = h.nzm.shape
    one = np.ones(idx.shape)
    shape = (nz, nm, h.ks.size)
    us = tm.sampled(np.broadcast_to(us, shape), idx, frac, one)
    uc = tm.sampled(np.broadcast_to(uc, shape), idx, frac, one) if hod["central_profile"] is not None else np.ones_like(us)
    ng2 = hod["ngal"][:, None] ** 2.0
    return uc, us, hod["NcNs"] / ng2, hod["NsNsm1"] / ng2


def pair_term(h, name, idx, frac):
    """s_gg[z,m,i,j] of twice the HOD `name`: the two-wavenumber pair term, which has no self-pairs."""
    uc, us, cN, cS = hod_sampled(h, name, idx, frac)
    cN, cS = cN[:, :, None, None], cS[:, :, None, None]
    return ((uc[:, :, :, None] * us[:, :, None, :] + us[:, :, :, None] * uc[:, :, None, :]) * cN
            + cS * us[:, :, :, None] * us[:, :, None, :])


def connected(h, names, rule, kindex=None, idx=None, frac=None, scale=None, damping=True):
    """The five terms of the quadruple `names` at the samples: a dict of (value, tol) pairs T1h, T2h13, T2h22, T3h, T4h
    (nz, n, n), the PT matrices Pbar, Bbar, Tbar, and J by name."""
    a, b, c, d = names
    idx, frac, scl = tm.tables(h, kindex=kindex, idx=idx, frac=frac, scale=scale, damping=False)
    nz, nm = h.nzm.shape
    ksamp = bs.sample_wavenumbers(h.ks, idx, frac)
    D = bs.damping(ksamp, h.p["kstar_damping"]) if damping else np.ones_like(ksamp)
    Pv = cn.sampled_plin(h.Pzk, idx, frac)
    P = (Pv, 3 * EPS * np.abs(Pv))
    legs = {nm_: bm.leg_terms(h, nm_, idx, frac) for nm_ in dict.fromkeys(names)}
    one = np.ones(idx.shape)
    S = {pair: tm.sampled(tm.square_term(h, *pair), idx, frac, one) for pair in dict.fromkeys([(a, b), (c, d)])}
    wnb = trapz_weights(h.ms)[None, :] * h.nzm * h.bh
    pt = pt_matrices(h.ks, h.Pzk, idx, frac, rule)

    def col(x):            # a (value, tol) pair (nz, n) along i
        return x[0][:, :, None], x[1][:, :, None]

    def row(x):
        return x[0][:, None, :], x[1][:, None, :]

    def I3(x, pair, at_i):     # I_{x,pair}: leg x at i (at_i) or j, the pair's square term at the other sample
        w, s = legs[x][0], S[pair]
        if at_i:
            return bm.mass_sum(wnb, w[:, :, :, None], s[:, :, None, :])
        return bm.mass_sum(wnb, s[:, :, :, None], w[:, :, None, :])

    def I2(x, y):
        if x == y and bm.kind(h, x) == "h":
            return bm.mass_sum(wnb, pair_term(h, x, idx, frac))
        return bm.mass_sum(wnb, legs[x][0][:, :, :, None], legs[y][0][:, :, None, :])

    Ja, Jb, Jc, Jd = col(legs[a][4]), col(legs[b][4]), row(legs[c][4]), row(legs[d][4])
    Pi, Pj = col(P), row(P)
    sig = prod(col(exact(scl)), row(exact(scl)))
    DD = prod(col(exact(D)), row(exact(D)))
    Iac, Iad, Ibc, Ibd = I2(a, c), I2(a, d), I2(b, c), I2(b, d)
    t13 = add(prod(Pi, add(prod(Ja, I3(b, (c, d), True)), prod(Jb, I3(a, (c, d), True)))),
              prod(Pj, add(prod(Jc, I3(d, (a, b), False)), prod(Jd, I3(c, (a, b), False)))))
    t22 = prod(pt["Pbar"], add(prod(Iac, Ibd), prod(Iad, Ibc)))
    t3 = prod(pt["Bbar"], add(prod(Iac, Jb, Jd), prod(Ibd, Ja, Jc), prod(Iad, Jb, Jc), prod(Ibc, Ja, Jd)))
    t4 = prod(pt["Tbar"], Ja, Jb, Jc, Jd)
    # T1h: section 15's restatement with its own scale (the damping folded in) and gate
    i1, f1, s1 = tm.tables(h, idx=idx, frac=frac, scale=scl, damping=damping)
    T1, A1 = tm.contract(h.nzm, h.ms, tm.sampled(tm.square_term(h, a, b), i1, f1, s1),
                         tm.sampled(tm.square_term(h, c, d), i1, f1, s1))
    out = dict(T1h=(T1, tm.gate(A1, nm)), T2h13=prod(sig, DD, t13), T2h22=prod(sig, DD, DD, t22), T3h=prod(sig, DD, t3),
               T4h=prod(sig, t4), J={nm_: legs[nm_][4] for nm_ in legs}, k=ksamp, D=D, P=P)
    out.update(pt)
    return out


TERMS = ("T1h", "T2h13", "T2h22", "T3h", "T4h")


def zsum(g, T):
    """(Tz, tol) of sum_z g[z] T[z] for T = (value, tol), each (nz, n, n)."""
    g = np.asarray(g, dtype=float)
    absum = np.einsum("z,zij->ij", np.abs(g), np.abs(T[0]))
    return np.einsum("z,zij->ij", g, T[0]), np.einsum("z,zij->ij", np.abs(g), T[1]) + g.size * 0.5 * EPS * absum


# ---------------------------------------------------------------------------------------- the general formulas (vectors)
def _F2G2(mp_or_np, k1, k2):
    """Symmetrised (F2, G2) of two vectors; zero where their sum vanishes."""
    dot = sum(x * y for x, y in zip(k1, k2))
    n1, n2 = sum(x * x for x in k1), sum(x * x for x in k2)
    mu = dot / mp_or_np.sqrt(n1 * n2)
    s = mp_or_np.sqrt(n1 / n2) + mp_or_np.sqrt(n2 / n1)
    return (5 + 7 * mu * s / 2 + 2 * mu * mu) / 7, (3 + 7 * mu * s / 2 + 4 * mu * mu) / 7


def _alpha_beta(k1, k2):
    k = [x + y for x, y in zip(k1, k2)]
    n1, n2 = sum(x * x for x in k1), sum(x * x for x in k2)
    return (sum(x * y for x, y in zip(k, k1)) / n1,
            sum(x * x for x in k) * sum(x * y for x, y in zip(k1, k2)) / (2 * n1 * n2))


def F3s_recursion(lib, q1, q2, q3):
    """Symmetrised F3 of three vectors from the recursion for F_n, G_n (Bernardeau et al. 2002, eqs. 43-44), over the six
    orderings; an ordering whose partial sum q_b + q_c vanishes is dropped (its F2 and G2 are zero).  lib: numpy or
    mpmath; the vectors are sequences of its numbers."""
    total = 0
    for a, b, c in itertools.permutations((q1, q2, q3)):
        p = [x + y for x, y in zip(b, c)]
        if all(x == 0 for x in p):
            continue
        F2bc, G2bc = _F2G2(lib, b, c)
        al_ap, be = _alpha_beta(a, p)
        al_pa, _ = _alpha_beta(p, a)
        total = total + (7 * al_ap * F2bc + 2 * be * G2bc + G2bc * (7 * al_pa + 2 * be)) / 18
    return total / 6


def trispectrum_general(lib, ks4, plin, P=None):
    """The tree-level trispectrum of four vectors that sum to zero by the general formula: 4 times the twelve
    permutations of F2 F2 P P P - three partitions into two pairs, {a, b} carrying q = k_a + k_b and {c, d} carrying -q,
    times one leg of each pair - plus 6 times the four permutations of F3s P P P; a term whose internal momentum
    vanishes is dropped.  plin(|k|) is the linear spectrum; P, if given, the four legs' own (sampled) spectra."""
    norm = lambda v: lib.sqrt(sum(x * x for x in v))      # noqa: E731
    P = [plin(norm(v)) for v in ks4] if P is None else P
    total = 0
    for b in (1, 2, 3):
        c, d = [x for x in (1, 2, 3) if x != b]
        q = [x + y for x, y in zip(ks4[0], ks4[b])]
        if all(x == 0 for x in q):
            continue
        Pq, mq = plin(norm(q)), [-x for x in q]
        for x in (0, b):
            for y in (c, d):
                total = total + 4 * _F2G2(lib, q, [-v for v in ks4[x]])[0] * _F2G2(lib, mq, [-v for v in ks4[y]])[0] \
                    * P[x] * P[y] * Pq
    for omit in range(4):
        tr = [x for x in range(4) if x != omit]
        total = total + 6 * F3s_recursion(lib, *(ks4[x] for x in tr)) * P[tr[0]] * P[tr[1]] * P[tr[2]]
    return total


# ---------------------------------------------------------------------------------------- mpmath, 40 digits
DPS = 40


def mp_plin(ks, Pz):
    import mpmath as mp
    lnk = [mp.log(mp.mpf(float(v))) for v in ks]
    lnP = [mp.log(mp.mpf(float(v))) for v in Pz]

    def at(q):
        lq = mp.log(q)
        lo = 0
        while lo < len(lnk) - 2 and lnk[lo + 1] <= lq:
            lo += 1
        t = (lq - lnk[lo]) / (lnk[lo + 1] - lnk[lo])
        return mp.exp(lnP[lo] + t * (lnP[lo + 1] - lnP[lo]))
    return at


def mp_pt_element(ks, Pz, ki, kj, Pi, Pj, rule):
    """(Pbar, Bbar, Tbar) of one element at 40 digits, from vectors: k_i along x, k_j at the rule's angle - its sine
    from (1 - mu)(1 + mu) -, F2 from dot products, F3s from the recursion, the trispectrum by the general formula.  The
    four legs read their own sampled spectra P_i, P_j (floats or mpmath numbers), the internal lines the interpolant."""
    import mpmath as mp
    with mp.workdps(DPS):
        plin = mp_plin(ks, Pz)
        ki, kj, Pi, Pj = (mp.mpf(v) for v in (ki, kj, Pi, Pj))
        out = [mp.mpf(0)] * 3
        for omm, opm, w in zip(rule.one_minus_mu, rule.one_plus_mu, rule.weights):
            omm, opm, w = mp.mpf(float(omm)), mp.mpf(float(opm)), mp.mpf(float(w))
            mu, sn = (opm - omm) / 2, mp.sqrt(omm * opm)
            v1, v2 = [ki, mp.mpf(0)], [kj * mu, kj * sn]
            m1, m2 = [-x for x in v1], [-x for x in v2]
            qp = [x + y for x, y in zip(v1, v2)]
            Pp = plin(mp.sqrt(sum(x * x for x in qp)))
            B = 2 * (_F2G2(mp, qp, m1)[0] * Pp * Pi + _F2G2(mp, qp, m2)[0] * Pp * Pj + _F2G2(mp, v1, v2)[0] * Pi * Pj)
            T = trispectrum_general(mp, [v1, m1, v2, m2], plin, [Pi, Pi, Pj, Pj])
            out = [out[0] + w * Pp, out[1] + w * B, out[2] + w * T]
        return out


def mp_element(h, names, rule, z, i, j, idx, frac, scl, damping=True):
    """The five terms and the three PT quantities of one element (z, i, j) at 40 digits, from the model's host tensors:
    every weight, square term, mass sum, bracket and PT quantity in mpmath.  k_s, D_s, the scales and the 1-halo term's
    folded scale are the contract's own float sequences and enter as they are."""
    import mpmath as mp
    a, b, c, d = names
    with mp.workdps(DPS):
        M = lambda v: mp.mpf(float(v))      # noqa: E731
        nm = h.ms.size
        wts, rho = trapz_weights(h.ms), float(h.rho_matter_z(0)[0])
        wn = [M(wts[m]) * M(h.nzm[z, m]) for m in range(nm)]
        wnb = [wn[m] * M(h.bh[z, m]) for m in range(nm)]

        def interp(fn, s):
            node, f = int(idx[z, s]), M(frac[z, s])
            return fn(node) if f == 0 else (1 - f) * fn(node) + f * fn(node + 1)

        def hod_u(name, m, node):
            hod = h.hods[name]
            uc = mp.mpf(1) if hod["central_profile"] is None else M(h.uk_profiles[hod["central_profile"]][z, m, node])
            return hod, uc, M(h.uk_profiles[hod["satellite_profile"]][z, m, node])

        def w_node(name, m, node):
            kind = tm._kind(h, name)
            if kind == "h":
                hod, uc, us = hod_u(name, m, node)
                return (uc * M(hod["Nc"][z, m]) + us * M(hod["Ns"][z, m])) / M(hod["ngal"][z])
            if kind == "m":
                return M(h.ms[m]) * M(h.uk_profiles[name][z, m, node]) / M(rho)
            return M(h.pk_profiles[name][z, m, node])

        def S_node(x, y, m, node):
            kx, ky = tm._kind(h, x), tm._kind(h, y)
            if kx == "h" and ky == "h":
                hod, uc, us = hod_u(x, m, node)
                return (2 * uc * us * M(hod["NcNs"][z, m]) + M(hod["NsNsm1"][z, m]) * us * us) / M(hod["ngal"][z]) ** 2
            if kx == "p" and ky == "p":
                return M(h.pk_profiles[x][z, m, node]) ** 2
            return w_node(x, m, node) * w_node(y, m, node)

        def w_at(name, s):
            return [interp(lambda node: w_node(name, m, node), s) for m in range(nm)]

        def S_at(x, y, s):
            return [interp(lambda node: S_node(x, y, m, node), s) for m in range(nm)]

        def J_at(name, s):
            I = mp.fsum(p * q for p, q in zip(wnb, w_at(name, s)))
            if tm._kind(h, name) == "m":
                return I + 1 - mp.fsum(wnb[m] * M(h.ms[m]) / M(rho) for m in range(nm))
            return I          # pressure: b = C = 0; an HOD: b = C

        def I2(x, y):
            if x == y and tm._kind(h, x) == "h":
                hod = h.hods[x]
                ng2 = M(hod["ngal"][z]) ** 2
                tot = mp.mpf(0)
                for m in range(nm):
                    uci, usi = (interp(lambda node: hod_u(x, m, node)[q], i) for q in (1, 2))
                    ucj, usj = (interp(lambda node: hod_u(x, m, node)[q], j) for q in (1, 2))
                    tot += wnb[m] * ((uci * usj + usi * ucj) * M(hod["NcNs"][z, m]) + M(hod["NsNsm1"][z, m]) * usi * usj) / ng2
                return tot
            return mp.fsum(p * q * r for p, q, r in zip(wnb, w_at(x, i), w_at(y, j)))

        ksamp = bs.sample_wavenumbers(h.ks, idx, frac)
        D = bs.damping(ksamp, h.p["kstar_damping"]) if damping else np.ones_like(ksamp)
        Pi, Pj = (interp(lambda node: M(h.Pzk[z, node]), s) for s in (i, j))
        Pbar, Bbar, Tbar = mp_pt_element(h.ks, h.Pzk[z], float(ksamp[z, i]), float(ksamp[z, j]), Pi, Pj, rule)
        Sab_i, Scd_j = S_at(a, b, i), S_at(c, d, j)
        I3 = lambda w, S: mp.fsum(p * q * r for p, q, r in zip(wnb, w, S))      # noqa: E731
        Ja, Jb, Jc, Jd = J_at(a, i), J_at(b, i), J_at(c, j), J_at(d, j)
        sig, DD = M(scl[z, i]) * M(scl[z, j]), M(D[z, i]) * M(D[z, j])
        Iac, Iad, Ibc, Ibd = I2(a, c), I2(a, d), I2(b, c), I2(b, d)
        t13 = (Pi * (Ja * I3(w_at(b, i), Scd_j) + Jb * I3(w_at(a, i), Scd_j))
               + Pj * (Jc * I3(w_at(d, j), Sab_i) + Jd * I3(w_at(c, j), Sab_i)))
        _, _, s1 = tm.tables(h, idx=idx, frac=frac, scale=scl, damping=damping)
        T1 = M(s1[z, i]) * M(s1[z, j]) * mp.fsum(p * q * r for p, q, r in zip(wn, Sab_i, Scd_j))
        return dict(T1h=T1, T2h13=sig * DD * t13, T2h22=sig * DD * DD * Pbar * (Iac * Ibd + Iad * Ibc),
                    T3h=sig * DD * Bbar * (Iac * Jb * Jd + Ibd * Ja * Jc + Iad * Jb * Jc + Ibc * Ja * Jd),
                    T4h=sig * Tbar * Ja * Jb * Jc * Jd, Pbar=Pbar, Bbar=Bbar, Tbar=Tbar)


def mp_err(got, ref):
    """|got - ref| of a float against an mpmath number, as a float."""
    import mpmath as mp
    with mp.workdps(DPS):
        return float(abs(mp.mpf(float(got)) - ref))


def view(h, z0, z1, nm):
    """A stand-in for the model restricted to the redshifts z0 .. z1 - 1 and the first nm masses, with the attributes this
    module and the two it builds on read.  An HOD keeps its ngal (the device reads the same number)."""
    import types
    zs, ms = slice(z0, z1), slice(0, nm)
    cut = lambda t: np.ascontiguousarray(np.broadcast_to(t, h.nzm.shape + (h.ks.size,))[zs, ms])      # noqa: E731
    hods = {}
    for name, hod in h.hods.items():
        hods[name] = dict(central_profile=hod["central_profile"], satellite_profile=hod["satellite_profile"],
                          ngal=np.asarray(hod["ngal"])[zs],
                          **{key: np.asarray(hod[key])[zs, ms] for key in ("Nc", "Ns", "NcNs", "NsNsm1")})
    rho = h.rho_matter_z(0)
    return types.SimpleNamespace(zs=h.zs[zs], ks=h.ks, ms=h.ms[ms], nzm=h.nzm[zs, ms], bh=h.bh[zs, ms], Pzk=h.Pzk[zs], p=h.p,
                                 hods=hods, uk_profiles={k: cut(v) for k, v in h.uk_profiles.items()},
                                 pk_profiles={k: cut(v) for k, v in h.pk_profiles.items()},
                                 rho_matter_z=lambda z: rho)
