"""The 2-, 3- and 4-halo terms of the trispectrum of two halo-model spectra and the connected covariance they give
(DESIGN.md section 31).

``connected_trispectrum_device`` / ``get_trispectrum`` contract T(k_i, -k_i, k_j, -k_j) of the spectra (a, b) at +-k_i
and (c, d) at +-k_j, averaged over the angle between k_i and k_j, on the GPU over the resident tensors: the 1-halo term
of section 15, the two 2-halo terms (3+1 and 2+2), the 3-halo term and the 4-halo term with the tree-level matter
trispectrum.  ``cl_cov_connected`` is their Limber projection.  This module also holds the host side of the contract,
plain arithmetic that the device follows: the angle rules, ``plin_at``, ``F3s``, ``tree_trispectrum`` and
``pt_averages``.  Linear halo bias only: no b_2, no b_3.  The model carries no third factorial moment of an HOD:
three or four galaxies in one halo are formed as w_g S_gg and S_gg S_gg (section 15's convention).  These are functions
of a model, not methods of it.
"""
import ctypes as C
import math
from dataclasses import dataclass

import numpy as np

from . import _native as nat
from . import bispectrum as bispec
from .bispectrum import F2
from .cov import limber_samples
from .quadrature import trapz_weights
from .spectra import _same_lookups

__all__ = ["AngleRule", "angle_rule", "plin_at", "F3s", "tree_trispectrum", "pt_averages", "pt_averages_device",
           "connected_trispectrum_device", "get_trispectrum", "cl_cov_connected"]

TERMS = ("1h", "2h13", "2h22", "3h", "4h")
MAX_SAMPLES = 256
MAX_NODES = 256
MAX_NK = 8192
_LD = np.longdouble
_PI = _LD("3.14159265358979323846264338327950288")


# ---------------------------------------------------------------------------------------- the angle rules
@dataclass(frozen=True, eq=False)
class AngleRule:
    """Nodes and weights of an average over the cosine mu of the angle between two wavevectors: mu, one_minus_mu,
    one_plus_mu and weights, each (nr,), read-only.  1 -+ mu are arrays of their own, formed without cancellation: the
    wavenumbers |k_i -+ k_j| are made from them.  Refused: no node or more than 256, a node at +-1 (|k_i - k_i| = 0),
    non-finite values, 1 -+ mu not positive, weights that do not sum to 1 within 4 ulp."""
    mu: np.ndarray
    one_minus_mu: np.ndarray
    one_plus_mu: np.ndarray
    weights: np.ndarray
    measure: str = "custom"

    def __post_init__(self):
        arrs = []
        for name in ("mu", "one_minus_mu", "one_plus_mu", "weights"):
            a = np.array(getattr(self, name), dtype=np.float64).reshape(-1)
            a.setflags(write=False)
            object.__setattr__(self, name, a)
            arrs.append(a)
        mu, omm, opm, w = arrs
        if not 1 <= mu.size <= MAX_NODES:
            raise ValueError(f"an angle rule has 1 to {MAX_NODES} nodes, got {mu.size}")
        if not (omm.size == opm.size == w.size == mu.size):
            raise ValueError("mu, one_minus_mu, one_plus_mu and weights must have one entry per node")
        if not all(np.all(np.isfinite(a)) for a in arrs):
            raise ValueError("an angle rule must be finite")
        if np.any(np.abs(mu) >= 1.0) or np.any(omm <= 0.0) or np.any(opm <= 0.0):
            raise ValueError("an angle rule must not have a node at mu = +-1 (1 - mu and 1 + mu must be positive)")
        if np.any(np.abs((1.0 - mu) - omm) > 4 * np.spacing(1.0)) or np.any(np.abs((1.0 + mu) - opm) > 4 * np.spacing(1.0)):
            raise ValueError("one_minus_mu / one_plus_mu are not 1 -+ mu")
        if abs(math.fsum(w) - 1.0) > 4 * np.spacing(1.0):
            raise ValueError(f"the weights of an angle rule must sum to 1 within 4 ulp, got {math.fsum(w)!r}")

    @property
    def nr(self):
        return self.mu.size


def _legendre_roots(n):
    """(t, w) of Gauss-Legendre on [-1, 1] for the roots x = 1 - t >= 0, in extended precision: Newton in t = 1 - x on the
    recurrence written for differences, D_{k+1} = (k D_k - (2k + 1) t P_k) / (k + 1), P_{k+1} = P_k + D_{k+1}, which
    forms nothing by cancellation, so t keeps its relative accuracy next to x = 1."""
    half = (n + 1) // 2
    theta = _PI * (4 * np.arange(1, half + 1, dtype=_LD) - 1) / (4 * n + 2)
    t = 2 * np.sin(theta / 2) ** 2
    for _ in range(12):
        P, D = np.ones_like(t), np.zeros_like(t)
        for k in range(n):
            D = (k * D - (2 * k + 1) * t * P) / (k + 1)
            P = P + D
        dP = n * (t * P - D) / (t * (2 - t))               # P_n'(x) = n (P_{n-1} - x P_n) / (1 - x^2)
        t = t + P / dP
    if n % 2:
        t[-1] = _LD(1)
    P, D = np.ones_like(t), np.zeros_like(t)
    for k in range(n):
        D = (k * D - (2 * k + 1) * t * P) / (k + 1)
        P = P + D
    return t, 2 * t * (2 - t) / (_LD(n) * n * D * D)


def angle_rule(n, measure="2d"):
    """The checked, immutable AngleRule of n nodes (1 .. 256).

    measure="3d": Gauss-Legendre in mu with weight 1/2, the average over directions in space - the covariance of P(k) in
    shells; exact for polynomials in mu of degree 2n - 1.  measure="2d": Gauss-Chebyshev, mu = cos((2t - 1) pi / 2n) with
    equal weights, the average over the angle between l and l' in the plane of the sky, which a Limber-projected
    covariance needs; exact for polynomials in mu of degree 2n - 1.  1 -+ mu are 2 sin^2 and 2 cos^2 of the half angle
    (Chebyshev) or carried through the root search (Legendre), formed in extended precision: correctly rounded where
    numpy's long double is wider than a double."""
    n = int(n)
    if not 1 <= n <= MAX_NODES:
        raise ValueError(f"an angle rule has 1 to {MAX_NODES} nodes, got {n}")
    if measure == "2d":
        theta = (2 * np.arange(1, n + 1, dtype=_LD) - 1) * _PI / (2 * n)
        omm, opm = 2 * np.sin(theta / 2) ** 2, 2 * np.cos(theta / 2) ** 2
        mu, w = np.cos(theta), np.full(n, 1.0 / n)
    elif measure == "3d":
        t, wt = _legendre_roots(n)
        mirror = slice(None, None, -1) if n % 2 == 0 else slice(-2, None, -1)
        omm = np.concatenate([t, (2 - t)[mirror]])
        opm = np.concatenate([2 - t, t[mirror]])
        mu = np.concatenate([1 - t, (t - 1)[mirror]])
        w = np.concatenate([wt, wt[mirror]]) / 2
    else:
        raise ValueError(f"measure must be '2d' or '3d', got {measure!r}")
    return AngleRule(mu.astype(np.float64), omm.astype(np.float64), opm.astype(np.float64), np.asarray(w, dtype=np.float64),
                     measure)


def _rule(rule):
    if not isinstance(rule, AngleRule):
        raise ValueError("rule must be an AngleRule (angle_rule(n, measure))")
    return rule


# ---------------------------------------------------------------------------------------- perturbation theory, host
def plin_at(ks, P, q):
    """P_lin at the wavenumbers q from its table P (nk,) on ks: linear in (ln k, ln P), continued beyond either end
    with the end panel's slope.  The panel is the last one whose left node is <= ln q."""
    lnk, lnP = np.log(np.asarray(ks, dtype=np.float64)), np.log(np.asarray(P, dtype=np.float64))
    if lnk.ndim != 1 or lnk.size < 2 or lnP.shape != lnk.shape:
        raise ValueError("ks and P must be one-dimensional, of one length, at least two points")
    lq = np.log(np.asarray(q, dtype=np.float64))
    lo = np.clip(np.searchsorted(lnk, lq, side="right") - 1, 0, lnk.size - 2)
    t = (lq - lnk[lo]) / (lnk[lo + 1] - lnk[lo])
    return np.exp(t * (lnP[lo + 1] - lnP[lo]) + lnP[lo])


def _pm(mu, omm, opm):
    mu = np.asarray(mu, dtype=np.float64)
    return mu, (1.0 - mu if omm is None else np.asarray(omm, dtype=np.float64)), (
        1.0 + mu if opm is None else np.asarray(opm, dtype=np.float64))


def F3s(k, kp, mu, one_minus_mu=None, one_plus_mu=None):
    """The symmetrised third-order kernel F3s(k, -k, k') of the standard recursion for F_n, G_n (Goroff et al. 1986;
    Bernardeau et al. 2002, eqs. 43-44), mu the cosine between k and k'; the orderings whose partial sum k - k vanishes
    are dropped (their G2 factor is zero).  With r = k'/k and q-+ = |k' -+ k|,

        54 F3s = 7 r mu F2(-k,k') + G2(-k,k') (k'/q-^2) [7 (k' - k mu) + 2 r (k' mu - k)]
               - 7 r mu F2(k,k')  + G2(k,k')  (k'/q+^2) [7 (k' + k mu) - 2 r (k + k' mu)].

    The brackets and q-+^2 are formed from k' - k and 1 -+ mu (pass them where they are known to full accuracy), as the
    device forms them."""
    k, kp = np.asarray(k, dtype=np.float64), np.asarray(kp, dtype=np.float64)
    mu, omm, opm = _pm(mu, one_minus_mu, one_plus_mu)
    d = k - kp
    qm2, qp2 = 2.0 * k * kp * omm + d * d, 2.0 * k * kp * opm + d * d
    s = k / kp + kp / k
    h, m2 = 0.5 * mu * s, mu * mu
    e2, g2 = (2.0 / 7.0) * m2 + 5.0 / 7.0, (4.0 / 7.0) * m2 + 3.0 / 7.0
    dk, r = kp - k, kp / k
    a = 7.0 * r * mu
    Am = 7.0 * (k * omm + dk) + 2.0 * r * (dk - kp * omm)
    Ap = 7.0 * (k * opm + dk) - 2.0 * r * (kp * opm - dk)
    return (((g2 - h) * (kp / qm2) * Am + a * (e2 - h)) + ((g2 + h) * (kp / qp2) * Ap - a * (e2 + h))) * (1.0 / 54.0)


def tree_trispectrum(ki, kj, mu, Pi, Pj, Pqm, Pqp, one_minus_mu=None, one_plus_mu=None):
    """The tree-level matter trispectrum T(k_i, -k_i, k_j, -k_j) at the cosine mu between k_i and k_j:

        12 F3s(k_i,-k_i,k_j) P_i^2 P_j + 12 F3s(k_j,-k_j,k_i) P_j^2 P_i + sum_{q = q-, q+} 4 P(q) [F2(q,k_j;k_i) P_j + F2(q,k_i;k_j) P_i]^2,

    q-+ = |k_i -+ k_j|, Pqm = P(q-), Pqp = P(q+).  The last sum is the general 2-2-1-1 sum - 4 times twelve permutations -
    with the four terms of vanishing internal momentum dropped; the F3 part is 6 times four permutations."""
    ki, kj = np.asarray(ki, dtype=np.float64), np.asarray(kj, dtype=np.float64)
    mu, omm, opm = _pm(mu, one_minus_mu, one_plus_mu)
    d = ki - kj
    qm, qp = np.sqrt(2.0 * ki * kj * omm + d * d), np.sqrt(2.0 * ki * kj * opm + d * d)
    um = F2(qm, kj, ki) * Pj + F2(qm, ki, kj) * Pi
    up = F2(qp, kj, ki) * Pj + F2(qp, ki, kj) * Pi
    F3 = F3s(ki, kj, mu, omm, opm) * (12.0 * Pi * Pi * Pj) + F3s(kj, ki, mu, omm, opm) * (12.0 * Pj * Pj * Pi)
    return 4.0 * Pqp * up * up + (4.0 * Pqm * um * um + F3)


def _pt_request(ks, Pzk, idx, frac, rule):
    """The checked host arrays of a request for the PT matrices: (ks, idx (nz, n) int32, frac, nz, nk, n).  Pzk may be a
    DeviceArray (nz, nk); it is then not read here."""
    _rule(rule)
    ks = np.ascontiguousarray(ks, dtype=np.float64).reshape(-1)
    nk = ks.size
    if nk < 2 or nk > MAX_NK or not np.all(np.isfinite(ks)) or np.any(ks <= 0) or np.any(np.diff(ks) <= 0):
        raise ValueError(f"ks must be positive and strictly increasing, 2 to {MAX_NK} points")
    shape = tuple(Pzk.shape) if isinstance(Pzk, nat.DeviceArray) else np.shape(Pzk)
    if len(shape) != 2 or shape[1] != nk or shape[0] < 1:
        raise ValueError(f"Pzk must have shape (nz, {nk}), got {shape}")
    nz = int(shape[0])
    if not isinstance(Pzk, nat.DeviceArray):
        P = np.asarray(Pzk, dtype=np.float64)
        if not np.all(np.isfinite(P)) or np.any(P <= 0):
            raise ValueError("Pzk must be finite and positive")
    idx = np.asarray(idx)
    if not np.issubdtype(idx.dtype, np.integer):
        raise ValueError("idx must be an integer array")
    if idx.ndim == 1:
        idx = np.broadcast_to(idx[None, :], (nz, idx.size))
    if idx.ndim != 2 or idx.shape[0] != nz:
        raise ValueError(f"idx must have shape (n,) or (nz, n) with nz = {nz}, got {idx.shape}")
    n = idx.shape[1]
    if not 1 <= n <= MAX_SAMPLES:
        raise ValueError(f"idx asks for {n} samples per redshift; the PT averages take 1 to {MAX_SAMPLES}")
    if idx.min() < 0 or idx.max() > nk - 1:
        raise ValueError(f"idx must lie in 0 .. nk - 1 = {nk - 1}, got {idx.min()} .. {idx.max()}")
    frac = np.zeros((nz, n)) if frac is None else np.broadcast_to(np.asarray(frac, dtype=np.float64), (nz, n))
    if not np.all((frac >= 0.0) & (frac <= 1.0)):
        raise ValueError("frac must lie in [0, 1]")
    if np.any((idx == nk - 1) & (frac != 0.0)):
        raise ValueError("idx = nk - 1 needs frac = 0 (there is no node to its right)")
    return ks, np.ascontiguousarray(idx, dtype=np.int32), np.ascontiguousarray(frac, dtype=np.float64), nz, nk, n


def sampled_plin(Pzk, idx, frac):
    """P_s of section 16: Pzk at the node where frac == 0, else (1 - f) P[idx] + f P[idx + 1]."""
    Pzk = np.asarray(Pzk, dtype=np.float64)
    z = np.arange(Pzk.shape[0])[:, None]
    Pl, Pr = Pzk[z, idx], Pzk[z, np.minimum(idx + 1, Pzk.shape[1] - 1)]
    return np.where(frac == 0.0, Pl, (1.0 - frac) * Pl + frac * np.where(frac == 0.0, 0.0, Pr))


def pt_averages(ks, Pzk, idx, frac, rule):
    """(Pbar, Bbar, Tbar), each (nz, n, n), on the host: the averages over the rule of P(q+), of the tree-level
    bispectrum B(k_i, k_j, -q+) and of tree_trispectrum at the samples (idx, frac) of the table Pzk (nz, nk) on ks.
    Each unordered pair is evaluated once, its sides ordered by (k, P), and mirrored: the matrices are bit-symmetric."""
    ks, idx, frac, nz, nk, n = _pt_request(ks, Pzk, idx, frac, rule)
    Pzk = np.asarray(Pzk, dtype=np.float64)
    ksamp, Psamp = bispec.sample_wavenumbers(ks, idx, frac), sampled_plin(Pzk, idx, frac)
    out = np.zeros((3, nz, n, n))
    i, j = np.triu_indices(n)
    for z in range(nz):
        k1, k2, P1, P2 = ksamp[z, i], ksamp[z, j], Psamp[z, i], Psamp[z, j]
        first = (k1 > k2) | ((k1 == k2) & (P1 >= P2))
        ka, kb = np.where(first, k1, k2), np.where(first, k2, k1)
        Pa, Pb = np.where(first, P1, P2), np.where(first, P2, P1)
        d = ka - kb
        acc = np.zeros((3, i.size))
        for mu, omm, opm, w in zip(rule.mu, rule.one_minus_mu, rule.one_plus_mu, rule.weights):
            qm, qp = np.sqrt(2.0 * ka * kb * omm + d * d), np.sqrt(2.0 * ka * kb * opm + d * d)
            Pm, Pp = plin_at(ks, Pzk[z], qm), plin_at(ks, Pzk[z], qp)
            acc[0] += w * Pp
            acc[1] += w * bispec.tree_bispectrum(ka, kb, qp, Pa, Pb, Pp)
            acc[2] += w * tree_trispectrum(ka, kb, mu, Pa, Pb, Pm, Pp, omm, opm)
        out[:, z, i, j] = acc
        out[:, z, j, i] = acc
    return out[0], out[1], out[2]


def _upload_rule(ctx, rule):
    return tuple(ctx.upload(a) for a in (rule.mu, rule.one_minus_mu, rule.one_plus_mu, rule.weights))


def pt_averages_device(ks, Pzk, idx, frac, rule, *, ctx=None):
    """pt_averages on the GPU (hmg_pt_averages): a DeviceArray (3, nz, n, n) = (Pbar, Bbar, Tbar).  Pzk may be a
    DeviceArray (nz, nk).  Everything that can be refused is, on the host, before any launch."""
    ks, idx, frac, nz, nk, n = _pt_request(ks, Pzk, idx, frac, rule)
    ctx = Pzk.ctx if ctx is None and isinstance(Pzk, nat.DeviceArray) else nat.context_or_default(ctx)
    d_ks, d_P = ctx.upload(ks), nat.as_device(ctx, Pzk)
    d_idx, d_frac = ctx.upload_int32(idx), ctx.upload(frac)
    d_rule = _upload_rule(ctx, rule)
    out = ctx.empty((3, nz, n, n))
    plane = 8 * nz * n * n
    ctx.call("hmg_pt_averages", nz=nz, nk=nk, n=n, nr=rule.nr, d_ks=d_ks.ptr, d_Pzk=d_P.ptr, d_idx=d_idx.ptr,
             d_frac=d_frac.ptr, d_mu=d_rule[0].ptr, d_omm=d_rule[1].ptr, d_opm=d_rule[2].ptr, d_w=d_rule[3].ptr,
             d_Pbar=out.ptr, d_Bbar=out.ptr + plane, d_Tbar=out.ptr + 2 * plane)
    return out


# ---------------------------------------------------------------------------------------- the terms, on the device
def _request(model, names, kindex, idx, frac, scale, damping, rule):
    """(records, tables, the 1-halo term's scale) of a request.  Every refusal happens here on the host, before any
    launch."""
    _rule(rule)
    recs = model._resolve(*names)
    hods = {r.name for r in recs if r.kind1 == "h"}
    if len(hods) > 1:
        raise NotImplementedError(
            f"trispectrum of {names!r}: two different HOD names ({sorted(hods)!r}) in one request need the cross moments "
            f"of the two HODs for their pair term, which the model does not carry")
    _same_lookups(recs, f"trispectrum of {names!r}")
    if model._nk > MAX_NK:
        raise ValueError(f"the model has {model._nk} wavenumbers; the PT averages take at most {MAX_NK}")
    tables = model._sample_tables(kindex, idx, frac, scale, False, MAX_SAMPLES, "the connected trispectrum")
    # the scale of the 1-halo term: section 15's, the damping folded in as trispectrum_device folds it
    scale1h = model._sample_tables(None, tables[0], tables[1], tables[2], damping, MAX_SAMPLES, "the connected trispectrum")[2]
    return recs, tables, scale1h


def connected_trispectrum_device(model, name, name2=None, name3=None, name4=None, kindex=None, damping=True, idx=None,
                                 frac=None, scale=None, rule=None, zweights=None, per_z=True):
    """(T, Tz) on the device: T (5, nz, n, n) = (T1h, T2h13, T2h22, T3h, T4h) of the spectra (name, name2) at +-k_i and
    (name3, name4; default: the first pair) at +-k_j, averaged over the angle between k_i and k_j with `rule` (default
    angle_rule(32, "2d")) - per_z=False: None - and Tz (5, n, n) = sum_z zweights[z] T[:, z], in z order, if zweights
    (nz,) is given, else None.

    Samples as for HaloModel.bispectrum_device (kindex, or idx / frac / scale tables; at most 256).  With J_x the 2-halo
    bracket of a leg, P the sampled linear spectrum, D = 1 - exp(-(k / kstar)^2) (damping=False: 1), sig = scale_i
    scale_j, w = wm nzm bh, I_{x,cd}(i;j) = sum_m w w_x(i) S_cd(j) and I_xy(i,j) = sum_m w w_x(i) w_y(j):

        T1h   = HaloModel.trispectrum_device's for the same tables, the same bits
        T2h13 = sig D_i D_j {P_i [J_a(i) I_{b,cd} + J_b(i) I_{a,cd}] + P_j [J_c(j) I_{d,ab} + J_d(j) I_{c,ab}]}
        T2h22 = sig (D_i D_j)^2 Pbar [I_ac I_bd + I_ad I_bc]
        T3h   = sig D_i D_j Bbar [I_ac J_b(i) J_d(j) + I_bd J_a(i) J_c(j) + I_ad J_b(i) J_c(j) + I_bc J_a(i) J_d(j)]
        T4h   = sig Tbar J_a(i) J_b(i) J_c(j) J_d(j)

    with (Pbar, Bbar, Tbar) of pt_averages.  Of twice the same HOD name I_xy uses the two-wavenumber pair term
    [(u_c(i) u_s(j) + u_s(i) u_c(j)) <NcNs> + <Ns(Ns-1)> u_s(i) u_s(j)] / ngal^2, which has no self-pairs.  Two different HOD
    names raise NotImplementedError.  The model carries no third factorial moment: three or four galaxies in one halo
    are formed as w_g S_gg and S_gg S_gg, section 15's convention.  Linear halo bias only."""
    name2 = name if name2 is None else name2
    name3, name4 = (name if name3 is None else name3), (name2 if name4 is None else name4)
    rule = angle_rule(32, "2d") if rule is None else rule
    recs, tables, scale1h = _request(model, (name, name2, name3, name4), kindex, idx, frac, scale, damping, rule)
    if zweights is not None:
        zweights = model._zweights(zweights)
    elif not per_z:
        raise ValueError("nothing asked for: per_z=False needs zweights")
    nz, n = model._nz, tables[0].shape[1]
    ctx = model._main(needs_aux=True)
    tr = [model._tracer(r, 1) for r in recs]
    d_idx, d_frac, d_scale = model._upload_tables(ctx, tables)
    d_scale1h = ctx.upload(scale1h)
    d_rule = _upload_rule(ctx, rule)
    d_g = ctx.upload(zweights) if zweights is not None else None
    T = ctx.empty((5, nz, n, n)) if per_z else None
    Tz = ctx.empty((5, n, n)) if zweights is not None else None
    ha, hb, hc, hd = (C.byref(t) for t in tr)
    ctx.call("hmg_trispectrum_connected", nz=nz, nm=model._nm, nk=model._nk, n=n, nr=rule.nr, h_a=ha, h_b=hb, h_c=hc,
             h_d=hd, **model._model_block("hmg_trispectrum_connected"),
             kstar=float(model.p["kstar_damping"]) if damping else 0.0, d_idx=d_idx.ptr, d_frac=d_frac.ptr,
             d_scale=d_scale.ptr, d_scale1h=d_scale1h.ptr, d_mu=d_rule[0].ptr, d_omm=d_rule[1].ptr, d_opm=d_rule[2].ptr,
             d_w=d_rule[3].ptr, d_zweights=nat.ptr(d_g), d_T=nat.ptr(T), d_Tz=nat.ptr(Tz))
    model._sync_point()
    return T, Tz


def _terms(T):
    """The dict of a (5, ...) host array: the five terms and "total", their sum in this order."""
    out = dict(zip(TERMS, T))
    out["total"] = (((T[0] + T[1]) + T[2]) + T[3]) + T[4]
    return out


def get_trispectrum(model, name, name2=None, name3=None, name4=None, kindex=None, damping=True, rule=None):
    """The angle-averaged halo-model trispectrum of two spectra at the nodes ks[kindex] (default: all; at most 256): a
    dict of six (nz, n, n) arrays, "1h", "2h13", "2h22", "3h", "4h" and "total" (their sum in this order); see
    connected_trispectrum_device.  rule defaults to angle_rule(32, "2d"); for the covariance of P(k) in shells pass
    angle_rule(n, "3d")."""
    T, _ = connected_trispectrum_device(model, name, name2, name3, name4, kindex=kindex, damping=damping, rule=rule)
    return _terms(T.numpy())


def limber_tables(model, ells, W1=1, W2=1, W3=1, W4=1, fsky=1.0):
    """The host tables of cl_cov_connected, cl_cov_1halo's: (idx, frac, g)."""
    ells = np.asarray(ells, dtype=np.float64).reshape(-1)
    zs = np.asarray(model.zs, dtype=np.float64).reshape(-1)
    if zs.size < 2:
        raise ValueError("cl_cov_connected integrates over the model's redshifts: it needs at least two")
    if not fsky > 0:
        raise ValueError(f"fsky must be positive, got {fsky!r}")
    chis = np.asarray(model.comoving_radial_distance(zs), dtype=np.float64).reshape(-1)
    hzs = np.asarray(model.h_of_z(zs), dtype=np.float64).reshape(-1)
    idx, frac = limber_samples(ells, chis, model.ks, zs=zs)
    g = trapz_weights(zs) * hzs / chis ** 6 / (4.0 * np.pi * fsky)
    for W in (W1, W2, W3, W4):
        g = g * np.broadcast_to(np.asarray(W, dtype=np.float64), zs.shape)
    return idx, frac, g


def cl_cov_connected(model, ells, name, name2=None, name3=None, name4=None, W1=1, W2=1, W3=1, W4=1, fsky=1.0,
                     damping=True, rule=None):
    """The connected (non-Gaussian, in-survey) covariance of two Limber spectra C_l^{ab} and C_l'^{cd} term by term: a dict
    of (n_l, n_l') matrices "1h", "2h" (the sum of the 3+1 and 2+2 terms), "3h", "4h" and "total" (1h + 2h + 3h + 4h),

        Cov(l, l') = 1 / (4 pi fsky) trapz_z[ H W1 W2 W3 W4 / chi^6  T(z; (l + 1/2)/chi, (l' + 1/2)/chi) ],

    with cov.cl_cov_1halo's measure and cov.limber_samples; "1h" is exactly cl_cov_1halo's.  rule defaults to
    angle_rule(32, "2d"): the average over the angle between l and l' in the plane of the sky.  The z sum is taken on the
    device, in z order.  Warning, as for cl_cov_1halo: the super-sample term cl_cov_ssc has another
    Limber measure (H^3 sigma_b / chi^4) and is not to be added to this without that in mind; nothing here sums them."""
    idx, frac, g = limber_tables(model, ells, W1, W2, W3, W4, fsky)
    if idx.shape[1] == 0:
        return {k: np.empty((0, 0)) for k in ("1h", "2h", "3h", "4h", "total")}
    _, Tz = connected_trispectrum_device(model, name, name2, name3, name4, damping=damping, idx=idx, frac=frac, rule=rule,
                                         zweights=g, per_z=False)
    Tz = Tz.numpy()
    two = Tz[1] + Tz[2]
    return {"1h": Tz[0], "2h": two, "3h": Tz[3], "4h": Tz[4], "total": ((Tz[0] + two) + Tz[3]) + Tz[4]}
