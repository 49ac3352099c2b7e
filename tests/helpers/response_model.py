"""Numpy restatement of the response of halo-model spectra to a long-wavelength density mode and of the super-sample
covariance from a HaloModel's host arrays alone: uk_profiles / pk_profiles / hods entries, nzm,
bh, ms, ks, Pzk.  The sampled square term is trispectrum_model's, the leg quantities (J, the HOD bias sum, P_s, k_s, D_s)
are bispectrum_model's; what a comparison with this tests is the two new mass sums, the epilogue and the contraction.

    R[p,z,s] = scale [ (47/21 - n_s/3) P2h + D I1 - (beta_a + beta_b) (P2h + D A1) ]
    A1 = sum_m wm nzm S_ab,  I1 = sum_m wm nzm bh S_ab,  P2h = P_s J_a J_b
    Cov[p,i,q,j] = sum_z g[z] r[p,z,i] r[q,z,j],  r = zscale R

Every quantity is a pair (value, tol).  tol bounds |device - restatement| when both follow the contract; it is derived
from rounding counts, not measured (EPS = 2^-52):

* A1, I1: (nm + 40) EPS A, A the same sum over absolute values (bispectrum_model.mass_sum: the count of section 16);
* J, beta, P_s: bispectrum_model's;  n_s: 3 EPS (|left| + |right|) of the two table entries it interpolates;
* a product: sum_i tol_i prod_{j != i} |x_j| plus one EPS of prod |x_j| per multiplication; a sum: the sum of the tols
  plus one EPS of the absolute sum per addition (bispectrum_model.prod / add);
* D_s, k_s, the scales, zscale and g are exact: host and device hold the same bits;
* Cov: the z sum of the products r r with their propagated tols, weighted with |g|, plus nz 2^-53 sum_z |g r r|
  (trispectrum_model.zsum's rule)."""
import numpy as np

from hmvec_amd.quadrature import trapz_weights

import bispectrum_model as bm
import trispectrum_model as tm

EPS = tm.EPS


def dlnp(h):
    """The slope table of the contract: np.gradient(log Pzk, log ks) along k."""
    return np.gradient(np.log(h.Pzk), np.log(h.ks), axis=-1)


def slope(h, idx, frac):
    """(n_s, tol) at the (nz, n) samples: the linear interpolant of dlnp, node idx + 1 not read where frac == 0."""
    dl = dlnp(h)
    z = np.arange(dl.shape[0])[:, None]
    left = dl[z, idx]
    right = np.where(frac == 0.0, 0.0, dl[z, np.minimum(idx + 1, h.ks.size - 1)])
    val = np.where(frac == 0.0, left, (1.0 - frac) * left + frac * right)
    return val, 3 * EPS * (np.abs(left) + np.abs(right))


def neg(x):
    return -x[0], x[1]


def legs(h, names, idx, frac, damping):
    """Per distinct name the leg quantities of section 16 - J (nz, n) and beta (nz,), each (value, tol) - and the shared
    (P, k, D): bispectrum_model.bispectrum of the triple (name, name, name) at one dummy triangle carries them all."""
    out, shared = {}, None
    tri = np.zeros((1, 3), dtype=int)
    for nm_ in dict.fromkeys(names):
        d = bm.bispectrum(h, (nm_, nm_, nm_), tri, idx=idx, frac=frac, damping=damping)
        J = (d["J"][0][0], d["J"][1][0])
        if bm.kind(h, nm_) == "h":
            beta = (d["b"][0][0], d["b"][1][0])
        else:
            beta = bm.exact(np.zeros(h.nzm.shape[0]))
        out[nm_] = (J, beta)
        shared = (d["P"], d["k"], d["D"])
    return out, shared


def response(h, pairs, kindex=None, idx=None, frac=None, scale=None, damping=True):
    """A dict of (value, tol) pairs, each stacked over the pairs: R, A1, I1, P2h (np, nz, n), beta_sum (np, nz), and the
    shared ns, P (nz, n) and exact k, D, scale (nz, n)."""
    pairs = [(a, a if b is None else b) for a, b in pairs]
    idx, frac, scale = tm.tables(h, kindex=kindex, idx=idx, frac=frac, scale=scale, damping=False)
    idx, frac, scale = np.asarray(idx), np.asarray(frac, dtype=float), np.asarray(scale, dtype=float)
    leg, (P, k, D) = legs(h, [nm_ for p in pairs for nm_ in p], idx, frac, damping)
    ns = slope(h, idx, frac)
    growth = bm.add(bm.exact(np.full(idx.shape, 47.0 / 21.0)), (-ns[0] / 3.0, ns[1] / 3.0 + EPS * np.abs(ns[0] / 3.0)))
    wn = trapz_weights(h.ms)[None, :] * h.nzm
    wnb = wn * h.bh
    one = np.ones(idx.shape)
    out = {key: [] for key in ("R", "A1", "I1", "P2h", "beta_sum")}
    for a, b in pairs:
        s = tm.sampled(tm.square_term(h, a, b), idx, frac, one)
        A1, I1 = bm.mass_sum(wn, s), bm.mass_sum(wnb, s)
        (Ja, ba), (Jb, bb) = leg[a], leg[b]
        P2h = bm.prod(P, Ja, Jb)
        bsum = bm.add(ba, bb)
        bcol = (bsum[0][:, None], bsum[1][:, None])
        mean = bm.prod(bcol, bm.add(P2h, bm.prod(bm.exact(D), A1)))
        bracket = bm.add(bm.prod(growth, P2h), bm.prod(bm.exact(D), I1), neg(mean))
        for key, v in (("R", bm.prod(bm.exact(scale), bracket)), ("A1", A1), ("I1", I1), ("P2h", P2h), ("beta_sum", bsum)):
            out[key].append(v)
    res = {key: tuple(np.stack([np.broadcast_to(v[j], v[0].shape) for v in vs]) for j in (0, 1)) for key, vs in out.items()}
    res.update(ns=ns, P=P, k=k, D=D, scale=scale)
    return res


def ssc(R, g, zscale=None):
    """(Cov, tol), each (np, n, np, n), of R = (value, tol) (np, nz, n), the z weights g (nz,) and zscale (np, nz)."""
    g = np.asarray(g, dtype=float)
    val, tol = R
    npairs, nz, n = val.shape
    if zscale is not None:
        val, tol = bm.prod(bm.exact(np.asarray(zscale, dtype=float)[:, :, None]), (val, tol))
    r = val.transpose(0, 2, 1).reshape(npairs * n, nz)
    t = np.broadcast_to(tol, val.shape).transpose(0, 2, 1).reshape(npairs * n, nz)
    ag, ar = np.abs(g), np.abs(r)
    cov = np.einsum("z,az,bz->ab", g, r, r)
    absum = np.einsum("z,az,bz->ab", ag, ar, ar)
    ctol = (np.einsum("z,az,bz->ab", ag, t, ar) + np.einsum("z,az,bz->ab", ag, ar, t) + EPS * absum
            + nz * 0.5 * EPS * absum)
    shape = (npairs, n, npairs, n)
    return cov.reshape(shape), ctol.reshape(shape)
