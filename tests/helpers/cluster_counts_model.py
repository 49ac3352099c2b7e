"""The numpy restatement of the cluster counts (hmvec_amd/csrc/kernels/clusters.hpp) and the derived
tolerance of its comparison with the device.

Same operations in the same order as the kernel, with scipy.special.erfc and np.exp / np.log where the device calls its
library:

  1. a pair p = tau G + g of a halo (gaussian) or a tile tau (none) belongs to lane p % 64; a lane adds its terms in
     ascending p, one chain per bin;
  2. the 64 lanes are summed by a balanced tree of depth 6 (wave_tree): S_a[z, m];
  3. the halos of a 64-mass tile are summed by the same tree, halos outside the window as 0;
  4. the tiles are added in ascending order.

The tolerance.  Every term of every sum is >= 0 (up to the rounding of one difference), so the sums are well conditioned
and the bound is a sum of per-term bounds plus the depth of the reduction times the sum.  With u = 2^-53, for an edge j
of a term: E_j = erfc(|u_j|) (the value the code evaluates), g_j = 2 / sqrt(pi) exp(-u_j^2) the Gaussian slope, and
  gaussian   M_j = E_j + g_j (|u_j| + q / sqrt 2)              library error of erfc and of q = exp(x), one unit each
             X_j = g_j (2 |u_j| + q / sqrt 2 (|sg t| + |mu + sg t| + |x|))   the IEEE roundings of x, e - q and the scaling
  none       M_j = E_j + g_j (|u_j| + scale |ln e_j|)          library error of erfc and of ln e_j
             X_j = g_j (4 |u_j| + scale |xi|)                  the roundings of xi, ln e - xi and the three of the scale
a term's error is at most  wt u (c (1/2 sum_{j = a, a+1} M_j + |P_a|) + 1/2 sum_j X_j).  The |P_a| stands for the
roundings of the difference and of the two products (3 u |P_a|) and of 2 - E where it is formed: that one is at most
u (2 - E) <= u max(3 E, 4 |P_a|), since 2 - E is only paired with a smaller tail (E < 1/2 gives |P_a| > 1/2); these small
constants are part of c.  c is MEASURED, not assumed: the worst |P_a - exact| / (u (1/2 sum_j M_j + |P_a|)) against 40-digit mpmath over the
fixed set CE_Q x CE_EDGES, taken through the public interface with T = G = 1, area = 1 (tests/test_gpu_cluster_counts.py
for the device, tests/test_cluster_counts_cpu.py for this restatement); the gates use twice the measured values.  Device
and restatement are each within their bound of the exact value, so they differ by at most the sum of the two.
"""
import numpy as np
from scipy.special import erfc

U = 2.0 ** -53
SQRT1_2 = 0.70710678118654752440
SQRT2 = 1.41421356237309504880
TINY = np.finfo(np.float64).tiny      # per term: a tail below the normal range has no relative accuracy (it may be 0)

# The fixed argument set of the measurement of c.  q <= 0 cannot be reached through the public interface (q = exp(.) > 0):
# those 20 points of linspace(-2, 40, 400) are left out.  The erfc arguments they would give, (e - q) / sqrt 2 with e - q
# in [0, 2], [5, 7], [6, 8], [8, 10] and [38, 40], all occur among the points kept (the edge 8 at q in [0, 8], ...).
CE_Q = np.linspace(-2.0, 40.0, 400)
CE_Q = CE_Q[CE_Q > 0.0]
CE_EDGES = np.array([-np.inf, 0.0, 5.0, 5.001, 6.0, 8.0, 38.0, np.inf])
# measured worst c (see above) and the gates built on them: twice the measured value
CE_DEVICE_MEASURED = 1.41         # the device's erfc and exp (MI355X, ROCm's device library)
CE_NUMPY_MEASURED = 1.68          # scipy.special.erfc and np.exp
CE_DEVICE = 2.0 * CE_DEVICE_MEASURED
CE_NUMPY = 2.0 * CE_NUMPY_MEASURED


def wave_tree(x):
    """The sum over the last axis (64 values) in wave_sum's order: a balanced binary tree of neighbours."""
    assert x.shape[-1] == 64
    for _ in range(6):
        x = x[..., 0::2] + x[..., 1::2]
    return x[..., 0]


def _terms(mu, sg, lnnoise, area, t, w, kind):
    """Per pair, for halos mu, sg of shape (H,): c (the value the edges are compared with), wt, scale and the relative
    rounding of c; arrays (H, count), count = T G (gaussian) or T (none)."""
    mu, sg = mu[:, None], sg[:, None]
    if kind == 0:
        T, G = lnnoise.size, t.size
        tt, ww = np.tile(t, T)[None, :], np.tile(w, T)[None, :]
        ln, ar = np.repeat(lnnoise, G)[None, :], np.repeat(area, G)[None, :]
        s1 = sg * tt
        s2 = mu + s1
        x = s2 - ln
        c = np.exp(x)
        wt = np.broadcast_to(ar * ww, c.shape)
        scale = np.full_like(c, SQRT1_2)
        slack = c * SQRT1_2 * (np.abs(s1) + np.abs(s2) + np.abs(x))
        lib = c * SQRT1_2
        nround = 2.0
    else:
        c = mu - lnnoise[None, :]
        wt = np.broadcast_to(area[None, :], c.shape)
        scale = np.broadcast_to(1.0 / (SQRT2 * sg), c.shape)
        slack = scale * np.abs(c)
        lib = None
        nround = 4.0
    return c, wt, scale, slack, lib, nround


def selection(lnobs, sigln, lnnoise, area, t, w, edges, kind, window=None, bound=False):
    """S (nz, nm, nq) of the restatement, zero outside the window (m_lo, m_hi); with bound=True also (Mb, Xb), the sums
    of wt (1/2 sum_j M_j + |P|) and wt / 2 sum_j X_j of every element (see the module's text)."""
    nz, nm = lnobs.shape
    nq = edges.size - 1
    m_lo, m_hi = (0, nm) if window is None else window
    S = np.zeros((nz, nm, nq))
    Mb, Xb = np.zeros_like(S), np.zeros_like(S)
    with np.errstate(divide="ignore"):
        ed = edges if kind == 0 else np.log(edges)
    for z in range(nz):
        c, wt, scale, slack, lib, nround = _terms(lnobs[z, m_lo:m_hi], sigln[z, m_lo:m_hi], lnnoise, area, t, w, kind)
        H, count = c.shape
        rounds = -(-count // 64)
        pad = rounds * 64 - count

        def lanes(a, fill=0.0):       # (H, count) -> (rounds, H, 64); a missing pair has the weight 0 (its term is +0)
            return np.moveaxis(np.pad(a, ((0, 0), (0, pad)), constant_values=fill).reshape(H, rounds, 64), 1, 0)

        c, wt, scale, slack = lanes(c), lanes(wt), lanes(scale, 1.0), lanes(slack)
        lib = None if lib is None else lanes(lib)
        acc = np.zeros((H, 64, nq))
        am, ax = np.zeros_like(acc), np.zeros_like(acc)
        with np.errstate(invalid="ignore", over="ignore"):
            for r in range(rounds):
                d = ed[None, None, :] - c[r][..., None]                 # (H, 64, nq + 1)
                u = d * scale[r][..., None]
                E = erfc(np.abs(u))
                neg = u < 0.0
                dp, Ep, negp = d[..., :-1], E[..., :-1], neg[..., :-1]
                dn, En, negn = d[..., 1:], E[..., 1:], neg[..., 1:]
                flip = dp + dn < 0.0
                hi = np.where(flip, np.where(negn, En, 2.0 - En), np.where(negp, 2.0 - Ep, Ep))
                lo = np.where(flip, np.where(negp, Ep, 2.0 - Ep), np.where(negn, 2.0 - En, En))
                P = 0.5 * (hi - lo)
                acc = acc + wt[r][..., None] * P
                if bound:
                    fin = np.isfinite(u)
                    au = np.where(fin, np.abs(u), 0.0)
                    g = np.where(fin, 2.0 / np.sqrt(np.pi) * np.exp(-au * au), 0.0)
                    if kind == 0:
                        Mj = E + g * (au + lib[r][..., None])
                    else:
                        Mj = E + g * (au + scale[r][..., None] * np.where(fin, np.abs(ed)[None, None, :], 0.0))
                    Xj = g * (nround * au + slack[r][..., None])
                    am = am + wt[r][..., None] * (0.5 * (Mj[..., :-1] + Mj[..., 1:]) + np.abs(P))
                    ax = ax + 0.5 * wt[r][..., None] * (Xj[..., :-1] + Xj[..., 1:])
        S[z, m_lo:m_hi] = wave_tree(np.moveaxis(acc, 1, -1))
        if bound:
            Mb[z, m_lo:m_hi], Xb[z, m_lo:m_hi] = am.sum(axis=1), ax.sum(axis=1)
    return (S, Mb, Xb) if bound else S


def mass_sums(S, wm, nzm, bh, window=None):
    """(n, bn) (nz, nq) from S (nz, nm, nq): 64-mass tiles by wave_tree, halos outside the window as 0, then the tiles in
    ascending order; n's term is wm (nzm S), bn's that times bh."""
    nz, nm, nq = S.shape
    m_lo, m_hi = (0, nm) if window is None else window
    ntile = -(-nm // 64)
    tn = np.zeros((nz, ntile * 64, nq))
    inside = np.zeros(nm, dtype=bool)
    inside[m_lo:m_hi] = True
    term = wm[None, :, None] * (nzm[:, :, None] * S)
    tn[:, :nm] = np.where(inside[None, :, None], term, 0.0)
    tb = np.zeros_like(tn)
    tb[:, :nm] = tn[:, :nm] * bh[:, :, None]
    n, bn = np.zeros((nz, nq)), np.zeros((nz, nq))
    for tile in range(ntile):
        n = n + wave_tree(np.moveaxis(tn[:, tile * 64:(tile + 1) * 64], 1, -1))
        bn = bn + wave_tree(np.moveaxis(tb[:, tile * 64:(tile + 1) * 64], 1, -1))
    return n, bn


def depth_selection(count):
    """Additions on the longest chain behind one S: a lane's chain, the tree, and the two products of a term."""
    return -(-int(count) // 64) + 6 + 2


def tolerances(S, Mb, Xb, wm, nzm, bh, count, c, sides=2, window=None, area_max=1.0):
    """(tol_S, tol_n, tol_bn): the bound on |device - restatement| (sides = 2: each is within its own bound of the exact
    value, c = CE_DEVICE + CE_NUMPY) or on |device - exact| (sides = 1, c = CE_DEVICE)."""
    tol_S = U * (c * Mb + sides * Xb + sides * depth_selection(count) * np.abs(S)) + sides * count * TINY * area_max
    nm = S.shape[1]
    ntile = -(-nm // 64)
    n, bn = mass_sums(np.abs(S), wm, nzm, np.abs(bh), window)
    tn, tbn = mass_sums(tol_S, wm, nzm, np.abs(bh), window)
    return tol_S, tn + sides * U * (2 + 6 + ntile) * n, tbn + sides * U * (3 + 6 + ntile) * bn


# ---------------------------------------------------------------- 40-digit references
def p_exact(q, ea, eb, scale=SQRT1_2):
    """P_a(q) = 1/2 [erfc((ea - q) scale) - erfc((eb - q) scale)] with mpmath, formed from the tails."""
    import mpmath as mp
    mp.mp.dps = 40
    q, scale = mp.mpf(q), mp.mpf(scale)

    def tail(e, sign):          # erfc(sign (e - q) scale)
        if np.isinf(e):
            return mp.mpf(0) if sign * e > 0 else mp.mpf(2)
        return mp.erfc(sign * (mp.mpf(e) - q) * scale)

    mid = (0.0 if np.isinf(ea) and np.isinf(eb) else ea + eb - 2.0 * float(q))
    if mid < 0:
        return (tail(eb, -1) - tail(ea, -1)) / 2
    return (tail(ea, 1) - tail(eb, 1)) / 2


def unit_error(q, ea, eb, P):
    """u (1/2 sum_j M_j + |P|) of a gaussian term of weight 1 at q: the denominator of the measurement of c."""
    out = 2.0 * abs(P)
    for e in (ea, eb):
        if np.isinf(e):
            continue
        a = abs(e - q) * SQRT1_2
        out += erfc(a) + 2.0 / np.sqrt(np.pi) * np.exp(-a * a) * (a + q * SQRT1_2)
    return 0.5 * U * out + TINY             # (below the normal range a tail may be flushed: 0 is then the answer)


def measure_c(lnq, P):
    """The worst |P - exact| / unit_error over the set: lnq (n,) the doubles ln q given as lnobs (q = exp(lnq) exactly, in
    mpmath), P (n, nq) the result at the edges CE_EDGES."""
    import mpmath as mp
    mp.mp.dps = 40
    worst, at = 0.0, None
    for i, lq in enumerate(lnq):
        q = mp.exp(mp.mpf(float(lq)))
        for a in range(CE_EDGES.size - 1):
            ea, eb = CE_EDGES[a], CE_EDGES[a + 1]
            exact = p_exact(q, ea, eb)
            err = abs(mp.mpf(float(P[i, a])) - exact)
            r = float(err / mp.mpf(unit_error(float(q), ea, eb, float(exact))))
            if r > worst:
                worst, at = r, (float(q), a)
    return worst, at


# ---------------------------------------------------------------- the z sums and the covariance, plainly
def counts(n, zw):
    return np.array([[np.sum(zw[i] * n[:, a]) for a in range(n.shape[1])] for i in range(zw.shape[0])])


def counts_cov(N, bn, tw, chis, hzs, sigma_b):
    nzb, nq = N.shape
    poisson, sample = np.zeros((nzb, nq, nzb, nq)), np.zeros((nzb, nq, nzb, nq))
    for i in range(nzb):
        for a in range(nq):
            poisson[i, a, i, a] = N[i, a]
            for b in range(nq):
                sample[i, a, i, b] = np.sum(tw[i] * chis ** 4 * sigma_b / hzs * bn[:, a] * bn[:, b])
    return poisson, sample


def cl_cov(bn, R, tw, hzs, sigma_b, zscale):
    nzb, nq, npairs, nl = tw.shape[0], bn.shape[1], R.shape[0], R.shape[2]
    out = np.zeros((nzb, nq, npairs, nl))
    for i in range(nzb):
        for a in range(nq):
            for p in range(npairs):
                out[i, a, p] = np.sum((tw[i] * hzs * sigma_b * zscale[p] * bn[:, a])[:, None] * R[p], axis=0)
    return out
