"""Numpy restatement of the HOD parameter ensemble from host arrays alone: nzm, bh (nz, nm), ms, ks,
Pzk (nz, nk), the satellite and the matter tensor (nz, nm, nk) and the occupation numbers of the S sets, each (S, nz, nm)
- from oracle.hmref.hod_occupations on the CPU, from the device's own (bit-checked) arrays on the GPU.

    w = wm nzm,  ngal = sum_m w (Nc + Ns),  bg = sum_m w bh (Nc + Ns) / ngal
    G = sum_m w (2 NcNs u_s + NsNsm1 u_s^2) / ngal^2          P1h_gg = D G
    X = sum_m w (m/rho_m0) u_m (Nc + Ns u_s) / ngal           P1h_gm = D X
    I = sum_m w bh (Nc + Ns u_s) / ngal,  C = sum_m w bh (Nc + Ns) / ngal,  J_g = (I + bg) - C
    I_m = sum_m w bh (m/rho_m0) u_m,  C_m = sum_m w bh m/rho_m0,  J_m = (I_m + 1) - C_m
    P2h_gg = Pzk J_g^2,  P2h_gm = Pzk J_g J_m

Every quantity is a pair (value, tol).  tol bounds |device - restatement| when both follow the contract; it is derived
from rounding counts, never from a device result (EPS = 2^-52):

* a mass sum: (nm + TERM_ROUNDINGS) EPS A, A the same sum over absolute values.  Each side adds nm terms in some order
  (half an EPS of A per addition and side) and a term carries at most eight roundings on either side - the weight, m/rho
  and its product, the products with the tensors, Ns u_s + Nc, the accumulate - counted at a full EPS each for both;
* 1 / ngal: its sum's tol over ngal^2 plus one EPS; products and sums propagate with bispectrum_model.prod / add;
* P_lin at a node is exact, and so is the damping factor against the ensemble itself (hmvec_amd.bispectrum.damping: host
  and device hold the same bits).  Against get_power_1halo, whose kernel evaluates 1 - exp(-(k/kstar)^2) with the
  device's exp, damping_tol is added: six ulp of exp(-x) - three of bispectrum.damping's stated bound, one of the
  library's exp, two roundings of its argument, each of which moves exp(-x) by x EPS <= EPS where D < 1 - plus one of D."""
import numpy as np

from hmvec_amd import bispectrum as bs
from hmvec_amd.quadrature import trapz_weights

import bispectrum_model as bm

EPS = bm.EPS
TERM_ROUNDINGS = 16
PLANES = ("gg_1h", "gg_2h", "gm_1h", "gm_2h")
PARTS = ("G", "X", "I")


def mass_sum(w, term):
    """sum over the mass axis (second to last of w's broadcast shape) and its tol."""
    t = w * term
    nm = t.shape[-2]
    return t.sum(axis=-2), (nm + TERM_ROUNDINGS) * EPS * np.abs(t).sum(axis=-2)


def inverse(x):
    v, t = x
    return 1.0 / v, t / (v * v) + EPS / np.abs(v)


def neg(x):
    return -x[0], x[1]


def damping_tol(ks, kstar):
    """What the damping factor of get_power_1halo's kernel may differ by from bispectrum.damping's."""
    x = (ks / kstar) ** 2
    return 6 * EPS * np.exp(-x) + EPS * bs.damping(ks, kstar)


def ensemble(nzm, bh, ms, ks, Pzk, rho_m0, us, um, occ, kstar, kindex=None, damping=True):
    """A dict of (value, tol) pairs: the planes gg_1h, gg_2h, gm_1h, gm_2h and the parts G, X, I, each (S, nz, n); ngal and
    bg (S, nz); D (n,) with a zero tol.  occ: Nc, Ns, NsNsm1, NcNs, each (S, nz, nm)."""
    kindex = np.arange(ks.size) if kindex is None else np.asarray(kindex)
    Nc, Ns, NN, CN = (np.asarray(occ[k], dtype=float)[..., None] for k in ("Nc", "Ns", "NsNsm1", "NcNs"))
    w = (trapz_weights(ms)[None, :] * nzm)[None, :, :, None]                # (1, nz, nm, 1)
    wb = w * bh[None, :, :, None]
    r = (ms / rho_m0)[None, None, :, None]
    u_s, u_m = us[None, :, :, kindex], um[None, :, :, kindex]
    one = np.ones((1, 1, 1, 1))
    n_ = mass_sum(w, (Nc + Ns) * one)                                       # (S, nz, 1)
    inv = inverse(n_)
    B = mass_sum(wb, (Nc + Ns) * one)
    bg = bm.prod(B, inv)
    C = bm.prod(B, inv)
    G = bm.prod(mass_sum(w, 2.0 * CN * u_s + NN * u_s * u_s), inv, inv)
    X = bm.prod(mass_sum(w, r * u_m * (Nc + Ns * u_s)), inv)
    I = bm.prod(mass_sum(wb, Nc + Ns * u_s), inv)
    Jg = bm.add(I, bg, neg(C))
    Jm = bm.add(mass_sum(wb, r * u_m), bm.exact(np.ones(())), neg(mass_sum(wb, r * one)))
    D = bs.damping(ks[kindex], kstar) if damping else np.ones(kindex.size)
    De = bm.exact(D[None, None, :])
    P = bm.exact(Pzk[None, :, kindex])
    out = dict(G=G, X=X, I=I, D=(D, np.zeros_like(D)))
    out["ngal"] = (n_[0][..., 0], n_[1][..., 0])
    out["bg"] = (bg[0][..., 0], bg[1][..., 0])
    out["gg_1h"], out["gm_1h"] = bm.prod(De, G), bm.prod(De, X)
    out["gg_2h"], out["gm_2h"] = bm.prod(P, Jg, Jg), bm.prod(P, Jg, Jm)
    return {k: (np.asarray(v[0]), np.broadcast_to(v[1], np.shape(v[0]))) for k, v in out.items()}


def with_damping_tol(ref, ks, kstar, kindex=None):
    """The 1-halo planes of `ref` with the tol of a comparison against get_power_1halo's own damping factor."""
    kindex = np.arange(ks.size) if kindex is None else np.asarray(kindex)
    dt = damping_tol(ks[kindex], kstar)[None, None, :]
    out = dict(ref)
    for key, part in (("gg_1h", "G"), ("gm_1h", "X")):
        out[key] = (ref[key][0], ref[key][1] + dt * np.abs(ref[part][0]))
    return out


def from_model(h, sets_occ, satellite="nfw", matter=None, kindex=None, damping=True):
    """ensemble() on a HaloModel's own host arrays."""
    matter = satellite if matter is None else matter
    return ensemble(h.nzm, h.bh, h.ms, h.ks, h.Pzk, float(h.rho_matter_z(0)[0]), h.uk_profiles[satellite],
                    h.uk_profiles[matter], sets_occ, h.p["kstar_damping"], kindex=kindex, damping=damping)
