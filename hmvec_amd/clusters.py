"""Cluster number counts N(z, q) and their covariance: how many halos of the model's mass function
a survey finds, in bins of redshift and of detection significance q.

The true observable O of a halo (z, m) is log-normal, ln O = lnobs[z, m] + sigma_ln t with t ~ N(0, 1); tile tau of the
survey has the solid angle area[tau] [sr] and the noise noise[tau]; the measured significance is
q = O / noise[tau] + N(0, 1) ("gaussian") or O / noise[tau] ("none").  With P_a the probability of bin [e_a, e_a+1),

    S_a[z, m] = sum_tau area[tau] sum_g w_g P_a(exp(lnobs + sigma_ln t_g - ln noise[tau])),
    n_a[z]    = sum_m wm[m] nzm[z, m] S_a[z, m],         bn_a[z] = sum_m wm[m] nzm[z, m] bh[z, m] S_a[z, m],
    N[i, a]   = sum_z zw[i, z] n_a[z],                   zw[i] = trapz_weights(zs of bin i) chi^2 / H.

``cluster_selection`` is the checked record of a survey, ``scatter_rule`` the default rule (t_g, w_g) for the scatter.
The selection and the mass sums are one native call (``hmg_cluster_selection``, csrc/kernels/clusters.hpp); the z sums
and the covariance algebra act on nz nq numbers and are host numpy.  ``cluster_abundance_device``,
``get_cluster_abundance``, ``get_cluster_counts``, ``cluster_counts_cov`` and ``cluster_cl_cov`` are functions of the
model, as section 23's ``angular_cov(model, ...)`` and section 24's ``get_xi_multipoles(model, ...)`` are, not methods:
the mixin list and the attribute surface of the class are recorded fixtures that this section leaves as they are.  Nothing
is cached on the model; cached spectra stay valid.
"""
import numpy as np

from . import _native as nat
from . import cov as _cov
from .functions import mdelta_from_mdelta
from .quadrature import trapz_weights

__all__ = ["cluster_selection", "scatter_rule", "ClusterSelection", "cluster_abundance_device", "get_cluster_abundance",
           "get_cluster_counts", "cluster_counts_cov", "cluster_cl_cov", "sz_lnobs", "powerlaw_lnobs", "z_bin_weights",
           "counts_from_abundance", "counts_cov_from_abundance", "cl_cov_from_abundance", "NOISE_MODELS", "SZ_DEFAULTS",
           "POWERLAW_DEFAULTS", "BINS_PER_LAUNCH"]

NOISE_MODELS = ("gaussian", "none")          # the native call's `kind`, by position
BINS_PER_LAUNCH = 8                          # csrc/kernels/clusters.hpp: CL_BINS (the entry point walks the chunks)
SZ_DEFAULTS = dict(C0=0.0, mpivot=3.0e14, bias=1.0, delta=500.0)        # the defaults of sz_lnobs (masses in Msun)
POWERLAW_DEFAULTS = dict(C=0.0, mpivot=3.0e14, zpivot=0.0)              # the defaults of powerlaw_lnobs


# ---------------------------------------------------------------- the survey
def scatter_rule(G=64, tmax=7.0):
    """(t, w): the G-node trapezoid rule for the unit normal on [-tmax, tmax], w_g = phi(t_g) h normalised to sum 1.  The
    default, 64 nodes to 7 sigma, integrates the selection to 1e-11 (32 nodes: 3e-5; Gauss-Hermite with 64 nodes: 6e-6 -
    the integrand has the width of the measurement noise, not of the scatter).  G = 1: (0, 1), no
    scatter."""
    if isinstance(G, bool) or not isinstance(G, (int, np.integer)) or G < 1:
        raise ValueError(f"G must be a positive integer, got {G!r}")
    tmax = float(tmax)
    if not (np.isfinite(tmax) and tmax > 0.0):
        raise ValueError(f"tmax must be finite and positive, got {tmax!r}")
    if G == 1:
        return np.zeros(1), np.ones(1)
    t = np.linspace(-tmax, tmax, int(G))
    w = np.exp(-0.5 * t * t)
    w[0] *= 0.5
    w[-1] *= 0.5
    return t, w / w.sum()


class ClusterSelection:
    """The checked, immutable record of a survey (cluster_selection): edges (nq + 1,), noise, lnnoise, area (T,), sigma_ln
    (a float or an array (nz, nm)), t, w (G,), noise_model; nq, T, G, omega = sum of area."""
    __slots__ = ("edges", "noise", "lnnoise", "area", "sigma_ln", "t", "w", "noise_model", "nq", "T", "G", "omega")

    def __init__(self, **fields):
        for k, v in fields.items():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
            object.__setattr__(self, k, v)

    def __setattr__(self, name, value):
        raise AttributeError("a ClusterSelection is immutable: make a new one with cluster_selection")

    __delattr__ = __setattr__


def _vector(name, v):
    v = np.array(v, dtype=np.float64, ndmin=1)
    if v.ndim != 1 or v.size < 1:
        raise ValueError(f"{name} must be a scalar or a one-dimensional array, got shape {v.shape}")
    return v


def cluster_selection(q_edges, noise, area, sigma_ln=0.2, rule=None, noise_model="gaussian"):
    """The record of a survey for the cluster counts (ClusterSelection).

    q_edges (nq + 1,): strictly increasing bin edges in significance; the first may be -inf ("gaussian" only), the last
    +inf; with "none" no edge may be negative.  noise, area: scalars or (T,), the noise (> 0, in the units of the
    observable) and the solid angle [sr] (>= 0) of every tile.  sigma_ln: the log-normal intrinsic scatter, a scalar or an
    (nz, nm) array, >= 0 (with "none": > 0).  rule: (t, w), a quadrature rule for the unit normal whose weights sum to 1
    within 1e-12 (None: scatter_rule()).  noise_model: "gaussian" (q = O / noise + N(0, 1)) or "none" (q = O / noise).
    Anything else raises ValueError."""
    if noise_model not in NOISE_MODELS:
        raise ValueError(f"noise_model must be one of {NOISE_MODELS}, got {noise_model!r}")
    edges = np.array(q_edges, dtype=np.float64)
    if edges.ndim != 1 or edges.size < 2:
        raise ValueError(f"q_edges must be one-dimensional with at least two edges, got shape {edges.shape}")
    if np.any(np.isnan(edges)) or not np.all(np.isfinite(edges[1:-1])) or edges[0] == np.inf or edges[-1] == -np.inf:
        raise ValueError("q_edges must be finite, but for a first edge of -inf and a last edge of +inf")
    if not np.all(edges[1:] > edges[:-1]):
        raise ValueError("q_edges must be strictly increasing")
    if noise_model == "none" and edges[0] < 0.0:
        raise ValueError('noise_model="none": q = O / noise is positive, so no edge may be negative or -inf')
    noise, area = _vector("noise", noise), _vector("area", area)
    T = max(noise.size, area.size)
    if noise.size not in (1, T) or area.size not in (1, T):
        raise ValueError(f"noise and area must be scalars or have one entry per tile, got {noise.size} and {area.size}")
    noise, area = np.broadcast_to(noise, (T,)).copy(), np.broadcast_to(area, (T,)).copy()
    if not np.all(np.isfinite(noise)) or np.any(noise <= 0.0):
        raise ValueError("noise must be finite and positive")
    if not np.all(np.isfinite(area)) or np.any(area < 0.0):
        raise ValueError("area must be finite and not negative")
    sig = np.array(sigma_ln, dtype=np.float64)
    if sig.ndim not in (0, 2):
        raise ValueError(f"sigma_ln must be a scalar or an (nz, nm) array, got shape {sig.shape}")
    if not np.all(np.isfinite(sig)) or np.any(sig < 0.0):
        raise ValueError("sigma_ln must be finite and not negative")
    if noise_model == "none" and np.any(sig == 0.0):
        raise ValueError('noise_model="none" needs sigma_ln > 0: without noise and scatter the selection is a step')
    if noise_model == "none":
        if rule is not None:
            raise ValueError('noise_model="none" is a closed form: it takes no rule')
        t, w = np.zeros(1), np.ones(1)
    else:
        try:
            t, w = scatter_rule() if rule is None else rule
        except (TypeError, ValueError):
            raise ValueError("rule must be a pair (t, w) of nodes and weights") from None
        t, w = np.array(t, dtype=np.float64), np.array(w, dtype=np.float64)
        if t.ndim != 1 or t.size < 1 or w.shape != t.shape:
            raise ValueError(f"rule must be two one-dimensional arrays of one length >= 1, got shapes {t.shape} and {w.shape}")
        if not (np.all(np.isfinite(t)) and np.all(np.isfinite(w))):
            raise ValueError("the nodes and weights of rule must be finite")
        if not abs(float(np.sum(w)) - 1.0) <= 1e-12:
            raise ValueError(f"the weights of rule must sum to 1 within 1e-12, got 1 + {float(np.sum(w)) - 1.0:.3e}")
    return ClusterSelection(edges=edges, noise=noise, lnnoise=np.log(noise), area=area,
                            sigma_ln=float(sig) if sig.ndim == 0 else sig, t=t, w=w, noise_model=noise_model,
                            nq=edges.size - 1, T=T, G=t.size, omega=float(np.sum(area)))


# ---------------------------------------------------------------- the request of a model
def mass_window(ms, mmin, mmax):
    """(m_lo, m_hi): the grid masses in [mmin, mmax] (None: the end of the grid), as the one-point methods select them."""
    ms = np.asarray(ms, dtype=np.float64)
    for name, v in (("mmin", mmin), ("mmax", mmax)):
        if v is not None and not (np.isscalar(v) and np.isfinite(v) and v > 0):
            raise ValueError(f"{name} must be a finite positive mass or None, got {v!r}")
    keep = np.nonzero((ms >= (ms[0] if mmin is None else mmin)) & (ms <= (ms[-1] if mmax is None else mmax)))[0]
    if keep.size == 0:
        raise ValueError(f"no point of the mass grid lies in mmin .. mmax = {mmin!r} .. {mmax!r}")
    return int(keep[0]), int(keep[-1]) + 1


def _request(model, lnobs, sel, mmin, mmax):
    """(lnobs, sigma_ln (nz, nm), window): every refusal of a call, on the host, before a context is touched."""
    if not isinstance(sel, ClusterSelection):
        raise ValueError("sel must be the record cluster_selection(...) returns")
    shape = (model.zs.size, model.ms.size)
    if isinstance(lnobs, nat.DeviceArray):
        if tuple(lnobs.shape) != shape:
            raise ValueError(f"lnobs must have shape (nz, nm) = {shape}, got {tuple(lnobs.shape)}")
    else:
        lnobs = np.ascontiguousarray(lnobs, dtype=np.float64)
        if lnobs.shape != shape:
            raise ValueError(f"lnobs must have shape (nz, nm) = {shape}, got {lnobs.shape}")
        if not np.all(np.isfinite(lnobs)):
            raise ValueError("lnobs must be finite")
    sig = sel.sigma_ln
    if isinstance(sig, np.ndarray) and sig.shape != shape:
        raise ValueError(f"sigma_ln of the selection must be a scalar or have shape (nz, nm) = {shape}, got {sig.shape}")
    sig = np.ascontiguousarray(np.broadcast_to(np.asarray(sig, dtype=np.float64), shape))
    return lnobs, sig, mass_window(model.ms, mmin, mmax)


def cluster_abundance_device(model, lnobs, sel, mmin=None, mmax=None, selection=False):
    """(n, bn) or, with selection=True, (n, bn, S) on the device: the abundance n[z, a] = sum_m wm nzm S_a [sr / Mpc^3] and
    the bias-weighted abundance bn[z, a] = sum_m wm nzm bh S_a of the HaloModel `model` in the nq bins of the selection
    `sel` (cluster_selection), both (nz, nq), and the selection S (nz, nm, nq) itself - the area-weighted probability
    that a halo (z, m) lands in bin a, zero outside the mass window.  lnobs (nz, nm): the mean log-observable of every
    halo, a host array or a device array (sz_lnobs, powerlaw_lnobs).  mmin, mmax: only the grid masses in [mmin, mmax].
    One native call; without selection nothing of size nz nm nq exists.  An element (z, a) has the same bits whichever
    other bins and redshifts the call holds."""
    lnobs, sig, (m_lo, m_hi) = _request(model, lnobs, sel, mmin, mmax)
    nz, nm, nq = model._nz, model._nm, sel.nq
    ctx = model._main(needs_aux=True)
    d_ln = lnobs if isinstance(lnobs, nat.DeviceArray) else ctx.upload(lnobs)
    d_sig, d_lnn, d_area = ctx.upload(sig), ctx.upload(sel.lnnoise), ctx.upload(sel.area)
    d_t, d_w, d_e = ctx.upload(sel.t), ctx.upload(sel.w), ctx.upload(sel.edges)
    n, bn = ctx.empty((nz, nq)), ctx.empty((nz, nq))
    S = ctx.empty((nz, nm, nq)) if selection else None
    ctx.call("hmg_cluster_selection", nz=nz, nm=nm, T=sel.T, G=sel.G, nq=nq, kind=NOISE_MODELS.index(sel.noise_model),
             d_lnobs=d_ln.ptr, d_sigln=d_sig.ptr, d_lnnoise=d_lnn.ptr, d_area=d_area.ptr, d_t=d_t.ptr, d_w=d_w.ptr,
             d_edges=d_e.ptr, m_lo=m_lo, m_hi=m_hi, **model._model_block("hmg_cluster_selection"), d_n=n.ptr, d_bn=bn.ptr,
             d_S=nat.ptr(S))
    model._sync_point()
    return (n, bn, S) if selection else (n, bn)


def get_cluster_abundance(model, lnobs, sel, mmin=None, mmax=None, selection=False):
    """cluster_abundance_device on the host: {"n", "bn", "bias" = bn / n (nz, nq)} and, with selection=True, "S"
    (nz, nm, nq).  The bias of an empty bin is nan."""
    got = cluster_abundance_device(model, lnobs, sel, mmin=mmin, mmax=mmax, selection=selection)
    out = {"n": got[0].numpy(), "bn": got[1].numpy()}
    out["bias"] = _ratio(out["bn"], out["n"])
    if selection:
        out["S"] = got[2].numpy()
    return out


def _ratio(a, b):
    with np.errstate(divide="ignore", invalid="ignore"):
        return a / b


# ---------------------------------------------------------------- the z sums and the covariance algebra (host numpy)
def z_bin_weights(zs, z_edges):
    """tw (nzb, nz): row i holds trapz_weights of the nodes of zs in [z_edges[i], z_edges[i + 1]], zero elsewhere.  zs and
    z_edges strictly increasing; every edge must be a node of zs - anything else raises ValueError naming the edge."""
    zs = np.asarray(zs, dtype=np.float64).reshape(-1)
    edges = np.asarray(z_edges, dtype=np.float64)
    if edges.ndim != 1 or edges.size < 2 or not np.all(np.isfinite(edges)) or not np.all(np.diff(edges) > 0):
        raise ValueError("z_edges must be one-dimensional, finite and strictly increasing, at least two edges")
    if zs.size < 2 or not np.all(np.diff(zs) > 0):
        raise ValueError("the counts integrate over the model's redshifts: zs must be strictly increasing, at least two")
    at = []
    for e in edges:
        hit = np.nonzero(zs == e)[0]
        if hit.size != 1:
            raise ValueError(f"z edge {float(e)!r} is not a node of the model's zs")
        at.append(int(hit[0]))
    tw = np.zeros((edges.size - 1, zs.size))
    for i, (lo, hi) in enumerate(zip(at[:-1], at[1:])):
        tw[i, lo:hi + 1] = trapz_weights(zs[lo:hi + 1])
    return tw


def counts_from_abundance(n, zw):
    """N[i, a] = sum_z zw[i, z] n[z, a]."""
    return np.einsum("iz,za->ia", zw, n)


def counts_cov_from_abundance(N, bn, tw, chis, hzs, sigma_b):
    """(poisson, sample), each (nzb, nq, nzb, nq): poisson[i,a,j,b] = delta_ij delta_ab N[i,a] and
    sample[i,a,j,b] = delta_ij sum_z tw[i,z] chi^4 sigma_b / H bn[z,a] bn[z,b]."""
    nzb, nq = N.shape
    poisson, sample = np.zeros((nzb, nq, nzb, nq)), np.zeros((nzb, nq, nzb, nq))
    g = tw * (chis ** 4 * sigma_b / hzs)[None, :]
    for i in range(nzb):
        poisson[i, np.arange(nq), i, np.arange(nq)] = N[i]
        sample[i, :, i, :] = np.einsum("z,za,zb->ab", g[i], bn, bn)
    return poisson, sample


def cl_cov_from_abundance(bn, R, tw, hzs, sigma_b, zscale):
    """Cov[i,a,p,l] = sum_z tw[i,z] H sigma_b zscale[p,z] bn[z,a] R[p,z,l]."""
    return np.einsum("iz,z,pz,za,pzl->iapl", tw, hzs * sigma_b, zscale, bn, R)


def _background(model):
    zs = np.asarray(model.zs, dtype=np.float64).reshape(-1)
    chis = np.asarray(model.comoving_radial_distance(zs), dtype=np.float64).reshape(-1)
    hzs = np.asarray(model.h_of_z(zs), dtype=np.float64).reshape(-1)
    return zs, chis, hzs


def _sigma_b(model, chis, sel, fsky, sigma_b):
    """sigma_b (nz,) of a request: the caller's, or sigma_b_disc on the model's sigma^2 grid at fsky (None: the survey's
    sum of area / 4 pi), as ssc_limber_tables forms it."""
    if sigma_b is not None:
        sigma_b = np.asarray(sigma_b, dtype=np.float64)
        if sigma_b.shape != chis.shape or not np.all(np.isfinite(sigma_b)):
            raise ValueError(f"sigma_b must be finite with one entry per redshift ({chis.size}), got shape {sigma_b.shape}")
        return sigma_b
    if fsky is None:
        fsky = sel.omega / (4.0 * np.pi)
    from .cosmology import sigma2_kgrid
    kq = sigma2_kgrid(model.p["sigma2_kmin"], model.p["sigma2_kmax"], model.p["sigma2_numks"])
    return _cov.sigma_b_disc(kq, model.sPzk, chis, fsky=fsky)


def get_cluster_counts(model, lnobs, sel, z_edges=None, zweights=None, mmin=None, mmax=None):
    """{"N", "bN", "bias" = bN / N (nzb, nq), "n", "bn" (nz, nq)}: the counts N[i, a] = sum_z zw[i, z] n_a[z] of the survey
    `sel` in nzb redshift bins and nq bins of significance, and their bias-weighted twin bN.  Exactly one of z_edges and
    zweights: z_edges (nzb + 1,), every edge a node of model.zs, gives zw[i] = trapz_weights of bin i's nodes times
    chi^2 / H (chi in Mpc, H in 1/Mpc: the comoving volume per steradian and unit redshift); zweights (nzb, nz) replaces
    zw.  Other arguments as cluster_abundance_device."""
    if (z_edges is None) == (zweights is None):
        raise ValueError("give exactly one of z_edges and zweights")
    _request(model, lnobs, sel, mmin, mmax)
    if zweights is None:
        zs, chis, hzs = _background(model)
        zw = z_bin_weights(zs, z_edges) * (chis ** 2 / hzs)[None, :]
    else:
        zw = np.asarray(zweights, dtype=np.float64)
        if zw.ndim != 2 or zw.shape[1] != model.zs.size or zw.shape[0] < 1 or not np.all(np.isfinite(zw)):
            raise ValueError(f"zweights must be finite with shape (nzb, nz) = (nzb, {model.zs.size}), got {zw.shape}")
    ab = get_cluster_abundance(model, lnobs, sel, mmin=mmin, mmax=mmax)
    N, bN = counts_from_abundance(ab["n"], zw), counts_from_abundance(ab["bn"], zw)
    return {"N": N, "bN": bN, "bias": _ratio(bN, N), "n": ab["n"], "bn": ab["bn"]}


def cluster_counts_cov(model, lnobs, sel, z_edges, fsky=None, sigma_b=None, mmin=None, mmax=None):
    """{"N" (nzb, nq), "poisson", "sample", "cov" = poisson + sample (nzb, nq, nzb, nq)}: the covariance of the counts of
    get_cluster_counts(z_edges=...).  poisson[i,a,j,b] = delta_ij delta_ab N[i,a];

        sample[i,a,j,b] = delta_ij sum_{z in i} tw_i[z] chi^4 sigma_b / H  bn_a[z] bn_b[z]

    is the response of the counts to section 17's background mode, <delta_b(z) delta_b(z')> = H delta_D(z - z') sigma_b:
    different z bins are uncorrelated in this Limber form.  sigma_b (nz,) [Mpc]: None takes cov.sigma_b_disc on the
    model's sigma^2 grid at fsky, None there the survey's sum of area / 4 pi."""
    _request(model, lnobs, sel, mmin, mmax)
    zs, chis, hzs = _background(model)
    tw = z_bin_weights(zs, z_edges)
    sigma_b = _sigma_b(model, chis, sel, fsky, sigma_b)
    ab = get_cluster_abundance(model, lnobs, sel, mmin=mmin, mmax=mmax)
    N = counts_from_abundance(ab["n"], tw * (chis ** 2 / hzs)[None, :])
    poisson, sample = counts_cov_from_abundance(N, ab["bn"], tw, chis, hzs, sigma_b)
    return {"N": N, "poisson": poisson, "sample": sample, "cov": poisson + sample}


def cluster_cl_cov(model, lnobs, sel, z_edges, ells, pairs, windows=None, fsky=None, sigma_b=None, damping=True,
                   mmin=None, mmax=None):
    """The covariance of the counts with the Limber spectra C_ell^p of the pairs p = (a, b), (nzb, nq, np, n_ell):

        Cov[i,a,p,l] = sum_{z in i} tw_i[z] H sigma_b W_p1 W_p2 bn_a[z] R_p(z, (l + 1/2) / chi)

    with R = dP / d delta_b from HaloModel.response_device at cov.limber_samples, windows, fsky, sigma_b and damping as in
    cov.cl_cov_ssc (fsky None: the survey's sum of area / 4 pi), so that spectra and counts can be fitted jointly."""
    _request(model, lnobs, sel, mmin, mmax)
    pairs = list(pairs)
    zs, chis, hzs = _background(model)
    tw = z_bin_weights(zs, z_edges)
    sigma_b = _sigma_b(model, chis, sel, fsky, sigma_b)
    idx, frac, _, zscale = _cov.ssc_limber_tables(model, ells, len(pairs), windows, None, sigma_b)
    if idx.shape[1] == 0:
        return np.empty((tw.shape[0], sel.nq, len(pairs), 0))
    bn = cluster_abundance_device(model, lnobs, sel, mmin=mmin, mmax=mmax)[1].numpy()
    R = model.response_device(pairs, idx=idx, frac=frac, damping=damping).numpy()
    return cl_cov_from_abundance(bn, R, tw, hzs, sigma_b, zscale)


# ---------------------------------------------------------------- mean observables
def _grid(model):
    return np.asarray(model.zs, dtype=np.float64).reshape(-1), np.asarray(model.ms, dtype=np.float64).reshape(-1)


def sz_lnobs(model, A0, B0, C0=SZ_DEFAULTS["C0"], mpivot=SZ_DEFAULTS["mpivot"], bias=SZ_DEFAULTS["bias"],
             delta=SZ_DEFAULTS["delta"], Q=None):
    """ln y0 (nz, nm) of the SZ scaling relation

        y0 = 10^A0 E(z)^2 (bias M_delta,c / mpivot)^(1 + B0) (1 + z)^C0 Q(theta_delta),

    E = H(z) / H(0).  M_delta,c (delta = 500) is the mass within delta times the critical density, from the model's
    mass definition and concentrations through mdelta_from_mdelta; theta_delta = R_delta,c / D_A [rad].
    Q = (theta_table, Q_table), interpolated linearly on the host (np.interp: constant beyond the ends), or None: Q = 1."""
    zs, ms = _grid(model)
    dlt, rho = model._mdef_delta_rho()
    rhoc = np.asarray(model.rho_critical_z(zs), dtype=np.float64).reshape(-1)
    mdc = np.asarray(mdelta_from_mdelta(ms, model.concentration(), np.asarray(dlt) * np.asarray(rho), delta * rhoc))
    ez = np.asarray(model.hubble_parameter(zs), dtype=np.float64).reshape(-1) / float(np.asarray(model.hubble_parameter(0.0)))
    out = (np.log(10.0) * A0 + 2.0 * np.log(ez)[:, None] + (1.0 + B0) * np.log(bias * mdc / mpivot)
           + C0 * np.log1p(zs)[:, None])
    if Q is not None:
        theta_t, q_t = (np.asarray(v, dtype=np.float64) for v in Q)
        if theta_t.ndim != 1 or theta_t.shape != q_t.shape or theta_t.size < 2 or np.any(np.diff(theta_t) <= 0) \
                or np.any(q_t <= 0):
            raise ValueError("Q must be (theta_table, Q_table): two arrays of one length, theta increasing, Q positive")
        rdc = (3.0 * mdc / (4.0 * np.pi * delta * rhoc[:, None])) ** (1.0 / 3.0)
        da = np.asarray(model.angular_diameter_distance(zs), dtype=np.float64).reshape(-1)
        out = out + np.log(np.interp(rdc / da[:, None], theta_t, q_t))
    return out


def powerlaw_lnobs(model, lnA, B, C=POWERLAW_DEFAULTS["C"], mpivot=POWERLAW_DEFAULTS["mpivot"],
                   zpivot=POWERLAW_DEFAULTS["zpivot"]):
    """ln O (nz, nm) = lnA + B ln(m / mpivot) + C ln((1 + z) / (1 + zpivot)) on the model's own masses: a richness-like
    proxy."""
    zs, ms = _grid(model)
    return lnA + B * np.log(ms / mpivot)[None, :] + C * np.log((1.0 + zs) / (1.0 + zpivot))[:, None]
