"""The CIB halo model: the cosmic infrared background of a Shang et al. (2012) luminosity-mass
relation at several observed frequencies, its auto and cross-frequency spectra, its crosses with matter (CIB x kappa) and
pressure (CIB x y), and their Limber C_ell.

With nu the observed frequency [GHz], a halo or subhalo of mass M (in the units of the model's ms) has the luminosity

    L(M, z; nu) = L0 Phi(z) Sigma(M) Theta((1 + z) nu, T_d(z)),         Phi = min(1 + z, 1 + z_p)^delta,
    Sigma(M) = M (2 pi sigma2)^-1/2 exp(-(log10 M - log10 M_eff)^2 / (2 sigma2)),      T_d = T0 (1 + z)^alpha,
    Theta(nu, T) = (nu / nu0)^(3 + beta) expm1(x0) / expm1(h nu / k T)  below nu0,   (nu / nu0)^-gamma  from nu0 on,

nu0 = x0 k T / h, x0 the root of x / (1 - exp(-x)) = 3 + beta + gamma (``sed_break``): where the slope of the modified
blackbody is -gamma.  Theta is dimensionless and 1 at nu0; L0 carries the amplitude and the units of L, so every
spectrum here is in units of L0^2 (crosses: L0) - multiply by the L0 of a fit, or pass it in the parameters.

    L_c[f, z, m] = L(ms[m], z; nu_f) / 4 pi  where ms[m] >= M_min, else 0
    L_s[f, z, m] = int_{ln M_min}^{ln ms[m]} dln m_s NlnMsub(m_s | ms[m]) L(m_s, z; nu_f) / 4 pi

are the emissivity weights of the centrals and the satellites, j_f(z) = int dm n (L_c + L_s u); NlnMsub is the subhalo
mass function of Tinker & Wetzel 2010 (``hmvec_amd.tinker.NlnMsub``), the integral an nsub-node Gauss-Legendre rule
(``sub_rule``).  With a flux cut S_cut[f], a source - a central, or a subhalo at a node - with
S = L / (4 pi (1 + z) chi^2) > S_cut[f] is masked.  Both are one native call (``hmg_cib_luminosity``); the spectra of all
F (F + 1) / 2 pairs, the F two-halo legs and the F crosses per partner are one more (``hmg_emission_power``), one pass over
the satellite tensor.  An emissivity tracer is the linear form of an HOD leg, so ``register_emission`` can put one
frequency into ``model.hods`` and every statistic of the library then works for it.

Everything here is a function of a model, as section 25's ``get_cluster_counts(model, ...)`` is: the attribute surface of
HaloModel is a recorded fixture that this section leaves as it is.  Nothing is cached on the model; only
``register_emission`` changes it."""
import numpy as np

from . import _native as nat
from . import bispectrum as bispec
from .hod_ensemble import check_kindex
from .quadrature import sub_rule, trapz_weights

__all__ = ["cib_defaults", "sed_break", "cib_sed", "sub_rule", "cib_luminosities", "emission_tables",
           "emission_power_device", "get_power_cib", "cl_cib", "register_emission", "pair_index", "pair_list",
           "EmissionTables", "EmissionPower", "emission_window", "cl_from_planes", "FMAX", "FREQ_TILE", "PARAMETERS"]

# Planck 2013 XXX / Viero et al. as used by McCarthy & Madhavacheril (2021); masses in the units of the model's ms
cib_defaults = dict(alpha=0.36, T0=24.4, beta=1.75, gamma=1.7, delta=3.6, z_p=2.0, log10_M_eff=12.6, sigma2=0.5,
                    M_min=1.0e10, L0=1.0)
PARAMETERS = ("alpha", "T0", "beta", "gamma", "delta", "z_p", "log10_M_eff", "sigma2", "M_min", "L0")   # h_par, then x0
FMAX = nat.DEFINES["HMG_CIB_FMAX"]           # frequencies of one call, at most
FREQ_TILE = 4                                # csrc/kernels/cib.hpp: CIB_T
KH_GHZ = 20.836619123327576                  # k_B / h [GHz / K]
FOURPI = 12.566370614359172
INV4PI = 0.07957747154594767


# ---------------------------------------------------------------- the SED
def sed_break(beta, gamma):
    """x0 = h nu0 / k T: the root of x / (1 - exp(-x)) = 3 + beta + gamma, by Newton's iteration from x = 3 + beta + gamma
    (the function is increasing and convex: the iteration descends to the root).  3 + beta + gamma must exceed 1."""
    s = 3.0 + float(beta) + float(gamma)
    if not (np.isfinite(s) and s > 1.0):
        raise ValueError(f"3 + beta + gamma must be finite and above 1, got {s!r}")
    x = s
    for _ in range(100):
        d = -np.expm1(-x)                               # 1 - exp(-x)
        step = (x / d - s) / ((d - x * np.exp(-x)) / (d * d))
        x, last = x - step, x
        if abs(x - last) <= 2e-16 * abs(x):
            break
    return float(x)


def _params(params):
    """The parameter dictionary of a request: cib_defaults overridden by `params`; every refusal of a value."""
    p = dict(cib_defaults)
    for k, v in (params or {}).items():
        if k not in p:
            raise ValueError(f"{k!r} is not a parameter of the CIB model; the parameters are {PARAMETERS}")
        p[k] = float(v)
    if not all(np.isfinite(p[k]) for k in PARAMETERS):
        raise ValueError("a parameter of the CIB model is not finite")
    if not (p["T0"] > 0 and p["sigma2"] > 0 and p["M_min"] > 0 and p["z_p"] > -1):
        raise ValueError("T0, sigma2 and M_min must be positive and z_p above -1")
    return p


def _frequencies(nus):
    nus = np.array(nus, dtype=np.float64, ndmin=1)
    if nus.ndim != 1 or nus.size < 1 or not np.all(np.isfinite(nus)) or np.any(nus <= 0):
        raise ValueError("the frequencies must be a one-dimensional array of finite positive numbers [GHz]")
    return nus


def sed_parts(nus, zs, p, x0):
    """(Theta, Phi), each (F, nz), in the order of the operations of csrc/kernels/cib.hpp."""
    zp1 = 1.0 + np.asarray(zs, dtype=np.float64).reshape(-1)
    phi = np.minimum(zp1, 1.0 + p["z_p"]) ** p["delta"]
    Td = p["T0"] * zp1 ** p["alpha"]
    nu0 = (x0 * KH_GHZ) * Td
    r = (zp1[None, :] * nus[:, None]) / nu0[None, :]
    with np.errstate(over="ignore"):
        low = r ** (3.0 + p["beta"]) * (np.expm1(x0) / np.expm1(x0 * r))
    theta = np.where(r < 1.0, low, r ** (-p["gamma"]))
    return theta, np.broadcast_to(phi[None, :], theta.shape)


def cib_sed(nus, zs, params=None):
    """Theta((1 + z) nu, T_d(z)), (F, nz): the SED factor of the model at the observed frequencies nus [GHz]."""
    p = _params(params)
    return sed_parts(_frequencies(nus), zs, p, sed_break(p["beta"], p["gamma"]))[0].copy()


# ---------------------------------------------------------------- pairs
def pair_index(f, g, F):
    """The plane of the pair (f, g), f <= g, of F frequencies: f F - f (f - 1) / 2 + (g - f)."""
    f, g = (int(f), int(g)) if f <= g else (int(g), int(f))
    if not 0 <= f <= g < F:
        raise ValueError(f"a pair of {F} frequencies must lie in 0 .. {F - 1}, got ({f}, {g})")
    return f * F - f * (f - 1) // 2 + (g - f)


def pair_list(F):
    """[(f, g), ...], f <= g, in the order of the planes."""
    return [(f, g) for f in range(F) for g in range(f, F)]


# ---------------------------------------------------------------- records
class _Record:
    __slots__ = ()

    def __init__(self, **fields):
        for k, v in fields.items():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
            object.__setattr__(self, k, v)

    def __setattr__(self, name, value):
        raise AttributeError(f"a {type(self).__name__} is immutable")

    __delattr__ = __setattr__


class EmissionTables(_Record):
    """The checked, immutable record of F emissivity tracers on a model's grid (cib_luminosities, emission_tables): Lc, Ls
    (device arrays (F, nz, nm)), jbar (F, nz) = int dm n (L_c + L_s), bias (F, nz) the luminosity-weighted halo bias, F,
    nus (F,) or None, params (a dict) or None, flux_cut (F,) or None."""
    __slots__ = ("Lc", "Ls", "jbar", "bias", "F", "nus", "params", "flux_cut", "shape")


class EmissionPower(_Record):
    """What emission_power_device returns, device arrays: P1h (npair, nz, n), I (F, nz, n), X1h (NP, F, nz, n) or None;
    partners (names), pairs, F, n, kindex (None: the whole grid)."""
    __slots__ = ("P1h", "I", "X1h", "partners", "pairs", "F", "n", "kindex")


def _grid(model):
    zs = np.asarray(model.zs, dtype=np.float64).reshape(-1)
    ms = np.asarray(model.ms, dtype=np.float64).reshape(-1)
    if ms.size < 2 or not np.all(np.diff(ms) > 0):
        raise ValueError("the masses of the model must be strictly ascending")
    return zs, ms


def _sums(model, Lc, Ls):
    """(jbar, bias), each (F, nz), through the model's get_ngal and get_bg."""
    jbar = np.stack([np.asarray(model.get_ngal(Lc[f], Ls[f])) for f in range(Lc.shape[0])])
    with np.errstate(divide="ignore", invalid="ignore"):
        bias = np.stack([np.asarray(model.get_bg(Lc[f], Ls[f], jbar[f])) for f in range(Lc.shape[0])])
    return jbar, bias


def _tables(model, d_Lc, d_Ls, **meta):
    jbar, bias = _sums(model, d_Lc.numpy(), d_Ls.numpy())
    return EmissionTables(Lc=d_Lc, Ls=d_Ls, jbar=jbar, bias=bias, F=d_Lc.shape[0], shape=tuple(d_Lc.shape), **meta)


def luminosity_call(model, nus, p, x0, scut, t, w):
    """One hmg_cib_luminosity launch: the device arrays (d_Lc, d_Ls), each (F, nz, nm).  No checks: cib_luminosities is the
    public face; the tests call this with rules of their own."""
    zs, ms = _grid(model)
    chis = np.asarray(model.comoving_radial_distance(zs), dtype=np.float64).reshape(-1)
    F, nz, nm = nus.size, zs.size, ms.size
    ctx = model._main(needs_aux=True)
    d_nus, d_chis, d_t, d_w = ctx.upload(nus), ctx.upload(chis), ctx.upload(t), ctx.upload(w)
    d_cut = None if scut is None else ctx.upload(scut)
    d_Lc, d_Ls = ctx.empty((F, nz, nm)), ctx.empty((F, nz, nm))
    par = (nat.C.c_double * nat.DEFINES["HMG_CIB_NPAR"])(*[p[k] for k in PARAMETERS], x0)
    ctx.call("hmg_cib_luminosity", F=F, nz=nz, nm=nm, nsub=t.size, d_nus=d_nus.ptr, d_zs=model._d_zs().ptr,
             d_ms=model._d_ms().ptr, d_chis=d_chis.ptr, d_scut=nat.ptr(d_cut), d_t=d_t.ptr, d_w=d_w.ptr, h_par=par,
             d_Lc=d_Lc.ptr, d_Ls=d_Ls.ptr)
    model._sync_point()
    return d_Lc, d_Ls


def cib_luminosities(model, nus_GHz, params=None, flux_cut=None, nsub=64):
    """The emissivity weights of the CIB model at the observed frequencies nus_GHz (F <= FMAX = 16) on the grid of the
    HaloModel `model`: an EmissionTables record with the device arrays Lc, Ls (F, nz, nm) and the host sums jbar and bias
    (F, nz).  params: overrides of cib_defaults.  flux_cut: None, or S_cut (F,) >= 0 in the units of L0 / Mpc^2 - a source
    with L / (4 pi (1 + z) chi^2) > S_cut[f] is masked, chi the model's comoving distance [Mpc].  nsub >= 2: the nodes of
    the subhalo integral.  A bad request raises ValueError and touches nothing."""
    p = _params(params)
    nus = _frequencies(nus_GHz)
    if nus.size > FMAX:
        raise ValueError(f"{nus.size} frequencies: one call takes at most FMAX = {FMAX}")
    t, w = sub_rule(nsub)
    _grid(model)
    scut = None
    if flux_cut is not None:
        scut = np.array(flux_cut, dtype=np.float64, ndmin=1)
        if scut.shape != nus.shape:
            raise ValueError(f"flux_cut must have one entry per frequency ({nus.size}), got shape {scut.shape}")
        if np.any(np.isnan(scut)) or np.any(scut < 0):
            raise ValueError("flux_cut must not be negative")
    x0 = sed_break(p["beta"], p["gamma"])
    d_Lc, d_Ls = luminosity_call(model, nus, p, x0, scut, t, w)
    return _tables(model, d_Lc, d_Ls, nus=nus, params=p, flux_cut=scut)


def emission_tables(model, Lc, Ls):
    """The EmissionTables record of the caller's own emissivity weights Lc, Ls (F, nz, nm), host or device arrays: another
    L-M relation, or the lines of a line-intensity survey as "frequencies"."""
    shape = None
    out = []
    for name, a in (("Lc", Lc), ("Ls", Ls)):
        if not isinstance(a, nat.DeviceArray):
            a = np.ascontiguousarray(a, dtype=np.float64)
            if not np.all(np.isfinite(a)):
                raise ValueError(f"{name} must be finite")
        want = (a.shape[0] if len(a.shape) == 3 else -1, model.zs.size, model.ms.size)
        if tuple(a.shape) != want:
            raise ValueError(f"{name} must have shape (F, nz, nm) = (F, {want[1]}, {want[2]}), got {tuple(a.shape)}")
        if shape is not None and tuple(a.shape) != shape:
            raise ValueError(f"Lc and Ls must have one shape, got {shape} and {tuple(a.shape)}")
        shape = tuple(a.shape)
        out.append(a)
    if not 1 <= shape[0] <= FMAX:
        raise ValueError(f"{shape[0]} frequencies: one call takes 1 .. FMAX = {FMAX}")
    _grid(model)
    ctx = model._main(needs_aux=True)
    d_Lc, d_Ls = (a if isinstance(a, nat.DeviceArray) else ctx.upload(a) for a in out)
    return _tables(model, d_Lc, d_Ls, nus=None, params=None, flux_cut=None)


# ---------------------------------------------------------------- spectra
def _check_tables(model, tables):
    if not isinstance(tables, EmissionTables):
        raise ValueError("tables must be the record cib_luminosities or emission_tables returns")
    if tables.shape[1:] != (model.zs.size, model.ms.size):
        raise ValueError(f"the tables were made for a grid {tables.shape[1:]}, the model's is {(model.zs.size, model.ms.size)}")


def _satellite(model, name):
    if name not in model.uk_profiles:
        raise ValueError(f"satellite_profile_name {name!r} is not a matter profile of this model")
    return name


def _partners(model, partners):
    """[(name, kind "m" | "p"), ...] of a request: at most two, each a matter or a pressure profile of the model."""
    partners = (partners,) if isinstance(partners, str) else tuple(partners)
    if len(partners) > 2:
        raise ValueError(f"at most two partners, got {len(partners)}")
    out = []
    for nm_ in partners:
        if nm_ in model.hods:
            raise ValueError(f"partner {nm_!r} is an HOD: a partner of an emission is a matter or a pressure profile")
        if nm_ in model.uk_profiles:
            out.append((nm_, "m"))
        elif nm_ in model.pk_profiles:
            out.append((nm_, "p"))
        else:
            raise ValueError(f"unknown partner {nm_!r}: no matter or pressure profile of this model has that name")
    return out


def emission_power_device(model, tables, partners=(), satellite_profile_name="nfw", kindex=None, damping=True):
    """The mass integrals of F emissivity tracers in one pass over the satellite tensor, on the device: an EmissionPower
    with P1h (npair, nz, n) of every pair f <= g (pair_index), the two-halo legs I (F, nz, n) - P2h_fg = Pzk I_f I_g - and
    the one-halo crosses X1h (NP, F, nz, n) with up to two partners, names of matter or pressure profiles.  kindex: the
    nodes of the k grid (default: all); damping as in get_power_1halo.  Nothing is registered; cached spectra stay valid."""
    _check_tables(model, tables)
    sat = _satellite(model, satellite_profile_name)
    parts = _partners(model, partners)
    nz, nm, nk = model._nz, model._nm, model._nk
    kindex = check_kindex(kindex, nk)
    F, NP, n = tables.F, len(parts), nk if kindex is None else kindex.size
    nodes = model.ks if kindex is None else model.ks[kindex]
    damp = bispec.damping(nodes, model.p["kstar_damping"]) if damping else np.ones(n)
    ctx = model._main(needs_aux=True)
    shape = (nz, nm, nk)
    # (another reader of the tensors than the batched mass integrals: a deferred left fill is written first)
    d_us = model.uk_profiles.dev(sat, fill=True)
    tensors = [(sat, d_us)]
    tr = []
    for nm_, kind in parts:
        d_ = (model.uk_profiles if kind == "m" else model.pk_profiles).dev(nm_, fill=True)
        tensors.append((nm_, d_))
        tr.append(nat.Tracer(nat.TRACER_MATTER if kind == "m" else nat.TRACER_PRESSURE, d_.ptr))
    for nm_, d_ in tensors:
        if d_.shape != shape:
            raise ValueError(f"profile {nm_!r} has shape {d_.shape}, the model's grid is {shape}")
    d_k = None if kindex is None else ctx.upload_int32(kindex)
    d_damp = ctx.upload(np.ascontiguousarray(damp, dtype=np.float64))
    npair = F * (F + 1) // 2
    P1h, I = ctx.empty((npair, nz, n)), ctx.empty((F, nz, n))
    X1h = ctx.empty((NP, F, nz, n)) if NP else None
    h_partners = (nat.Tracer * NP)(*tr) if NP else None
    ctx.call("hmg_emission_power", F=F, nz=nz, nm=nm, nk=nk, n=n, d_us=d_us.ptr, d_Lc=tables.Lc.ptr, d_Ls=tables.Ls.ptr,
             NP=NP, h_partners=h_partners, **model._model_block("hmg_emission_power"), d_kindex=nat.ptr(d_k),
             d_damp=d_damp.ptr, d_P1h=P1h.ptr, d_I=I.ptr, d_X1h=nat.ptr(X1h))
    model._sync_point()
    return EmissionPower(P1h=P1h, I=I, X1h=X1h, partners=tuple(nm_ for nm_, _ in parts), pairs=tuple(pair_list(F)), F=F,
                         n=n, kindex=kindex)


def _partner_brackets(model, parts, cols):
    """J_p (NP, nz, n) = (I_p + b_p) - C_p of the partners' two-halo terms: b = 1 for matter, 0 for pressure."""
    out = []
    for nm_, kind in parts:
        i1, c1, _, _ = model.two_halo_terms(nm_)
        out.append((i1[:, cols] + (1.0 if kind == "m" else 0.0)) - c1)
    return np.array(out)


def assemble(P1h, I, X1h, Pzk, J):
    """The planes of get_power_cib from the mass integrals, host arrays: ({"1h", "2h", "total"} of the pairs (npair, nz,
    n), the same of the crosses (NP, F, nz, n) or None).  P2h_fg = (Pzk I_f) I_g, P2h_pf = (Pzk I_f) J_p."""
    F = I.shape[0]
    PI = Pzk[None] * I
    two = np.stack([PI[f] * I[g] for f, g in pair_list(F)])
    auto = {"1h": P1h, "2h": two, "total": P1h + two}
    if X1h is None:
        return auto, None
    two_x = PI[None] * J[:, None]
    return auto, {"1h": X1h, "2h": two_x, "total": X1h + two_x}


def get_power_cib(model, nus, partners=("nfw",), params=None, flux_cut=None, nsub=64, tables=None,
                  satellite_profile_name="nfw", kindex=None, damping=True):
    """The CIB spectra of the frequencies nus [GHz] on the host: a dict with "1h", "2h", "total" (npair, nz, n) of the pairs
    f <= g in the order of "pairs"; "cross_1h", "cross_2h", "cross_total" (NP, F, nz, n) with the partners (matter
    profiles: CIB x matter; pressure profiles: CIB x pressure), P2h_pf = Pzk I_f J_p with the partner's bracket from
    two_halo_terms; "jbar" and "bias" (F, nz); "I" (F, nz, n).  The spectra are those of the emissivity j, not of
    j / jbar.  tables: an EmissionTables record instead of nus, params, flux_cut and nsub (nus is then ignored)."""
    parts = _partners(model, partners)          # (the refusals of the second call before the first one launches)
    _satellite(model, satellite_profile_name)
    check_kindex(kindex, model._nk)
    if tables is None:
        tables = cib_luminosities(model, nus, params=params, flux_cut=flux_cut, nsub=nsub)
    r = emission_power_device(model, tables, partners=partners, satellite_profile_name=satellite_profile_name,
                              kindex=kindex, damping=damping)
    cols = np.arange(model._nk) if r.kindex is None else r.kindex
    J = _partner_brackets(model, parts, cols) if parts else None
    auto, cross = assemble(r.P1h.numpy(), r.I.numpy(), None if r.X1h is None else r.X1h.numpy(),
                           np.asarray(model.Pzk)[:, cols], J)
    out = dict(auto)
    out.update(pairs=list(r.pairs), jbar=np.array(tables.jbar), bias=np.array(tables.bias), I=r.I.numpy(),
               partners=list(r.partners))
    if cross is not None:
        out.update({"cross_" + k: v for k, v in cross.items()})
    return out


# ---------------------------------------------------------------- C_ell
def emission_window(zs, hzs):
    """W_j(z) = a / H: with hmg_limber's prefactor H W1 W2 / chi^2 two of them give int dchi a^2 / chi^2 P_jj."""
    return 1.0 / ((1.0 + np.asarray(zs, dtype=np.float64)) * np.asarray(hzs, dtype=np.float64))


def cl_from_planes(ells, zs, ks, chis, hzs, planes, W1, W2):
    """The Limber sum of hmg_limber on host arrays, with the model's redshifts as the nodes of the z integral:
    C_ell = sum_z trapz_weights(zs)[z] (H W1 W2 / chi^2)[z] P(z, k = (ell + 1/2) / chi[z]), P linear in k between the
    nodes and clamped to the grid.  planes (..., nz, nk) -> (..., n_ell)."""
    ells = np.asarray(ells, dtype=np.float64).reshape(-1)
    planes = np.asarray(planes, dtype=np.float64)
    pref = trapz_weights(zs) * (hzs * W1 * W2 / chis ** 2.0) if np.size(zs) > 1 else hzs * W1 * W2 / chis ** 2.0
    out = np.zeros(planes.shape[:-2] + (ells.size,))
    for z in range(np.size(zs)):
        kev = np.clip((ells + 0.5) / chis[z], ks[0], ks[-1])
        i = np.clip(np.searchsorted(ks, kev, side="right") - 1, 0, ks.size - 2)
        tx = (kev - ks[i]) / (ks[i + 1] - ks[i])
        out = out + pref[z] * ((1.0 - tx) * planes[..., z, i] + tx * planes[..., z, i + 1])
    return out


def _windows(model, parts, windows, zs):
    """The partners' windows W_p(z) (NP, nz): the caller's, else the CMB-lensing window (matter) or 1 (pressure)."""
    windows = [None] * len(parts) if windows is None else list(windows)
    if len(windows) != len(parts):
        raise ValueError(f"windows must have one entry per partner ({len(parts)}), got {len(windows)}")
    out = []
    for (nm_, kind), W in zip(parts, windows):
        if W is None:
            W = model.lensing_window(zs, 1100.0) if kind == "m" else np.ones(zs.size)
        W = np.asarray(W, dtype=np.float64)
        if W.shape != zs.shape or not np.all(np.isfinite(W)):
            raise ValueError(f"the window of partner {nm_!r} must be finite with one entry per redshift ({zs.size})")
        out.append(W)
    return out


def cl_cib(model, ells, tables, partners=(), windows=None, satellite_profile_name="nfw", damping=True):
    """The Limber spectra of the CIB: {"cl" (npair, n_ell): C_ell^{nu nu'} = int dchi a^2 / chi^2 P_jj(k = (ell + 1/2) /
    chi), "cross" (NP, F, n_ell): C_ell^{nu kappa} for a matter partner (window: windows[p], default the CMB-lensing
    window of source redshift 1100) and C_ell^{nu y} for a pressure partner (default window 1, as C_yy), "pairs"}.  The z
    integral is the trapezoid rule over the model's redshifts (at least two); one hmg_limber call per plane."""
    _check_tables(model, tables)
    parts = _partners(model, partners)
    zs = np.asarray(model.zs, dtype=np.float64).reshape(-1)
    if zs.size < 2 or not np.all(np.diff(zs) > 0):
        raise ValueError("the Limber integral runs over the model's redshifts: zs must be strictly increasing, at least two")
    ells = np.asarray(ells, dtype=np.float64)
    if ells.ndim != 1 or ells.size < 1 or not np.all(np.isfinite(ells)) or np.any(ells < 0):
        raise ValueError("ells must be a one-dimensional array of finite multipoles >= 0")
    Wp = _windows(model, parts, windows, zs)
    got = get_power_cib(model, None, partners=partners, tables=tables, satellite_profile_name=satellite_profile_name,
                        damping=damping)
    hzs = np.asarray(model.h_of_z(zs), dtype=np.float64).reshape(-1)
    chis = np.asarray(model.comoving_radial_distance(zs), dtype=np.float64).reshape(-1)
    Wj = emission_window(zs, hzs)

    def limber(plane, W2):
        return model.limber_integral(ells, zs, model.ks, plane, zs, Wj, W2, hzs, chis)

    out = {"cl": np.stack([limber(P, Wj) for P in got["total"]]), "pairs": got["pairs"], "partners": got["partners"]}
    if parts:
        out["cross"] = np.stack([np.stack([limber(got["cross_total"][p, f], Wp[p]) for f in range(tables.F)])
                                 for p in range(len(parts))])
    return out


# ---------------------------------------------------------------- one frequency as an HOD-shaped entry
def register_emission(model, name, tables, f, satellite_profile_name="nfw", ignore_existing=False):
    """Put frequency f of `tables` into model.hods as an HOD-shaped entry `name`: Nc = L_c, Ns = L_s, NcNs = L_c L_s,
    NsNsm1 = L_s^2, ngal = jbar, bg = bias.  Every statistic of the library then works for the CIB at that frequency -
    get_power(name) jbar^2 is P1h[f, f] + P2h[f, f] of get_power_cib - in units of jbar.  Refuses a name that is taken (a
    profile's always, an HOD's unless ignore_existing) and a frequency whose jbar is not positive at every redshift."""
    from .halomodel import HodEntry
    _check_tables(model, tables)
    sat = _satellite(model, satellite_profile_name)
    if not isinstance(name, str) or not name:
        raise ValueError("name must be a non-empty string")
    if name in model.uk_profiles or name in model.pk_profiles:
        raise ValueError(f"{name!r} already names a profile of this model")
    if name in model.hods and not ignore_existing:
        raise ValueError(f"{name!r} already names an HOD of this model (ignore_existing=True replaces it)")
    if isinstance(f, bool) or not isinstance(f, (int, np.integer)) or not 0 <= f < tables.F:
        raise ValueError(f"f must be a frequency of the tables, 0 .. {tables.F - 1}, got {f!r}")
    jbar, bias = tables.jbar[f], tables.bias[f]
    if not (np.all(np.isfinite(jbar)) and np.all(jbar > 0) and np.all(np.isfinite(bias))):
        raise ValueError(f"frequency {f} has no emission at some redshift: jbar must be positive")
    nz, nm = model._nz, model._nm
    Lc = tables.Lc.view(int(f) * nz * nm, (nz, nm)).numpy()
    Ls = tables.Ls.view(int(f) * nz * nm, (nz, nm)).numpy()
    ctx = model._main(needs_aux=True)
    dev = {"Nc": ctx.upload(Lc), "Ns": ctx.upload(Ls), "NsNsm1": ctx.upload(Ls * Ls), "NcNs": ctx.upload(Lc * Ls),
           "ngal": ctx.upload(jbar), "bg": ctx.upload(bias)}
    model._bump()
    model.hods[name] = HodEntry(dev, dict(satellite_profile=sat, central_profile=None, emission=True))
