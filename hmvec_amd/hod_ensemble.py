"""HOD parameter ensembles.

``HaloModel.hod_ensemble_device`` / ``get_power_hod_ensemble`` give P_gg and P_gm of many HOD parameter sets at once
against one mass function and one pair of profile tensors; ``HaloModel.hod_ensemble_occupations`` gives their occupation
numbers.  The functions of this module are the host side - plain data and arithmetic, no library calls: the table of
parameter sets, the central-difference stencil of a Fisher forecast and its derivatives, the checks of a request and the
layout of the coefficient block the two native calls share.  ``HodEnsembleMixin`` holds those methods of HaloModel.
"""
import numpy as np

from . import _native as nat
from . import bispectrum as bispec
from .params import default_params

__all__ = ["hod_sets", "stencil", "central_differences", "COLUMNS", "HodSets", "StencilPlan", "HodEnsembleResult"]

COLUMNS = ("sig_log_mstellar", "alphasat", "Bsat", "betasat", "Bcut", "betacut")     # the order of a native set
SHORT = {"sig": "sig_log_mstellar"}
THRESHOLD = "log10mthresh"        # the pseudo-parameter a stencil may step
SET_TILE = 8                      # the coefficient block pads S to a multiple of this (csrc/kernels/hodens.hpp: HE_TS)
POWER_KEYS = ("gg_1h", "gg_2h", "gm_1h", "gm_2h")      # the planes of the native result, in order


class HodSets(np.ndarray):
    """An (S, 6) float64 table of HOD parameter sets; ``columns`` names its columns, ``column(name)`` returns one."""
    columns = COLUMNS

    def column(self, name):
        return np.asarray(self[:, COLUMNS.index(_column(name))])


def _column(name):
    key = name[4:] if isinstance(name, str) and name.startswith("hod_") else name
    key = SHORT.get(key, key)
    if key not in COLUMNS:
        raise ValueError(f"{name!r} is not a column of an HOD parameter set; the columns are {COLUMNS}")
    return key


def _check(table):
    if not np.all(np.isfinite(table)):
        raise ValueError("an HOD parameter set holds a value that is not finite")
    if np.any(table[:, 0] <= 0.0):
        raise ValueError("sig_log_mstellar must be positive")
    if np.any(table[:, 2] <= 0.0):
        raise ValueError("Bsat must be positive")
    if np.any(table[:, 4] < 0.0):
        raise ValueError("Bcut must not be negative")
    return table


def _base_row(base):
    """The six defaults: default_params, overridden by `base` - a mapping of columns (short names or the hod_* keys of a
    parameter dictionary; other keys are ignored only if they are hod_* or cosmology keys of default_params) or one set."""
    row = np.array([default_params["hod_" + c] for c in COLUMNS], dtype=np.float64)
    if base is None:
        return row
    if isinstance(base, dict):
        for k, v in base.items():
            if k == THRESHOLD or (k in default_params and (not k.startswith("hod_") or k[4:] not in COLUMNS)):
                continue
            row[COLUMNS.index(_column(k))] = float(v)
        return row
    b = np.asarray(base, dtype=np.float64)
    if b.shape not in ((6,), (1, 6)):
        raise ValueError(f"base must be a mapping or one parameter set of 6 numbers, got shape {b.shape}")
    return b.reshape(6).copy()


def hod_sets(n=None, base=None, **columns):
    """An (S, 6) table of parameter sets (HodSets).  Every column starts from default_params, or from `base` (a mapping or
    one set); a keyword per column - sig (or sig_log_mstellar), alphasat, Bsat, betasat, Bcut, betacut, with or without
    the hod_ prefix - gives a scalar, broadcast, or one value per set.  S is n, or the common length of the columns.
    Unknown columns, values that are not finite, sig <= 0, Bsat <= 0 and Bcut < 0 raise ValueError."""
    row = _base_row(base)
    cols = {}
    for k, v in columns.items():
        key = _column(k)
        if key in cols:
            raise ValueError(f"column {key!r} is given twice")
        v = np.asarray(v, dtype=np.float64)
        if v.ndim > 1:
            raise ValueError(f"column {k!r} must be a scalar or one-dimensional, got shape {v.shape}")
        cols[key] = v
    sizes = {v.size for v in cols.values() if v.ndim == 1}
    if n is not None:
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 1:
            raise ValueError(f"n must be a positive integer, got {n!r}")
        sizes.add(int(n))
    if len(sizes) > 1:
        raise ValueError(f"the columns have different lengths: {sorted(sizes)}")
    S = sizes.pop() if sizes else 1
    if S < 1:
        raise ValueError("no parameter set: a column is empty")
    table = np.tile(row, (S, 1))
    for key, v in cols.items():
        table[:, COLUMNS.index(key)] = v
    return _check(table).view(HodSets)


def as_sets(sets):
    """The checked, contiguous (S, 6) float64 table of a request."""
    t = np.array(sets, dtype=np.float64, ndmin=2)
    if t.ndim != 2 or t.shape[1] != 6 or t.shape[0] < 1:
        raise ValueError(f"sets must have shape (S, 6) with S >= 1, got {np.shape(sets)}")
    return np.ascontiguousarray(_check(t))


class StencilPlan:
    """Which rows of a stencil belong to which parameter: ``params`` in order, ``steps[p]``, ``rows[p] = (plus, minus)``,
    row 0 the base; ``log10mthresh_offset`` (S,) is what each row adds to the base thresholds (zero unless the
    pseudo-parameter log10mthresh is stepped)."""

    def __init__(self, params, steps, rows, offset):
        self.params, self.steps, self.rows, self.log10mthresh_offset = tuple(params), dict(steps), dict(rows), offset
        self.size = offset.size


def stencil(base, steps):
    """(sets, plan): the 1 + 2P sets of a central-difference stencil about `base` (as hod_sets takes it) - row 0 the base,
    then for each parameter of `steps` (a mapping parameter -> step > 0, in its order) the row with the parameter raised
    and the row with it lowered by the step.  "log10mthresh" is allowed as a pseudo-parameter: its two rows are the base
    set, and plan.log10mthresh_offset says what to add to the thresholds."""
    row = _check(_base_row(base)[None, :])[0]
    params, hs, rows = [], {}, {}
    table = [row.copy()]
    offset = [0.0]
    for p, h in steps.items():
        key = THRESHOLD if p == THRESHOLD else _column(p)
        h = float(h)
        if key in hs:
            raise ValueError(f"parameter {key!r} is stepped twice")
        if not (np.isfinite(h) and h > 0.0):
            raise ValueError(f"the step of {p!r} must be finite and positive, got {h!r}")
        rows[key] = (len(table), len(table) + 1)
        for sign in (1.0, -1.0):
            r = row.copy()
            if key == THRESHOLD:
                offset.append(sign * h)
            else:
                r[COLUMNS.index(key)] += sign * h
                offset.append(0.0)
            table.append(r)
        params.append(key)
        hs[key] = h
    return _check(np.array(table)).view(HodSets), StencilPlan(params, hs, rows, np.array(offset))


def central_differences(values, plan):
    """{parameter: d values / d parameter} by central differences from ensemble results with the stencil's rows on axis 0:
    (values[plus] - values[minus]) / (2 step)."""
    values = np.asarray(values)
    if values.shape[0] != plan.size:
        raise ValueError(f"values has {values.shape[0]} rows on axis 0, the stencil has {plan.size}")
    return {p: (values[plan.rows[p][0]] - values[plan.rows[p][1]]) / (2.0 * plan.steps[p]) for p in plan.params}


# ---------------------------------------------------------------- the checks of a request
def per_set(x, S, nz, what):
    """x as a contiguous (S, nz) float64 array: (nz,) is shared by the sets."""
    x = np.asarray(x, dtype=np.float64)
    if x.shape == (nz,):
        x = np.broadcast_to(x[None, :], (S, nz))
    if x.shape != (S, nz):
        raise ValueError(f"{what} must have shape (nz,) = ({nz},) or (S, nz) = ({S}, {nz}), got {x.shape}")
    if not np.all(np.isfinite(x)) or np.any(x <= 0.0):
        raise ValueError(f"{what} must be finite and positive")
    return np.ascontiguousarray(x)


def check_corr(corr):
    if corr not in ("max", "min"):
        raise ValueError(f"corr must be 'max' or 'min', got {corr!r}")
    return {"max": 0, "min": 1}[corr]


def check_kindex(kindex, nk):
    """None (the whole grid) or the int32 nodes of a request: one-dimensional, not empty, in 0 .. nk - 1, any order."""
    if kindex is None:
        return None
    kindex = np.asarray(kindex)
    if kindex.ndim != 1 or not np.issubdtype(kindex.dtype, np.integer):
        raise ValueError("kindex must be a one-dimensional integer array of indices into ks")
    if kindex.size < 1:
        raise ValueError("kindex is empty: at least one node is needed")
    if kindex.min() < 0 or kindex.max() > nk - 1:
        raise ValueError(f"kindex must lie in 0 .. nk - 1 = {nk - 1}, got {kindex.min()} .. {kindex.max()}")
    return np.ascontiguousarray(kindex, dtype=np.int32)


def coef_block_size(S, nz, nm):
    """Doubles of the coefficient block of S sets: coef[nz][nm][Spad][4] and craw[S][nz], Spad = S rounded up to 8."""
    spad = (S + SET_TILE - 1) // SET_TILE * SET_TILE
    return 4 * nz * nm * spad + S * nz


def bisection_step(lo, hi, mid, miss, active):
    """One update of utils.vectorized_bisection_search ("decreasing") for the active sets (rows) alone: where the model's
    n_gal is above the target the threshold rises."""
    over = (miss > 0) & active[:, None]
    under = (miss <= 0) & active[:, None]
    lo[over] = mid[over]
    hi[under] = mid[under]


class HodEnsembleResult:
    """What hod_ensemble_device returns, device arrays: power (4, S, nz, n) = (P1h_gg, P2h_gg, P1h_gm, P2h_gm), ngal, bg
    and log10mthresh (S, nz), parts (3, S, nz, n) = (G, X, I) or None; iterations is the number of launches of the n_gal
    bisection (0 with mthresh)."""

    def __init__(self, power, ngal, bg, log10mthresh, parts, iterations=0):
        self.power, self.ngal, self.bg, self.log10mthresh, self.parts = power, ngal, bg, log10mthresh, parts
        self.iterations = iterations


class HodEnsembleMixin:
    """HaloModel's P_gg and P_gm of S parameter sets in one pass over the tensors (hmg_hod_ensemble, hmg_hod_ensemble_power).
    Nothing is registered in hods and the model's version does not change: cached spectra stay valid."""

    def _hodens_request(self, sets, mthresh, ngal, corr):
        """(sets (S, 6), corr flag, log10 thresholds (S, nz) or None, n_gal targets (S, nz) or None): every refusal of the
        HOD half of a request, on the host."""
        sets = as_sets(sets)
        if (mthresh is None) == (ngal is None):
            raise ValueError("give exactly one of mthresh and ngal")
        S, nz = sets.shape[0], self._nz
        flag = check_corr(corr)
        if ngal is not None:
            return sets, flag, None, per_set(ngal, S, nz, "ngal")
        return sets, flag, np.log10(per_set(mthresh, S, nz, "mthresh")), None

    def _hodens_occ(self, ctx, d_par, flag, l10, S, occ=None, coef=None):
        """One hmg_hod_ensemble launch at the thresholds l10 (S, nz): (d_lthr, d_ngal, d_bg)."""
        nz, nm = self._nz, self._nm
        d_thr, d_ngal, d_bg = ctx.upload(np.ascontiguousarray(l10)), ctx.empty((S, nz)), ctx.empty((S, nz))
        ctx.call("hmg_hod_ensemble", S=S, nz=nz, nm=nm, corr=flag, d_par=d_par.ptr, d_lthr=d_thr.ptr, d_zs=self._d_zs().ptr,
                 **self._model_block("hmg_hod_ensemble"), d_ngal=d_ngal.ptr, d_bg=d_bg.ptr, d_occ=nat.ptr(occ),
                 d_coef=nat.ptr(coef))
        return d_thr, d_ngal, d_bg

    def _hodens_bisect(self, ctx, d_par, target):
        """log10 mthresh (S, nz) by one batched bisection, and its number of launches.  The rules are those of
        utils.vectorized_bisection_search with the stop test per set: a set stops updating once all of its redshifts meet
        hod_bisection_search_rtol - the thresholds add_hod(ngal=target[s]) finds for that set alone - while the others go
        on; the number of launches is the largest iteration count."""
        p = self.p
        S = target.shape[0]
        lo = np.zeros_like(target) + p["hod_bisection_search_min_log10mthresh"]
        hi = np.zeros_like(target) + p["hod_bisection_search_max_log10mthresh"]
        out = np.zeros_like(target)
        active = np.ones(S, dtype=bool)
        n_iter, warned = 0, False
        while active.any():
            mid = np.where(active[:, None], (lo + hi) / 2.0, out)
            got = self._hodens_occ(ctx, d_par, 0, mid, S)[1].numpy()
            miss = (got - target) / target
            out[active] = mid[active]
            bisection_step(lo, hi, mid, miss, active)
            active &= np.any(np.abs(miss) > p["hod_bisection_search_rtol"], axis=1)
            n_iter += 1
            if n_iter > p["hod_bisection_search_warn_iter"] and not warned:
                print("WARNING: Bisection search has done more than ", p["hod_bisection_search_warn_iter"],
                      " loops. Still searching...")
                warned = True
        return out, n_iter

    def _hodens_thresholds(self, ctx, d_par, l10, target):
        """The log10 thresholds of a request as add_hod forms them, and the bisection's launches."""
        if l10 is not None:
            return l10, 0
        lm, n_iter = self._hodens_bisect(ctx, d_par, target)
        return np.log10(10 ** (lm * self.p["hod_A_log10mthresh"])), n_iter

    def _hodens_tensor(self, name, what):
        if name in self.pk_profiles and name not in self.uk_profiles:
            raise ValueError(f"{what} {name!r} is a pressure profile: an HOD ensemble takes matter profiles")
        if name not in self.uk_profiles:
            raise ValueError(f"{what} {name!r} is not a matter profile of this model")
        return name

    def hod_ensemble_device(self, sets, mthresh=None, ngal=None, corr="max", satellite_profile_name="nfw", matter_name=None,
                            kindex=None, damping=True, parts=False):
        """P_gg and P_gm of S HOD parameter sets at once, on the device: a hod_ensemble.HodEnsembleResult with power
        (4, S, nz, n) = (P1h_gg, P2h_gg, P1h_gm, P2h_gm), ngal, bg and log10mthresh (S, nz) and parts (3, S, nz, n) =
        (G, X, I) or None.  sets: (S, 6) as hod_ensemble.hod_sets makes them; exactly one of mthresh and ngal, each (nz,),
        shared by the sets, or (S, nz) - ngal runs one batched bisection whose thresholds are those add_hod(ngal=...)
        finds for each set alone.  Plane by plane the result is get_power_1halo / get_power_2halo of (g_s, g_s) and
        (g_s, matter_name) for g_s = add_hod(mthresh=..., corr=corr, satellite_profile_name=..., param_override=set s)
        without a central profile; matter_name defaults to the satellite profile.  kindex: the nodes of the k grid
        (default: all); damping as in get_power_1halo.  Nothing is registered in hods; cached spectra stay valid."""
        sets, flag, l10, target = self._hodens_request(sets, mthresh, ngal, corr)
        sat = self._hodens_tensor(satellite_profile_name, "satellite_profile_name")
        mat = sat if matter_name is None else self._hodens_tensor(matter_name, "matter_name")
        nz, nm, nk = self._nz, self._nm, self._nk
        kindex = check_kindex(kindex, nk)
        S, n = sets.shape[0], nk if kindex is None else kindex.size
        nodes = self.ks if kindex is None else self.ks[kindex]
        damp = bispec.damping(nodes, self.p["kstar_damping"]) if damping else np.ones(n)
        ctx = self._main(needs_aux=True)
        shape = (nz, nm, nk)
        # (another reader of the tensors than the batched mass integrals: a deferred left fill is written first)
        d_us = self.uk_profiles.dev(sat, fill=True)
        d_um = d_us if mat == sat else self.uk_profiles.dev(mat, fill=True)
        for nm_, d_ in ((sat, d_us), (mat, d_um)):
            if d_.shape != shape:
                raise ValueError(f"profile {nm_!r} has shape {d_.shape}, the model's grid is {shape}")
        d_par = ctx.upload(sets)
        l10, n_iter = self._hodens_thresholds(ctx, d_par, l10, target)
        coef = ctx.empty((coef_block_size(S, nz, nm),))
        d_thr, d_ngal, d_bg = self._hodens_occ(ctx, d_par, flag, l10, S, coef=coef)
        d_k = None if kindex is None else ctx.upload_int32(kindex)
        d_damp = ctx.upload(np.ascontiguousarray(damp, dtype=np.float64))
        out = ctx.empty((4, S, nz, n))
        P = ctx.empty((3, S, nz, n)) if parts else None
        ctx.call("hmg_hod_ensemble_power", S=S, nz=nz, nm=nm, nk=nk, n=n, d_us=d_us.ptr, d_um=d_um.ptr, d_coef=coef.ptr,
                 d_ngal=d_ngal.ptr, d_bg=d_bg.ptr, **self._model_block("hmg_hod_ensemble_power"), d_kindex=nat.ptr(d_k),
                 d_damp=d_damp.ptr, d_out=out.ptr, d_parts=nat.ptr(P))
        self._sync_point()
        return HodEnsembleResult(out, d_ngal, d_bg, d_thr, P, n_iter)

    def get_power_hod_ensemble(self, sets, mthresh=None, ngal=None, corr="max", satellite_profile_name="nfw",
                               matter_name=None, kindex=None, damping=True, parts=False):
        """hod_ensemble_device on the host: a dict of gg_1h, gg_2h, gg, gm_1h, gm_2h, gm, each (S, nz, n), and ngal, bg,
        log10mthresh (S, nz); with parts=True also G, X, I (S, nz, n)."""
        r = self.hod_ensemble_device(sets, mthresh=mthresh, ngal=ngal, corr=corr,
                                     satellite_profile_name=satellite_profile_name, matter_name=matter_name, kindex=kindex,
                                     damping=damping, parts=parts)
        power = r.power.numpy()
        out = dict(zip(POWER_KEYS, power))
        out["gg"], out["gm"] = power[0] + power[1], power[2] + power[3]
        out["ngal"], out["bg"], out["log10mthresh"] = r.ngal.numpy(), r.bg.numpy(), r.log10mthresh.numpy()
        if parts:
            out.update(zip(("G", "X", "I"), r.parts.numpy()))
        return out

    def hod_ensemble_occupations(self, sets, mthresh=None, ngal=None, corr="max"):
        """{Nc, Ns, NsNsm1, NcNs (S, nz, nm), ngal, bg (S, nz)}: the occupation numbers and sums of every set, each the
        bits add_hod gives for that set alone."""
        sets, flag, l10, target = self._hodens_request(sets, mthresh, ngal, corr)
        S = sets.shape[0]
        ctx = self._main(needs_aux=True)
        d_par = ctx.upload(sets)
        l10, _ = self._hodens_thresholds(ctx, d_par, l10, target)
        occ = ctx.empty((4, S, self._nz, self._nm))
        _, d_ngal, d_bg = self._hodens_occ(ctx, d_par, flag, l10, S, occ=occ)
        self._sync_point()
        out = dict(zip(("Nc", "Ns", "NsNsm1", "NcNs"), occ.numpy()))
        out["ngal"], out["bg"] = d_ngal.numpy(), d_bg.numpy()
        return out
