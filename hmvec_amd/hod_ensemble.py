"""HOD parameter ensembles.

``HaloModel.hod_ensemble_device`` / ``get_power_hod_ensemble`` give P_gg and P_gm of many HOD parameter sets at once
against one mass function and one pair of profile tensors; ``HaloModel.hod_ensemble_occupations`` gives their occupation
numbers.  This module holds the host side - plain data and arithmetic, no library calls: the table of parameter sets,
the central-difference stencil of a Fisher forecast and its derivatives, the checks of a request and the layout of the
coefficient block the two native calls share.
"""
import numpy as np

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
