"""Host model of the analytic NFW transform u(k|m,z) (hmvec_amd/csrc/kernels/nfw.hpp, ``nfw_rows``) that
tests/test_nfw_cpu.py, tests/test_gpu_nfw_bands.py and tests/test_gpu_fuzz.py share.  mpmath and numpy only; the one
repository source it reads is sici.hpp, for the Cephes coefficient tables of ``sici_table_host``.

* ``band(c, x)``: which of the kernel's nine evaluation forms a point takes - the kernel's tests in the kernel's order on
  the float64 ``xc = (1.0 + c) * x``.  The collapsed form splits by the ``sici_aux`` branches of its two arguments:
  ``col<8`` both rationals of [4, 8), ``col<64`` neither argument on the asymptotic series, ``col≥64`` the asymptotic
  series for xc at least (x <= xc, so this holds all of x >= 64 and the rows where only xc has crossed).
* ``u_mpmath(c, x)``: the closed form at 40 digits, c and x the exact doubles, xc = (1 + c) x exact.
* ``budget(c, x)``: (B, S).  B = 2^-52 (|u| + |x du/dx| + |c du/dc|) is what no float64 evaluation avoids (rounding of
  the result and of x, c, 1 + c, c x and xc ahead of sin, cos, f and g); S = 2^-52 (|sin x| (|Si xc| + |Si x|) +
  |sin cx / xc| + |cos x| (|Ci xc| + |Ci x|)) / m_c is the size of the terms the closed form itself subtracts.
* ``restate(c, x)``: each band as the kernel writes it - same formula, same tables, same recurrence for the series row -
  in correctly rounded double operations: no FMA, no fast reciprocal, sine, cosine or logarithm.
* ``K[band]``: the gate, |u - u_mpmath| <= K B (K S in the closed band).  K is 4 x the worst error of the RESTATEMENT
  over ``point_set()`` in units of B (S), rounded up, at least 8 - measured on the reference side, never on the kernel.
  The factor 4 is for what the kernel does differently: FMA contraction, one ~1 ulp reciprocal shared between
  quotients, a sincos of 1 ulp + 2e-16 and a short logarithm.
* ``point_set()`` / ``table()``: the fixed (c, x) points and everything above evaluated on them, once per process.
"""
import functools
import math
import os
import re
from fractions import Fraction

import mpmath as mp
import numpy as np

BANDS = ("s5", "s8", "s16", "s32", "col<8", "col<64", "col≥64", "mixed", "closed")
EPS = 2.0 ** -52
DPS = 40

# Worst |restate - u_mpmath| / B (/ S in the closed band) over point_set() (1613 points: ten concentrations x 131
# wavenumbers, the neighbours of every band boundary, the col<8 fill, the two sides of xc = 1e9 and two points beyond), measured on
# 2026-10-20 with mpmath 1.3.0, and K = max(8, ceil(4 x worst)).  tests/test_nfw_cpu.py fails if the restatement
# leaves K / 4.
# The worst points: the collapsed forms at c = 0.1 (1/m_c = 227) with x next to 4, 8 and 64, the 32-term series at
# c = 2.5, xc = 10, the mixed form at c = 5, x = 3.98, the closed form at c = 0.1, x = 3.16.  INVFACT here is the
# correctly rounded 1/(2n+1)!; five of the kernel's literals are its neighbours.
RESTATE_WORST = {"s5": 0.250, "s8": 0.250, "s16": 0.507, "s32": 26.0, "col<8": 91.9, "col<64": 88.2, "col≥64": 25.4,
                 "mixed": 26.1, "closed": 6.05}
K = {b: max(8, math.ceil(4.0 * w)) for b, w in RESTATE_WORST.items()}
assert K == {"s5": 8, "s8": 8, "s16": 8, "s32": 104, "col<8": 368, "col<64": 353, "col≥64": 102, "mixed": 105,
             "closed": 25}

NFW_XS1, NFW_XS2, NFW_X1, NFW_X2, SICI_X, SICI_MID_X, SICI_ASYM_X, CODY_WAITE_X = 0.1, 0.8, 4.0, 10.0, 4.0, 8.0, 64.0, 1.0e9
NFW_NT1, NFW_NT2, NFW_NS, NFW_NS2 = 5, 8, 16, 32
EULER_GAMMA, HALF_PI = float(np.euler_gamma), 0.5 * math.pi


# ---------------------------------------------------------------- the kernel's band ladder
def band(c, x):
    """Name of the form nfw_rows evaluates at concentration c and x = ks * rs * (1 + z) (both float64)."""
    c, x = float(c), float(x)
    xc = (1.0 + c) * x
    series = c >= 0.5                              # a[row][0] of nfw_series_row
    if series and xc <= NFW_X1:
        return "s5" if xc <= NFW_XS1 else "s8" if xc <= NFW_XS2 else "s16"
    if series and xc <= NFW_X2:
        return "s32"
    if x > SICI_X and xc < CODY_WAITE_X:
        return "col<8" if xc < SICI_MID_X else "col<64" if xc < SICI_ASYM_X else "col≥64"
    if x <= SICI_X and xc > SICI_MID_X:
        return "mixed"
    return "closed"


def bands(c, x):
    """band() over broadcast arrays: an array of indices into BANDS."""
    c, x = np.broadcast_arrays(np.asarray(c, dtype=np.float64), np.asarray(x, dtype=np.float64))
    xc = (1.0 + c) * x
    series = c >= 0.5
    col = np.where(xc < SICI_MID_X, 4, np.where(xc < SICI_ASYM_X, 5, 6))
    short = np.where(xc <= NFW_XS1, 0, np.where(xc <= NFW_XS2, 1, 2))
    out = np.full(c.shape, 8)
    out = np.where((x <= SICI_X) & (xc > SICI_MID_X), 7, out)
    out = np.where((x > SICI_X) & (xc < CODY_WAITE_X), col, out)
    out = np.where(series & (xc <= NFW_X2), 3, out)
    return np.where(series & (xc <= NFW_X1), short, out)


# ---------------------------------------------------------------- 40-digit reference and the budgets
def _u(c, x):
    """The closed form at the working precision in force (c, x: mpf)."""
    xc = (1 + c) * x
    return (mp.sin(x) * (mp.si(xc) - mp.si(x)) - mp.sin(c * x) / xc + mp.cos(x) * (mp.ci(xc) - mp.ci(x))) \
        / (mp.log1p(c) - c / (1 + c))


def u_mpmath(c, x):
    with mp.workdps(DPS):
        return +_u(mp.mpf(float(c)), mp.mpf(float(x)))


def budget(c, x):
    """(B, S) as floats; S is the gate's unit in the closed band only, B everywhere else."""
    with mp.workdps(DPS + 20):
        cm, xm = mp.mpf(float(c)), mp.mpf(float(x))
        u = _u(cm, xm)
        ux = mp.diff(lambda t: _u(cm, t), xm)
        uc = mp.diff(lambda t: _u(t, xm), cm)
        B = EPS * (abs(u) + abs(xm * ux) + abs(cm * uc))
        xc = (1 + cm) * xm
        S = EPS * (abs(mp.sin(xm)) * (abs(mp.si(xc)) + abs(mp.si(xm))) + abs(mp.sin(cm * xm) / xc)
                   + abs(mp.cos(xm)) * (abs(mp.ci(xc)) + abs(mp.ci(xm)))) / (mp.log1p(cm) - cm / (1 + cm))
        return float(B), float(S)


# ---------------------------------------------------------------- the restatement
def _tables():
    """The arrays of sici_table_host, from its `static const double hXX[n] = {...}` lines."""
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "hmvec_amd", "csrc", "sici.hpp")
    with open(src) as f:
        text = f.read()
    T = {}
    for name, n, body in re.findall(r"static const double h(\w+)\[(\d+)\]\s*=\s*\{([^}]*)\}", text):
        T[name] = [float(v) for v in body.split(",")]
        assert len(T[name]) == int(n), name
    want = {"SN": 6, "SD": 6, "CN": 6, "CD": 6, "FN4": 7, "FD4": 7, "GN4": 8, "GD4": 7, "FN8": 9, "FD8": 8, "GN8": 9,
            "GD8": 9, "AF": 8, "AG": 9}
    assert {k: len(v) for k, v in T.items()} == want, sorted(T)
    return T


T = _tables()
INVFACT = [float(Fraction(1, math.factorial(2 * n + 1))) for n in range(NFW_NS2)]
NFW_NQ, NFW_CQ = 10, 1.5          # nfw_series_row: a_1 .. a_10 of a row with c < 1.5 come from quadrature


def _gauss16():
    """The positive nodes of the 16-point Gauss-Legendre rule and their weights, correctly rounded."""
    with mp.workdps(40):
        xs = [mp.findroot(lambda t: mp.legendre(16, t), mp.mpf(float(x)))
              for x in np.polynomial.legendre.leggauss(16)[0][8:]]
        ws = [2 * (1 - x * x) / (16 * (x * mp.legendre(16, x) - mp.legendre(15, x))) ** 2 for x in xs]
        return [float(x) for x in xs], [float(w) for w in ws]


GAUSS_X, GAUSS_W = _gauss16()


def horner(x, c):
    """horner_s: c[0] x^(n-1) + ... + c[n-1]."""
    a = c[0] * x + c[1]
    for v in c[2:]:
        a = a * x + v
    return a


def horner1(x, c):
    """horner1_s: the same with a leading coefficient 1 in front of c."""
    a = x + c[0]
    for v in c[1:]:
        a = a * x + v
    return a


def series_row(c):
    """nfw_series_row: a_n = (-1)^n J_(2n+1)(c) / ((2n+1)! m_c) by J_p = c^(p-1)/(p-1) - 2 J_(p-1) - J_(p-2)."""
    opc = 1.0 + c
    mc = math.log(opc) - c / opc
    inv_mc = 1.0 / mc
    jm2, jm1, cp = c / opc, mc, c
    a = [1.0] * NFW_NS2
    for p in range(2, 2 * NFW_NS2):
        jp = cp * (1.0 / (p - 1)) - 2.0 * jm1 - jm2
        cp *= c
        if p & 1:
            n = (p - 1) >> 1
            a[n] = (-jp if n & 1 else jp) * INVFACT[n] * inv_mc
        jm2, jm1 = jm1, jp
    if 0.5 <= c < NFW_CQ:
        # the low moments J_3 .. J_(2 NFW_NQ + 1) from the 16-point Gauss-Legendre rule on [0, c] instead
        h = 0.5 * c
        acc = [0.0] * NFW_NQ
        for i in range(16):
            t = h * (-GAUSS_X[i >> 1] if i & 1 else GAUSS_X[i >> 1]) + h
            d, t2 = 1.0 + t, t * t
            pw = (h * GAUSS_W[i >> 1]) / (d * d) * t
            for n in range(NFW_NQ):
                pw *= t2
                acc[n] += pw
        for n in range(1, NFW_NQ + 1):
            a[n] = (-acc[n - 1] if n & 1 else acc[n - 1]) * INVFACT[n] * inv_mc
    return a


def sici_aux(x, z, want_f=True):
    """f(x), g(x) of Si/Ci for x > 4, z = 1/x^2."""
    if x >= SICI_ASYM_X:
        return ((x * z) * horner(z, T["AF"]) if want_f else 0.0), z * horner(z, T["AG"])
    s = "4" if x < SICI_MID_X else "8"
    gn, gd = z * horner(z, T["GN" + s]), horner1(z, T["GD" + s])
    if not want_f:
        return 0.0, gn * (1.0 / gd)
    fn, fd = horner(z, T["FN" + s]), x * horner1(z, T["FD" + s])
    r = 1.0 / (fd * gd)
    return fn * (gd * r), gn * (fd * r)


def sici_fast(x, sx, cx, z):
    """(si, ci, small) of the closed band: for x <= 4, ci is Ci(x) - gamma - ln x."""
    if x <= SICI_X:
        x2 = x * x
        sd, cd = horner(x2, T["SD"]), horner(x2, T["CD"])
        r = 1.0 / (sd * cd)
        return x * horner(x2, T["SN"]) * (cd * r), x2 * horner(x2, T["CN"]) * (sd * r), True
    f, g = sici_aux(x, z)
    return HALF_PI - f * cx - g * sx, f * sx - g * cx, False


def restate(c, x, which=None):
    """u(c, x) by the form of band(c, x) (or of `which`), in plain double arithmetic."""
    c, x = float(c), float(x)
    which = which or band(c, x)
    opc = 1.0 + c
    xc = opc * x
    if which in ("s5", "s8", "s16", "s32"):
        n = {"s5": NFW_NT1, "s8": NFW_NT2, "s16": NFW_NS, "s32": NFW_NS2}[which]
        return horner(x * x, series_row(c)[n - 1::-1])
    ln_opc = math.log(opc)
    inv_mc = 1.0 / (ln_opc - c / opc)
    inv_opc2 = 1.0 / (opc * opc)
    if which.startswith("col"):
        zx = 1.0 / (x * x)
        zc = zx * inv_opc2
        _, g1 = sici_aux(x, zx, want_f=False)
        f2, g2 = sici_aux(xc, zc)
        sd, cd = math.sin(c * x), math.cos(c * x)
        return (g1 + (f2 - xc * zc) * sd - g2 * cd) * inv_mc
    if which == "mixed":
        s1, c1, sd, cd = math.sin(x), math.cos(x), math.sin(c * x), math.cos(c * x)
        x2 = x * x
        zc = (1.0 / x2) * inv_opc2
        sden, cden = horner(x2, T["SD"]), horner(x2, T["CD"])
        r = 1.0 / (sden * cden)
        si = x * horner(x2, T["SN"]) * (cden * r)
        ci = (EULER_GAMMA + math.log(x)) + x2 * horner(x2, T["CN"]) * (sden * r)
        f2, g2 = sici_aux(xc, zc)
        return (HALF_PI * s1 + (f2 - xc * zc) * sd - g2 * cd - s1 * si - c1 * ci) * inv_mc
    s1, c1, s2, c2 = math.sin(x), math.cos(x), math.sin(xc), math.cos(xc)
    zx = 1.0 / (x * x)
    zc = zx * inv_opc2
    si1, ci1, sm1 = sici_fast(x, s1, c1, zx)
    si2, ci2, sm2 = sici_fast(xc, s2, c2, zc)
    dci = ci2 - ci1
    if sm1:
        dci += ln_opc if sm2 else -(EULER_GAMMA + math.log(x))
    scx = s2 * c1 - c2 * s1
    return (s1 * (si2 - si1) - scx * (xc * zc) + c1 * dci) * inv_mc


# ---------------------------------------------------------------- the fixed point set
CS = (0.1, 0.3, float(np.nextafter(0.5, 0.0)), 0.5, 1.0, 2.5, 5.0, 11.0, 30.0, 100.0)
XC_EDGES = (0.1, 0.8, 4.0, 8.0, 10.0, 64.0)
X_EDGES = (4.0, 8.0, 64.0)


def _around_xc(opc, b):
    """The x on the two sides of the float64 test `opc * x <= b`: the largest with opc * x < b, the smallest with
    opc * x > b and, where the product can hit it, one with opc * x == b."""
    x = b / opc
    while opc * x >= b:
        x = float(np.nextafter(x, 0.0))
    while opc * float(np.nextafter(x, np.inf)) < b:
        x = float(np.nextafter(x, np.inf))
    out = [x]
    x = float(np.nextafter(x, np.inf))
    if opc * x == b:
        out.append(x)
        while opc * x == b:
            x = float(np.nextafter(x, np.inf))
    out.append(x)
    return out


@functools.lru_cache(maxsize=None)
def point_set():
    """The (c, x) pairs, as two float64 arrays sorted by (c, x) without repeats."""
    pts = set()
    for c in CS:
        opc = 1.0 + c
        pts.update((c, float(x)) for x in np.geomspace(1e-5, 1e8, 131))
        for b in XC_EDGES:
            pts.update((c, x) for x in _around_xc(opc, b))
        for b in X_EDGES:
            pts.update((c, float(x)) for x in (np.nextafter(b, 0.0), b, np.nextafter(b, np.inf)))
        if opc * SICI_X < SICI_MID_X:
            # col<8 is the window 4 < x, (1+c) x < 8 of the rows with c < 1: the geometric grid puts two or three
            # points of a row there, so eight evenly spaced ones fill it up to the 30 every band must have
            pts.update((c, float(x)) for x in np.linspace(SICI_X, SICI_MID_X / opc, 10)[1:-1])
    # beyond the Cody-Waite range of sincos_fast: the last xc < 1e9 of a row (still collapsed) and its first xc >= 1e9,
    # one mid-range, one at the far end
    pts.update((5.0, x) for x in _around_xc(6.0, CODY_WAITE_X)[:2] + [5.0e9, _around_xc(6.0, 1.0e12)[0]])
    pts = sorted(pts)
    return np.array([p[0] for p in pts]), np.array([p[1] for p in pts])


class Table:
    """point_set() with its band, the 40-digit u, the budgets and the restatement at every point."""

    def __init__(self):
        self.c, self.x = point_set()
        self.band = np.array([band(c, x) for c, x in zip(self.c, self.x)])
        self.u = [u_mpmath(c, x) for c, x in zip(self.c, self.x)]
        BS = np.array([budget(c, x) for c, x in zip(self.c, self.x)])
        self.B, self.S = BS[:, 0], BS[:, 1]
        self.unit = np.where(self.band == "closed", self.S, self.B)       # the gate is K[band] * unit
        self.K = np.array([K[b] for b in self.band], dtype=np.float64)
        self.restated = np.array([restate(c, x) for c, x in zip(self.c, self.x)])
        counts = {b: int(np.sum(self.band == b)) for b in BANDS}
        assert set(self.band) <= set(BANDS) and min(counts.values()) >= 30, counts

    def err(self, got, u=None):
        """|got - u_mpmath| per point, the difference taken at 40 digits."""
        with mp.workdps(DPS):
            return np.array([float(abs(mp.mpf(float(g)) - r)) for g, r in zip(got, self.u if u is None else u)])

    def worst(self, got):
        """{band: worst |got - u_mpmath| / unit} over the set."""
        ratio = self.err(got) / self.unit
        return {b: float(np.max(ratio[self.band == b])) for b in BANDS}


@functools.lru_cache(maxsize=None)
def table():
    return Table()


def reference(cs, xs):
    """(u as mpf, gate as floats) of arbitrary points - for grids that are not the point set."""
    u = [u_mpmath(c, x) for c, x in zip(cs, xs)]
    BS = np.array([budget(c, x) for c, x in zip(cs, xs)])
    bd = [band(c, x) for c, x in zip(cs, xs)]
    gate = np.array([K[b] * (bs[1] if b == "closed" else bs[0]) for b, bs in zip(bd, BS)])
    return u, gate, np.array(bd)
