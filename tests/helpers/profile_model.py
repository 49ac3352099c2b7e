"""The radial-profile transform (hmvec/fft.py:35-115 as oracle/hmref.py:183-212 restates it, quirks kept) as a 40-digit
discrete reference with an error scale, the row sets that reach every branch of the row kernels, and the gates - shared by
tests/test_profile_model_cpu.py (pins the model, measures the constants) and tests/test_gpu_profile_rows.py (holds every
route of hmg_profile_fft, hmg_profile_fft_table and hmg_sine_transform to it).  DESIGN.md section 30.

The operation.  Inputs are the float64 arrays and scalars handed to the C entry point, taken as exact.  Per sample
rho_n = amp t^gamma (1 + t^alpha)^(-expo), t = x_n / xc (or a table entry); theta_n = 0 where |x_n| > cmax, else 1 (a
sample at equality is kept); y_n = x_n rho_n theta_n; mnorm = trapz(theta rho x^2, xs) with do_mass_norm, else 1;
F_j = sum_{n<N} y_n sin(2 pi j n / N) (phase index from 0 while x starts at dx); u_j = step F_j / kts[j] / mnorm,
j = 1..M = N // 2 (for even N the table entry sin(pi n) is exactly 0, so u_M = 0 exactly); kout_j = kts[j] / rss / (1+z);
out(k) = np.interp(ks, kout[1:], u[1:], left=u_1, right=0) * post.  np.interp decides its two fills on the float64 kout
array, so the model does: k < fl(kout_1) takes u_1, k > fl(kout_M) takes 0, where fl(kout_j) is numpy's
(kts[j] / rss) / (1 + z).  Everything between is the exact piecewise-linear function through the exact (kout_j, u_j); it
is continuous at both fills (for even N), so the float decision costs nothing there.

The arithmetic.  Sample values come from mpmath at DPS digits.  The sums over n run in integers: y_n and the one table
sin(2 pi r / N), cos(2 pi r / N), r < N, are scaled by powers of two to ~DPS 3.33 + 64 bits and truncated, j n is
reduced mod N in integers, and the products are added exactly.  A row that needs few modes gets the direct sum; a row
where the direct sum would cost more gets a mixed-radix transform (smallest prime factor first; 2, 3, 5 for every
length of the row sets that takes it) in the same integers.  tests/test_profile_model_cpu.py checks both against an
mpmath-only direct sum and checks 40 against 60 digits.  References are kept as hi + lo float64 pairs
(helpers/math_probe.py): err = |(got - hi) - lo|.

The scale S: what no float64 evaluation of this form avoids, in units of 2^-52.
  w_n = 1 + |gamma l_n| + expo [log1p(tau_n) + |alpha l_n| tau_n / (1 + tau_n)], l_n = ln(x_n / xc), tau_n = t^alpha:
  one rounding in each of l, alpha l, the log1p and the outer exponent, carried to rho (d rho / rho = d(exponent); the
  rounding of alpha l reaches log1p(tau) with the factor tau / (1 + tau)).  Table variant: w_n = 1.
  Without the norm  S_j = step sum_n |y_n| w_n / kts[j].
  With it, u = A / m, A = step F / kt, m = sum_n g_n, g_n = theta rho_n x_n^2 D_n (D_n the trapezoid weight):
      du = dA / m - A dm / m^2,   |dA| <= eps step sum |y_n| w_n / kt,   |dm| <= eps sum |g_n| w_n,
      |A| <= step sum |y_n| / kt,
  hence  S_j = step / (kts[j] |m|) * [ sum |y_n| w_n  +  sum |y_n| * (sum |g_n| w_n / |m|) ]
  - the issue's "S_j sum|theta rho x^2 D| / |mnorm|" with the weights w_n kept where the derivation puts them (equal to
  it for constant w_n; for a positive profile sum |g_n| = |m|).
  At a target between modes j and j + 1 with weight f:  S(k) = (1 - f) S_j + f S_{j+1} + j |u_{j+1} - u_j| - the last
  term is the mode position (kts[1], 1 / (rss (1+z)) and k / k_lo are each rounded once: f moves by j eps).  A target
  whose f lies within KNOT j eps of 0 or 1 sits on a knot to that rounding and may be interpolated in either bracket
  (the one-row kernels place mode j at j k_lo and do take the other one): there the term is j times the larger of the two
  adjacent |u_{j+1} - u_j|.  T1 puts every target on a knot.
  Left fill: S_1.  Beyond fl(kout_M): the reference is 0, S = 0 and the device must return 0 exactly.

The gate:  |out - ref| <= K[route] 2^-52 S(k) |post|.  K[route] = 4 x the worst ratio the float64 numpy restatement
below (np.log / np.exp / np.log1p in the kernel's exp-log form, np.fft.rfft, trapezoid, np.interp) reaches over that
route's whole row set, measured on the CPU - never from a device's output.  The factor 4 is DESIGN.md section 8's: the
device's log, exp and log1p are stated at < 2 ulp where numpy's are below 1, and it rounds Im F * sc * rj and the
interpolation FMA separately.  Every K must lie below the operation-count bound 2 log2 N + 8, else S is wrong.
tests/test_profile_model_cpu.py re-measures: the restatement must be inside K / 4 and above K / 16.
"""
import atexit
import collections.abc
import ctypes
import dataclasses
import functools
import os
import shutil
import subprocess
import tempfile
from fractions import Fraction

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
EPS = 2.0 ** -52
KNOT = 8.0      # a target with weight f within KNOT j 2^-52 of 0 or 1 counts as on the knot (mode-position term)
DPS = 40
FFT_MAX_PASSES = 16

# K[route] = 4 x MEASURED[route]: the numpy restatement's worst |err| / (2^-52 S |post|) over every row set of the route
# (measured with numpy 2.2.6 / mpmath 1.3.0 by tests/test_profile_model_cpu.py::test_restatement_sits_inside_its_constants,
# which prints them).
MEASURED = {"spec2500": 0.219,      # nxs = 5000 gas T1 (alpha = 1 member 0.079; cconst 0.068)
            "ct": 0.150,            # nxs = 3000 T2 (1000: 0.144, 2000: 0.087, 4000: 0.071, 6000: 0.115)
            "rt": 0.157,            # nxs = 600 T1 (5400: 0.156, 30: 0.116, 16: 0.058; 16 without norm, with post: 0.129)
            "pruned": 0.198,        # nxs = 10000 T1 (25000: 0.186, 30000: 0.138)
            "chirp": 0.138,         # nxs = 30000 T2
            "band": 0.049,          # nxs = 30000 / xmax = 2, two rows
            "rocfft": 0.260,        # nxs = 7000 T2 (45: 0.151, 14: 0.074)
            "table": 0.983,         # nxs = 5000 shared table T1 (1000: 0.857; T2: 0.45-0.64) - w_n = 1 and a seeded
                                    # non-smooth table: the mode-position term carries S at high j
            "sine": 0.535}          # n = 600 (5000: 0.269)
K = {route: 4.0 * worst for route, worst in MEASURED.items()}
assert K == {"spec2500": 0.876, "ct": 0.6, "rt": 0.628, "pruned": 0.792, "chirp": 0.552, "band": 0.196, "rocfft": 1.04,
             "table": 3.932, "sine": 2.14}


def count_bound(n):
    return 2.0 * np.log2(n) + 8.0


# ---------------------------------------------------------------- the plan the kernels use (tests/cpp/ldsfft_host.cpp)
@functools.lru_cache(maxsize=None)
def _planlib():
    tmp = tempfile.mkdtemp(prefix="ldsfft_plan_")
    atexit.register(shutil.rmtree, tmp, ignore_errors=True)
    out = os.path.join(tmp, "libldsfft_host.so")
    src = os.path.join(TESTS, "cpp", "ldsfft_host.cpp")
    subprocess.run(["g++", "-O0", "-std=c++17", "-shared", "-fPIC", src, "-o", out], check=True)
    lib = ctypes.CDLL(out)
    lib.ldsfft_plan.argtypes = [ctypes.c_int, ctypes.c_void_p]
    lib.ldsfft_plan.restype = ctypes.c_int
    return lib


@functools.lru_cache(maxsize=None)
def plan_radices(M):
    """The radices of the host plan builder's length-M plan (fft_plan_fill), () when it has none."""
    rad = (ctypes.c_int * FFT_MAX_PASSES)()
    n = _planlib().ldsfft_plan(int(M), rad)
    return tuple(rad[i] for i in range(n))


def input_predicates(xs, cmax, nxs):
    """`pruned` and `lead3` of profile_fused_row for one row, restated from xs, cmax and the plan's first radix."""
    M = nxs // 2
    rad = plan_radices(M) if nxs % 2 == 0 and M >= 4 else ()
    if not rad:
        return {"pruned": False, "lead3": False}
    stride0 = M // rad[0]
    pruned = len(rad) > 1 and bool(xs[2 * stride0] > cmax)
    lead3 = M == 2500 and pruned and bool(xs[2 * 375] > cmax)
    return {"pruned": pruned, "lead3": lead3}


def output_predicates(kts, rss, z, ks, nxs, hints):
    """`jn`, `nleft` and the last pass's `keep` of profile_fused_row for one row (float64, the kernel's own operations)."""
    M = nxs // 2
    isc0 = 1.0 / (rss * (1.0 + z))
    klo0 = kts[1] * isc0
    idk0 = 1.0 / klo0
    jn, nleft, capped = M, 0, True
    if hints:
        tmax = ks[-1] * idk0
        if tmax < float(M - 4):
            jn, capped = int(tmax) + 3, False
        nleft = int(np.count_nonzero(ks < klo0))
    rad = plan_radices(M) if nxs % 2 == 0 and M >= 4 else ()
    keep = bool(rad) and 2 * jn + 2 < M // rad[-1]
    return {"jn": jn, "nleft": nleft, "keep": keep, "capped": capped, "beyond": bool(np.any(ks > kts[M] * isc0))}


# ---------------------------------------------------------------- a call of the entry point
@dataclasses.dataclass
class Case:
    name: str
    route: str
    nxs: int
    xmax: float
    cmax: np.ndarray                 # (nz, nm)
    rss: np.ndarray                  # (nz, nm)
    zs: np.ndarray                   # (nz,)
    ks: np.ndarray
    hints: bool
    amp: object = None               # (nz, nm) arrays or None = the constant
    xc: object = None
    alpha: object = None
    expo: object = None
    amp_c: float = 1.0
    xc_c: float = 1.0
    alpha_c: float = 1.0
    expo_c: float = 1.0
    gamma: float = -0.2
    do_norm: int = 1
    post: object = None
    logx: bool = False
    table: object = None             # (1, nxs) or (nz nm, nxs): hmg_profile_fft_table
    env: dict = dataclasses.field(default_factory=dict)     # switches of the context that runs the named route
    off: dict = dataclasses.field(default_factory=dict)     # ... of the context that must not run it
    off_equal: bool = False          # the `off` context runs the same route (rocFFT rows: the same bits)
    claims: tuple = ()               # what the row set is there to hit (the CPU test asserts each)
    same_as: str = ""                # the case whose rows and targets these are (its reference serves; "-T3": reversed)

    @property
    def shape(self):
        return self.cmax.shape

    @property
    def xs(self):
        return np.linspace(0.0, self.xmax, self.nxs + 1)[1:]

    @property
    def step(self):
        xs = self.xs
        return (xs[-1] - xs[0]) / self.nxs

    @property
    def kts(self):
        return np.fft.rfftfreq(self.nxs, self.step) * 2 * np.pi

    def row_params(self, i, j):
        pick = lambda a, c: float(c) if a is None else float(a[i, j])
        return pick(self.amp, self.amp_c), pick(self.xc, self.xc_c), pick(self.alpha, self.alpha_c), pick(self.expo, self.expo_c)

    def row_table(self, i, j):
        return self.table[0 if self.table.shape[0] == 1 else i * self.shape[1] + j]

    def reversed(self, name):
        """The same rows on the reversed target grid without hint arrays: the per-target path."""
        return dataclasses.replace(self, name=name, ks=self.ks[::-1].copy(), hints=False, same_as=self.name, claims=())


# ---------------------------------------------------------------- exact sums in integers
def _bits(dps):
    return int(dps * 3.33) + 64


def _to_int(v, shift):
    """floor-ish(v 2^shift) of an mpf as a Python int (truncation towards zero)."""
    sign, man, exp, _ = v._mpf_
    e = exp + shift
    m = int(man) << e if e >= 0 else int(man) >> -e
    return -m if sign else m


@functools.lru_cache(maxsize=8)
def _trig_table(N, dps):
    """(cos, sin)(2 pi r / N), r < N, as object arrays of integers scaled by 2^_bits(dps); exact 0, +-1 at the axes."""
    B = _bits(dps)
    with mp.workdps(dps + 25):
        c = np.empty(N, dtype=object)
        s = np.empty(N, dtype=object)
        for r in range(N // 2 + 1):
            q = mp.mpf(2 * r) / N                  # angle / pi
            cr, sr = _to_int(mp.cospi(q), B), _to_int(mp.sinpi(q), B)
            c[r], s[r] = cr, sr
            if r:
                c[N - r], s[N - r] = cr, -sr
    return c, s


def _smallest_factor(n):
    for p in range(2, int(n ** 0.5) + 1):
        if n % p == 0:
            return p
    return n


def _fft_cost(N):
    cost, n = 0, N
    while n > 1:
        p = _smallest_factor(n)
        cost += p
        n //= p
    return cost * N


def _fft_int(xr, xi, N, tstride, C, S, B):
    """Forward DFT X_k = sum_n x_n exp(-2 pi i n k / N) of integer (fixed-point) vectors, decimation in time by the
    smallest prime factor; twiddles exp(-2 pi i t / Ntot) = (C[t], -S[t]) scaled 2^B; products are shifted back by B."""
    if N == 1:
        return xr, xi
    r = _smallest_factor(N)
    m = N // r
    subs = [_fft_int(xr[q::r], None if xi is None else xi[q::r], m, tstride * r, C, S, B) for q in range(r)]
    outr = np.empty(N, dtype=object)
    outi = np.empty(N, dtype=object)
    k = np.arange(m)
    for s in range(r):
        ar = subs[0][0].copy()
        ai = subs[0][1].copy() if subs[0][1] is not None else np.zeros(m, dtype=object)
        for q in range(1, r):
            idx = (q * (k + m * s)) % N * tstride
            tc, ts = C[idx], S[idx]                      # W = tc - i ts
            br, bi = subs[q]
            if bi is None:
                ar = ar + ((br * tc) >> B)
                ai = ai - ((br * ts) >> B)
            else:
                ar = ar + ((br * tc + bi * ts) >> B)
                ai = ai + ((bi * tc - br * ts) >> B)
        outr[s * m:(s + 1) * m] = ar
        outi[s * m:(s + 1) * m] = ai
    return outr, outi


def sine_sums(y, N, modes, dps=DPS, method="auto"):
    """F_j = sum_n y_n sin(2 pi j n / N) for j in `modes` (y: list of mpf, the leading samples of a length-N row whose
    rest is zero), as mpf at `dps`.  method: "direct", "fft" or "auto" (the cheaper of the two)."""
    modes = np.asarray(modes, dtype=np.int64)
    nn = len(y)
    if nn == 0 or modes.size == 0:
        return [mp.mpf(0)] * modes.size
    B = _bits(dps)
    C, S = _trig_table(N, dps)
    with mp.workdps(dps + 25):
        top = max(abs(v) for v in y)
        if top == 0:
            return [mp.mpf(0)] * modes.size
        By = B - int(mp.floor(mp.log(top, 2)))
        Y = np.array([_to_int(v, By) for v in y], dtype=object)
        if method == "auto":
            method = "fft" if _fft_cost(N) * 6 < nn * modes.size else "direct"
        out = []
        if method == "direct":
            n = np.arange(nn, dtype=np.int64)
            for j in modes:
                acc = int(np.dot(Y, S[(int(j) * n) % N]))
                out.append(mp.ldexp(mp.mpf(acc), -(By + B)))
        else:
            full = np.zeros(N, dtype=object)
            full[:nn] = Y
            _, xi = _fft_int(full, None, N, 1, C, S, B)
            for j in modes:
                out.append(mp.ldexp(mp.mpf(-int(xi[int(j) % N])), -By))
    return out


def sine_sums_mpmath(y, N, modes, dps=DPS):
    """The same sums in mpmath arithmetic alone (slow: the CPU test's cross-check at a handful of modes)."""
    out = []
    with mp.workdps(dps + 10):
        for j in modes:
            out.append(mp.fsum(v * mp.sinpi(mp.mpf(2 * ((int(j) * n) % N)) / N) for n, v in enumerate(y)))
    return out


# ---------------------------------------------------------------- samples of one row
@functools.lru_cache(maxsize=8)
def _lnx(nxs, xmax, dps):
    xs = np.linspace(0.0, xmax, nxs + 1)[1:]
    with mp.workdps(dps + 10):
        return [mp.log(mp.mpf(float(x))) for x in xs]


def kept(xs, cmax):
    """theta: np.where(np.abs(xs) > cmax, 0, 1) - a sample at equality is kept."""
    return ~(np.abs(xs) > cmax)


_ROW_CACHE = {}


def row_samples(case, i, j, dps=DPS):
    """(y list of mpf over the kept leading samples, mnorm mpf, A1 = sum|y|w, A0 = sum|y|, G1 = sum|g|w) of row (i, j);
    kept per (grid, row parameters, cmax, norm, digits): the target grids of a row set share their rows."""
    if CASES.get(case.name) is not case:
        return _row_samples(case, i, j, dps)
    tab = None if case.table is None else (id(case.table), 0 if case.table.shape[0] == 1 else i * case.shape[1] + j)
    key = (case.nxs, float(case.xmax), case.row_params(i, j), float(case.gamma), float(case.cmax[i, j]), int(case.do_norm),
           tab, dps)
    if key not in _ROW_CACHE:
        _ROW_CACHE[key] = _row_samples(case, i, j, dps)
    return _ROW_CACHE[key]


def _row_samples(case, i, j, dps):
    xs = case.xs
    keep = kept(xs, case.cmax[i, j])
    nn = int(np.count_nonzero(keep))
    assert np.all(keep[:nn]) and not np.any(keep[nn:])
    with mp.workdps(dps + 10):
        X = [mp.mpf(float(x)) for x in xs[:nn]]
        if case.table is not None:
            rho = [mp.mpf(float(v)) for v in case.row_table(i, j)[:nn]]
            w = np.ones(nn)
        else:
            amp, xc, al, ex = (mp.mpf(v) for v in case.row_params(i, j))
            g = mp.mpf(float(case.gamma))
            lnxc = mp.log(xc)
            lnx = _lnx(case.nxs, float(case.xmax), dps)
            rho, w = [], np.empty(nn)
            for n in range(nn):
                l = lnx[n] - lnxc
                tau = mp.exp(al * l)
                l1 = mp.log1p(tau)
                rho.append(amp * mp.exp(g * l - ex * l1))
                w[n] = float(1 + abs(g * l) + ex * (l1 + abs(al * l) * tau / (1 + tau)))
        y = [X[n] * rho[n] for n in range(nn)]
        ya = np.array([float(abs(v)) for v in y])
        A1, A0 = float(np.sum(ya * w)), float(np.sum(ya))
        if case.do_norm:
            # the trapezoid weights of the uniform float64 grid, exactly
            xf = [mp.mpf(float(x)) for x in xs[:nn + 1]]
            gs = []
            for n in range(nn):
                lo = xf[n - 1] if n > 0 else xf[0]
                hi = xf[n + 1] if n + 1 < case.nxs else xf[n]
                gs.append(rho[n] * X[n] * X[n] * (hi - lo) / 2)
            m = mp.fsum(gs)
            G1 = float(np.sum(np.array([float(abs(v)) for v in gs]) * w))
        else:
            m, G1 = mp.mpf(1), 0.0
    return y, m, A1, A0, G1


def _split(v):
    hi = float(v)
    return hi, float(v - hi)


def kout_float(kts, rss, z):
    return kts / rss / (1 + z)


@functools.lru_cache(maxsize=None)
def _reference_cached(name, dps):
    return _reference(CASES[name], dps)


def reference(case, dps=DPS):
    """{"hi", "lo", "S": (nz, nm, nk); "u1hi", "u1lo", "S1": (nz, nm)} - out = hi + lo, the gate's scale S (without the
    2^-52, with |post|), and the left-fill value u_1 post with its scale.  Cached per case of CASES."""
    if CASES.get(case.name) is not case:
        return _reference(case, dps)
    if case.same_as:
        ref = _reference_cached(case.same_as, dps)
        return {k: v[..., ::-1] for k, v in ref.items() if v.ndim == 3} | {k: v for k, v in ref.items() if v.ndim == 2} \
            if case.name.endswith("-T3") else ref
    return _reference_cached(case.name, dps)


def _reference(case, dps):
    nz, nm = case.shape
    ks, kts, N, M = case.ks, case.kts, case.nxs, case.nxs // 2
    nk = ks.size
    hi, lo, S = np.zeros((nz, nm, nk)), np.zeros((nz, nm, nk)), np.zeros((nz, nm, nk))
    u1hi, u1lo, S1 = np.zeros((nz, nm)), np.zeros((nz, nm)), np.zeros((nz, nm))
    for i in range(nz):
        for j in range(nm):
            y, m, A1, A0, G1 = row_samples(case, i, j, dps)
            rs, z = float(case.rss[i, j]), float(case.zs[i])
            pf = 1.0 if case.post is None else float(case.post[i, j])
            kf = kout_float(kts, rs, z)
            left, right = ks < kf[1], ks > kf[M]
            mid = np.nonzero(~left & ~right)[0]
            br = np.clip(np.searchsorted(kf[1:M + 1], ks[mid], side="right"), 1, max(M - 1, 1))   # kf[br] <= k
            with mp.workdps(dps + 10):
                # the weight of every target first: it decides which neighbours the mode-position term needs
                step, sc = mp.mpf(float(case.step)), mp.mpf(rs) * (1 + mp.mpf(z))
                fs, extra = [], []
                for t, q in zip(mid.tolist(), br.tolist()):
                    q1 = min(q + 1, M)
                    if q1 == q:
                        fs.append(mp.mpf(0))
                        continue
                    k0, k1 = mp.mpf(float(kts[q])) / sc, mp.mpf(float(kts[q1])) / sc
                    f = (mp.mpf(float(ks[t])) - k0) / (k1 - k0)
                    fs.append(f)
                    if abs(f) < KNOT * q * EPS and q > 1:
                        extra.append(q - 1)
                    if abs(1 - f) < KNOT * q * EPS and q1 < M:
                        extra.append(q1 + 1)
                need = np.unique(np.concatenate([[1], br, np.minimum(br + 1, M), np.asarray(extra, dtype=br.dtype)]))
                F = dict(zip(need.tolist(), sine_sums(y, N, need, dps)))
                u = {q: step * F[q] / mp.mpf(float(kts[q])) / m for q in F}
                ma = float(abs(m))
                Sj = lambda q: (float(case.step) / (float(kts[q]) * ma) * (A1 + A0 * G1 / ma)) if case.do_norm else \
                    float(case.step) * A1 / float(kts[q])
                P = mp.mpf(pf)
                u1hi[i, j], u1lo[i, j] = _split(u[1] * P)
                S1[i, j] = Sj(1) * abs(pf)
                hi[i, j, left], lo[i, j, left], S[i, j, left] = u1hi[i, j], u1lo[i, j], S1[i, j]
                for t, q, f in zip(mid.tolist(), br.tolist(), fs):
                    q1 = min(q + 1, M)
                    if q1 == q:                                   # M == 1: a single mode
                        val, s = u[q], Sj(q)
                    else:
                        val = u[q] + (u[q1] - u[q]) * f
                        ff = float(f)
                        # a target within the position's own rounding of a knot may be interpolated in either bracket
                        du = abs(u[q1] - u[q])
                        if abs(f) < KNOT * q * EPS and q > 1:
                            du = max(du, abs(u[q] - u[q - 1]))
                        if abs(1 - f) < KNOT * q * EPS and q1 < M:
                            du = max(du, abs(u[q1 + 1] - u[q1]))
                        s = (1 - ff) * Sj(q) + ff * Sj(q1) + q * float(du)
                    hi[i, j, t], lo[i, j, t] = _split(val * P)
                    S[i, j, t] = s * abs(pf)
    return {"hi": hi, "lo": lo, "S": S, "u1hi": u1hi, "u1lo": u1lo, "S1": S1}


def ratios(got, hi, lo, S):
    """|got - ref| / (2^-52 S), elementwise; where S == 0 (beyond the last mode: the reference is exactly 0) the ratio
    is 0 for an exact 0 and inf for anything else."""
    got = np.asarray(got, dtype=np.float64)
    err = np.abs((got - hi) - lo)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(S > 0, err / (EPS * np.where(S > 0, S, 1.0)), np.where(err == 0, 0.0, np.inf))
    return np.where(np.isfinite(got), r, np.inf)


# ---------------------------------------------------------------- the float64 numpy restatement
_trapz = getattr(np, "trapezoid", None) or np.trapz


def restatement(case, uniform=False):
    """(out (nz, nm, nk), u_1 post (nz, nm)) in plain float64 numpy, the integrand in the kernel's exp / log form.
    uniform: the output side as the one-row kernels run it - the modes on the uniform grid j k_lo, k_lo = kts[1] *
    (1 / (rss (1+z))), the bracket by j = int(k / k_lo), the weight k (1 / k_lo) - j in one rounding (an FMA on the device,
    exact rationals here), u_j as Im F * (-step / mnorm * (1 / kts[1])) * (1 / j) - instead of np.interp on kts / rss / (1+z)."""
    nz, nm = case.shape
    xs, kts, M = case.xs, case.kts, case.nxs // 2
    out, c = np.zeros((nz, nm, case.ks.size)), np.zeros((nz, nm))
    lx = np.log(xs)
    for i in range(nz):
        for j in range(nm):
            if case.table is not None:
                rho = np.asarray(case.row_table(i, j), dtype=np.float64)
            else:
                amp, xc, al, ex = case.row_params(i, j)
                lt = lx - (0.0 if (case.xc is None and case.xc_c == 1.0) else np.log(xc))
                ta = np.exp(np.minimum(al * lt, 700.0))
                rho = amp * np.exp(case.gamma * lt - ex * np.log1p(ta))
            theta = np.where(np.abs(xs) > case.cmax[i, j], 0.0, 1.0)
            mnorm = _trapz(theta * rho * xs ** 2.0, xs) if case.do_norm else 1.0
            ukt = -np.fft.rfft(xs * (rho * theta)).imag * case.step
            with np.errstate(invalid="ignore", divide="ignore"):
                uk = ukt / kts / mnorm
            kout = kts / case.rss[i, j] / (1 + case.zs[i])
            pf = 1.0 if case.post is None else case.post[i, j]
            if uniform:
                sc = -case.step / mnorm * (1.0 / kts[1])
                jj = np.arange(1, M + 1)
                u = np.concatenate([[0.0], np.fft.rfft(xs * (rho * theta)).imag[1:M + 1] * sc * (1.0 / jj)])
                if case.nxs % 2 == 0:
                    u[M] = 0.0
                isc0 = 1.0 / (case.rss[i, j] * (1.0 + case.zs[i]))
                klo, idk, khi = kts[1] * isc0, 1.0 / (kts[1] * isc0), kts[M] * isc0
                q = np.clip((case.ks * idk).astype(np.int64), 1, M - 1)
                fr = np.array([float(Fraction(float(k)) * Fraction(float(idk)) - int(b)) for k, b in zip(case.ks, q)])
                val = u[q] + (u[q + 1] - u[q]) * fr
                out[i, j] = np.where(case.ks < klo, u[1], np.where(case.ks > khi, 0.0, val)) * pf
                c[i, j] = u[1] * pf
                continue
            out[i, j] = np.interp(case.ks, kout[1:M + 1], uk[1:M + 1], left=uk[1], right=0) * pf
            c[i, j] = uk[1] * pf
    return out, c


def oracle_call(case):
    """oracle.hmref.profile_fft fed the same rows (its own power-law form of the family), times post."""
    from oracle import hmref
    nz, nm = case.shape

    def rho_x(xs):
        if case.table is not None:
            t = np.asarray(case.table)
            return np.broadcast_to(t[0], (nz, nm, xs.size)).copy() if t.shape[0] == 1 else t.reshape(nz, nm, xs.size)
        full = lambda a, c: np.full((nz, nm), float(c)) if a is None else np.asarray(a, dtype=np.float64)
        amp, xc, al, ex = (full(a, c)[..., None] for a, c in ((case.amp, case.amp_c), (case.xc, case.xc_c),
                                                               (case.alpha, case.alpha_c), (case.expo, case.expo_c)))
        t = xs[None, None, :] / xc
        return amp * t ** case.gamma * (1.0 + t ** al) ** (-ex)

    out = hmref.profile_fft(rho_x, case.cmax, case.rss, case.zs, case.ks, case.xmax, case.nxs,
                            do_mass_norm=bool(case.do_norm))
    return out if case.post is None else out * case.post[..., None]


# ---------------------------------------------------------------- hmg_sine_transform
SINE_LENGTHS = (600, 5000)


def sine_rows(n):
    """(x, y (2, n)) of the stand-alone sine transform: the grid of the profiles and two seeded non-smooth rows."""
    rng = np.random.default_rng(7000 + n)
    x = np.linspace(0.0, 20.0, n + 1)[1:]
    y = rng.standard_normal((2, n)) * np.exp(-np.linspace(0, 5, n))[None, :]
    y[1] = np.abs(y[1]) / (1.0 + x) ** 2
    return x, y


@functools.lru_cache(maxsize=None)
def sine_reference(n, dps=DPS):
    """{"hi", "lo": (2, n // 2 + 1), "S": (2, 1)}: uk_j = step sum_n x_n y_n sin(2 pi j n / N) = -Im rfft(x y) step, all
    modes j = 0..n // 2; S = step sum |x y|."""
    x, y = sine_rows(n)
    step = (x[-1] - x[0]) / n
    modes = np.arange(n // 2 + 1)
    hi, lo = np.zeros((2, modes.size)), np.zeros((2, modes.size))
    with mp.workdps(dps + 10):
        for r in range(2):
            prod = [mp.mpf(float(a)) * mp.mpf(float(b)) for a, b in zip(x, y[r])]
            F = sine_sums(prod, n, modes, dps)
            for q in modes:
                hi[r, q], lo[r, q] = _split(mp.mpf(float(step)) * F[q])
    S = step * np.sum(np.abs(x[None, :] * y), axis=1, keepdims=True)
    return {"hi": hi, "lo": lo, "S": np.broadcast_to(S, hi.shape).copy()}


def sine_restatement(n):
    x, y = sine_rows(n)
    step = (x[-1] - x[0]) / n
    return -np.fft.rfft(x[None, :] * y, axis=-1).imag * step


# ---------------------------------------------------------------- the row sets
def _grid(nxs, xmax):
    xs = np.linspace(0.0, xmax, nxs + 1)[1:]
    step = (xs[-1] - xs[0]) / nxs
    return xs, np.fft.rfftfreq(nxs, step) * 2 * np.pi


ZS = np.array([0.3, 1.7])
NK2 = 37


def _below(v):
    return float(np.nextafter(v, 0.0))


def _above(v):
    return float(np.nextafter(v, np.inf))


def _family(member, rows, seed):
    """Per-row parameters: the gas member (gamma = -0.2, alpha and expo per row, xc = 1) or the alpha = 1 member with
    xc per row (the pressure profile's)."""
    rng = np.random.default_rng(seed)
    shape = (2, rows // 2)
    if member == "gas":
        al = rng.uniform(0.7, 1.3, shape)
        return dict(amp=rng.uniform(0.5, 40.0, shape), alpha=al, expo=(rng.uniform(2.5, 4.5, shape) - 0.2) / al, gamma=-0.2)
    return dict(amp=rng.uniform(0.5, 40.0, shape), xc=rng.uniform(0.3, 0.9, shape), expo=rng.uniform(3.5, 5.5, shape),
                alpha_c=1.0, gamma=-0.3)


def _edge_cmax(nxs, xmax):
    """Eight truncation radii for a one-row length: both sides of the `pruned` edge xs[2 M / R0] (at it the sample is
    kept and the row is not pruned), short supports, the last sample, and no truncation."""
    xs, _ = _grid(nxs, xmax)
    rad = plan_radices(nxs // 2) if nxs % 2 == 0 and nxs >= 8 else ()
    e = xs[2 * (nxs // 2 // rad[0])] if rad else xs[nxs // 4]
    return np.array([_below(e), e, xs[max(nxs // 50, 1)], 0.4 * e, xs[-2], 1.25 * xmax, _above(xs[nxs // 8]), 0.8 * e])


def _t1(kts, M, rows):
    """T1: ks = the float64 kout_j, j = 1..M, of the first row's rs (1+z); the other rows sit around it."""
    s0 = 0.37
    fac = np.resize(np.array([1.0, 0.8, 1.25, 1.0, 0.5, 2.0, 0.97, 1.1]), rows).reshape(2, rows // 2)
    rss = s0 * fac / (1 + ZS[:, None])
    ks = (kts / rss[0, 0] / (1 + ZS[0]))[1:M + 1]
    return ks.copy(), rss


def _t2(kts, M, rows, modes_lo=20.3):
    """T2: 37 ascending targets; the rows' rs (1+z) put, in order: a row that is all left fill; one with targets beyond
    kout_M; one with tmax in [M - 4, M) (jn capped); one that needs ~20 modes (`keep` where the last pass is long
    enough); one whose fl(k_lo) is a target; three ordinary ones."""
    ks = np.geomspace(1e-3, 1.0, NK2)
    klo = np.array([2.0, ks[-1] / (1.5 * M), ks[-1] / (M - 2.5), ks[-1] / modes_lo, np.sqrt(ks[9] * ks[11]),
                    3.0 * ks[-1] / M, 10.0 * ks[-1] / M, ks[-1] / min(200.0, 0.7 * M)])
    klo = np.resize(klo, rows).reshape(2, rows // 2)
    rss = kts[1] / (klo * (1 + ZS[:, None]))
    if rows >= 5:
        r, c = divmod(4, rows // 2)
        ks[10] = kout_float(kts, rss[r, c], ZS[r])[1]
    assert np.all(np.diff(ks) > 0)
    return ks, rss


def _one_row_cases(tag, route, nxs, xmax, cmax8, env, off, claims, member="gas", seed=0, grids=("T1", "T2", "T3")):
    xs, kts = _grid(nxs, xmax)
    M = nxs // 2
    fam = _family(member, 8, seed or nxs)
    out = {}
    for g in grids:
        ks, rss = _t1(kts, M, 8) if g == "T1" else _t2(kts, M, 8)
        c = Case(name=f"{tag}-{g}", route=route, nxs=nxs, xmax=xmax, cmax=np.asarray(cmax8, dtype=np.float64).reshape(2, 4),
                 rss=rss, zs=ZS, ks=ks, hints=True, env=dict(env), off=dict(off), claims=claims if g == "T2" else (), **fam)
        if g == "T3":
            c = out[f"{tag}-T2"].reversed(c.name)
        out[c.name] = c
    return out


def _build_cases():
    cases = {}
    fused_off = {"HMG_FUSED_FFT": "0"}
    t2claims = ("allleft", "beyond", "capped", "equal_klo")
    # ---- nxs = 5000 / xmax = 20: the hand-sequenced 2500 plan
    xs, _ = _grid(5000, 20.0)
    gas = [_below(xs[749]), xs[749], _above(xs[749]), _below(xs[1250]), xs[1250], 0.4, 19.99, 25.0]
    a1 = [xs[750], xs[749], _below(xs[1250]), xs[1250], 0.4, 19.99, 25.0, 3.0]
    cases.update(_one_row_cases("spec2500-gas", "spec2500", 5000, 20.0, gas, {}, fused_off,
                                t2claims + ("keep", "pruned", "unpruned", "lead3", "nolead3")))
    cases.update(_one_row_cases("spec2500-alpha1", "spec2500", 5000, 20.0, a1, {}, fused_off,
                                t2claims + ("keep", "pruned", "unpruned", "lead3", "nolead3"), member="alpha1", seed=11,
                                grids=("T2", "T3")))
    # ---- compile-time plans; 6000 with the long-grid routes off
    for nxs in (1000, 2000, 3000, 4000, 6000):
        env = {"HMG_PRUNED_FFT": "0"} if nxs == 6000 else {}
        cases.update(_one_row_cases(f"ct{nxs}", "ct", nxs, 20.0, _edge_cmax(nxs, 20.0), env, {**env, **fused_off},
                                    t2claims + ("keep", "pruned", "unpruned"), member="gas" if nxs % 2000 else "alpha1",
                                    grids=("T1", "T2", "T3") if nxs == 1000 else ("T2",)))
    # ---- run-time plan
    for nxs in (600, 30, 16, 5400):
        cl = t2claims + (("pruned", "unpruned") + (("keep",) if nxs >= 600 else ()))
        cases.update(_one_row_cases(f"rt{nxs}", "rt", nxs, 20.0, _edge_cmax(nxs, 20.0), {}, fused_off, cl,
                                    grids=("T1", "T2", "T3") if nxs in (600, 30) else ("T1", "T2") if nxs == 16 else ("T2",)))
    # ---- rocFFT fallback: the only route of these lengths (HMG_FUSED_FFT=0 gives the same bits)
    for nxs in (14, 45, 7000):
        cm = _edge_cmax(nxs, 20.0)
        if nxs == 7000:
            cm = np.minimum(cm, 3.0 + 0.1 * np.arange(8))      # (short supports: the reference runs direct sums here)
        cases.update(_one_row_cases(f"rocfft{nxs}", "rocfft", nxs, 20.0, cm, {}, fused_off, t2claims,
                                    grids=("T1", "T2", "T3") if nxs == 14 else ("T1", "T2") if nxs == 45 else ("T2",)))
        for c in cases.values():
            if c.name.startswith(f"rocfft{nxs}-"):
                c.off_equal = True
    # ---- the smallest shape without the mass norm, with a post array and a prepared ln x table
    b = cases["rt16-T2"]
    cases["rt16-nonorm-post-logx"] = dataclasses.replace(b, name="rt16-nonorm-post-logx", do_norm=0, logx=True, claims=(),
                                                         post=np.array([[3.0, -0.7, 1e-3, 41.0], [0.11, 2.5, -8.0, 1.0]]))
    b = cases["spec2500-gas-T2"]
    cases["spec2500-gas-T2-logx"] = dataclasses.replace(b, name="spec2500-gas-T2-logx", logx=True, claims=(), same_as=b.name)
    # ---- long grids: pruned decomposition (chirp off), chirp route (default switches, rows that need <= 590 modes)
    nochirp = {"HMG_CHIRP": "0"}
    for nxs, xmax in ((30000, 50.0), (25000, 50.0)):
        xs, kts = _grid(nxs, xmax)
        M = nxs // 2
        cm = np.array([[2.5, 0.4, _below(xs[1999]), xs[1999]], [1.1, 2.9, 3.3, xs[1200]]])
        fam = _family("gas", 8, nxs)
        ks, rss = _t2(kts, M, 8)
        t2 = Case(name=f"pruned{nxs}-T2", route="pruned", nxs=nxs, xmax=xmax, cmax=cm, rss=rss, zs=ZS, ks=ks, hints=True,
                  env=nochirp, off={"HMG_PRUNED_FFT": "0"}, claims=t2claims, **fam)
        cases[t2.name] = t2
        cases[f"pruned{nxs}-T3"] = t2.reversed(f"pruned{nxs}-T3")
        if nxs == 30000:
            cases["chirp30000-T2"] = dataclasses.replace(t2, name="chirp30000-T2", route="chirp", env={}, off=nochirp,
                                                         claims=("fewmodes",), same_as=t2.name)
    # (every mode read on the decomposition: nxs = 10000 / xmax = 20 - too long for one row, LP = 1000 or 1250 - four rows)
    xs, kts = _grid(10000, 20.0)
    fam4 = _family("gas", 4, 10000)
    ks1, rss1 = _t1(kts, 5000, 4)
    cases["pruned10000-T1"] = Case(name="pruned10000-T1", route="pruned", nxs=10000, xmax=20.0,
                                   cmax=np.array([[2.5, 0.4], [_below(xs[1999]), xs[1999]]]), rss=rss1, zs=ZS, ks=ks1,
                                   hints=True, env=nochirp, off={"HMG_PRUNED_FFT": "0", "HMG_FUSED_FFT": "0"}, **fam4)
    # ---- narrow band: the support fills the grid, every row needs few modes (2 jn + 2 <= 1000); two rows
    xs, kts = _grid(30000, 2.0)
    ks = np.geomspace(1e-3, 1.0, NK2)
    klo = np.array([[ks[-1] / 400.3], [ks[-1] / 47.7]])
    fam = _family("alpha1", 8, 5)
    fam = {k: (v[:, :1].copy() if isinstance(v, np.ndarray) else v) for k, v in fam.items()}
    cases["band30000-T2"] = Case(name="band30000-T2", route="band", nxs=30000, xmax=2.0, cmax=np.array([[2.0], [2.5]]),
                                 rss=kts[1] / (klo * (1 + ZS[:, None])), zs=ZS, ks=ks, hints=True, env={},
                                 off={"HMG_BAND_FFT": "0"}, claims=("fullsupport", "fewmodes"), **fam)
    # ---- table variant: a seeded positive non-smooth table, shared by the rows or one per row
    for nxs in (1000, 5000):
        xs, kts = _grid(nxs, 20.0)
        M = nxs // 2
        rng = np.random.default_rng(900 + nxs)
        cm = (np.array(gas) if nxs == 5000 else _edge_cmax(nxs, 20.0)).reshape(2, 4)
        for rho_rows in (1, 8):
            tab = rng.uniform(0.05, 1.0, (rho_rows, nxs)) / (1.0 + xs[None, :]) ** 3
            for g in ("T1", "T2"):
                if g == "T1" and rho_rows == 8:
                    continue
                ks, rss = _t1(kts, M, 8) if g == "T1" else _t2(kts, M, 8)
                name = f"table{nxs}-r{rho_rows}-{g}"
                # (the table entry point takes no hint arrays)
                cases[name] = Case(name=name, route="table", nxs=nxs, xmax=20.0, cmax=cm, rss=rss, zs=ZS, ks=ks, hints=False,
                                   table=tab, env={}, off=fused_off)
                if g == "T2" and rho_rows == 1:
                    cases[f"table{nxs}-r1-T3"] = cases[name].reversed(f"table{nxs}-r1-T3")
    return cases


# the names of the row sets, for parametrised tests that must not build them at collection (asserted against the build)
CASE_NAMES = (
    "spec2500-gas-T1", "spec2500-gas-T2", "spec2500-gas-T3", "spec2500-alpha1-T2", "spec2500-alpha1-T3", "ct1000-T1",
    "ct1000-T2", "ct1000-T3", "ct2000-T2", "ct3000-T2", "ct4000-T2", "ct6000-T2", "rt600-T1", "rt600-T2", "rt600-T3",
    "rt30-T1", "rt30-T2", "rt30-T3", "rt16-T1", "rt16-T2", "rt5400-T2", "rocfft14-T1", "rocfft14-T2", "rocfft14-T3",
    "rocfft45-T1", "rocfft45-T2", "rocfft7000-T2", "rt16-nonorm-post-logx", "spec2500-gas-T2-logx", "pruned30000-T2",
    "pruned30000-T3", "chirp30000-T2", "pruned25000-T2", "pruned25000-T3", "pruned10000-T1", "band30000-T2",
    "table1000-r1-T1", "table1000-r1-T2", "table1000-r1-T3", "table1000-r8-T2", "table5000-r1-T1", "table5000-r1-T2",
    "table5000-r1-T3", "table5000-r8-T2")


class _Cases(collections.abc.Mapping):
    """The row sets by name, built on first use (building them asks the host plan builder for radices: a compiler run
    that must not happen at import, where it would break test collection instead of failing a test)."""
    _d = None

    def _get(self):
        if self._d is None:
            type(self)._d = _build_cases()
            assert tuple(self._d) == CASE_NAMES, sorted(set(self._d) ^ set(CASE_NAMES))
        return self._d

    def __getitem__(self, k):
        return self._get()[k]

    def __iter__(self):
        return iter(self._get())

    def __len__(self):
        return len(self._get())


CASES = _Cases()


def claims_hit(case):
    """Which of the claims a case's rows hit, from the restated predicates."""
    xs, kts = case.xs, case.kts
    nz, nm = case.shape
    hit = set()
    M = case.nxs // 2
    for i in range(nz):
        for j in range(nm):
            pi = input_predicates(xs, case.cmax[i, j], case.nxs)
            po = output_predicates(kts, case.rss[i, j], case.zs[i], case.ks, case.nxs, case.hints)
            hit.add("pruned" if pi["pruned"] else "unpruned")
            hit.add("lead3" if pi["lead3"] else "nolead3")
            if po["keep"]:
                hit.add("keep")
            if po["nleft"] == case.ks.size:
                hit.add("allleft")
            if po["beyond"]:
                hit.add("beyond")
            if po["capped"] and not po["beyond"]:
                hit.add("capped")
            if po["jn"] <= 590:
                hit.add("fewmodes")
            if np.any(case.ks == kout_float(kts, case.rss[i, j], case.zs[i])[1]):
                hit.add("equal_klo")
            if case.cmax[i, j] >= xs[-1]:
                hit.add("fullsupport")
    return hit
