"""The pointwise probe of the device math headers: build, call, point sets, 50-digit references and gates, shared by
tests/test_math_probe_cpu.py (no device: builds the probe, checks independent implementations against every gate) and
tests/test_gpu_math_probe.py (the probe on the device against the same references and gates).

* ``build()`` compiles tests/hip/math_probe.hip into tests/hip/libmathprobe.so with the flags the library's Makefile
  gives its kernel units (asked of make, not restated), when the .so is missing or older than the source or any header
  under hmvec_amd/csrc.  ``call(fn, x, y, z)`` runs one function at n points on the device.
* ``Ref`` holds a reference as a float64 pair hi + lo (hi the rounded value, lo the remainder), so that an error of a
  fraction of an ulp is measured, not rounded away: err = |(got - hi) - lo|.
* Every gate is a function of the point and of the reference alone.  u = 2^-53.  No point is left out of a comparison.

The constants that the issue leaves to a measurement were set on 2026-10-21 with SciPy 1.15.3 (Cephes) and
mpmath 1.3.0 at 50 digits on the point sets below, by the rule "worst error of the independent implementation, in the
gate's unit, times 2, rounded up to an integer"; tests/test_math_probe_cpu.py fails if the independent implementation
leaves half of a gate that was set this way (MEASURED holds the figures):

    C_J = 8         scipy j0 / j1 on 20000 random points of (0, 5] and 5000 of (5, 200] (a denser sample of the same
                    ranges than the test's set, whose own worst is 2.75): worst 3.60 u (J0 at x = 0.678) and 2.77 u s(x)
                    (J1 at x = 2.12) after the phase term; nothing beyond the phase term above 5
    C_I0E = 5       scipy i0e: worst 2.07 x 2^-52 relative
    C_J2_SERIES = 4 numpy restatement of the nested series below 2.0: worst 1.65 u relative (Cephes jv(2, x) is the
                    recurrence 2 J1/x - J0 there and cancels: 18 u on the set, no measure of the series)
    C2              16 from the project (helpers/angcov_model.py) for H1 and F1 = G4; for the others the numpy
                    restatement's worst (err - coef dJ) / (u |value|): g 2.70 -> 6, H2 3.87 -> 8, F2 5.88 -> 12,
                    S 0.83 -> 2, G 0.55 -> 2
    K_AUX = 8       f and g of sici_aux below 64, from an operation count: see ``aux_gate``

The Bessel gate's phase term is the header's own: above 5 the argument x - pi/4 (x - 3 pi/4 in j1.hpp) is rounded once,
half a spacing of x, and sincos_fast adds 2e-16 absolute; both under the envelope sqrt(2/(pi x)).
"""
import ctypes
import functools
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
REPO = os.path.dirname(TESTS)
CSRC = os.path.join(REPO, "hmvec_amd", "csrc")
SRC = os.path.join(TESTS, "hip", "math_probe.hip")
LIB = os.path.join(TESTS, "hip", "libmathprobe.so")

U = 2.0 ** -53
DPS = 50

# the enum of tests/hip/math_probe.hip, in its order
FN = {name: i for i, name in enumerate(
    ["j0", "j1", "j2", "j01", "i0e", "sincos_fast", "xi_sincos", "sin_minus_ycos", "rcp_fast", "sici", "sici_aux_fg",
     "sici_aux_g", "log", "exp_clamp", "exp_noclamp", "log1p", "log1p_abs", "fm_rcp", "gnfw", "gnfw_alpha1", "node_g_h2",
     "node_h1_g4", "node_f2", "xi_panel", "gauss_m0_m1", "gauss_m2"])}
GNFW_GAMMA = -0.2

C_J = 8.0
C_I0E = 5.0
C_J2_SERIES = 4.0
C2 = {"h1": 16.0, "f1": 16.0, "g": 6.0, "h2": 8.0, "f2": 12.0, "S": 2.0, "G": 2.0}
# what the rule was applied to (tests/test_math_probe_cpu.py re-measures them on the test's own, thinner sets)
MEASURED = {"j0": 3.60, "j1": 2.77, "i0e": 2.07, "j2_series": 1.65,
            "g": 2.70, "h1": 3.02, "h2": 3.87, "f1": 5.38, "f2": 5.88, "S": 0.83, "G": 0.55}


# ---------------------------------------------------------------- build and call
class ProbeBuildError(RuntimeError):
    pass


def _newest_source():
    t = os.path.getmtime(SRC)
    for root, _, files in os.walk(CSRC):
        for f in files:
            if f.endswith((".hpp", ".h")):
                t = max(t, os.path.getmtime(os.path.join(root, f)))
    return t


def cxxflags():
    """CXXFLAGS of hmvec_amd/csrc/Makefile, as make expands them."""
    r = subprocess.run(["make", "-s", "-C", CSRC, "--eval=print-cxxflags: ; @echo $(CXXFLAGS)", "print-cxxflags"],
                       capture_output=True, text=True)
    if r.returncode != 0 or not r.stdout.strip():
        raise ProbeBuildError(f"make could not print the library's CXXFLAGS: {r.stderr[-1000:]}")
    return r.stdout.split()


def build(force=False):
    """The path of a current libmathprobe.so; raises ProbeBuildError (the tests then FAIL) if there is none and hipcc
    cannot make one."""
    if not force and os.path.exists(LIB) and os.path.getmtime(LIB) >= _newest_source():
        return LIB
    hipcc = os.environ.get("HIPCC") or os.path.join(os.environ.get("ROCM", "/opt/rocm"), "bin", "hipcc")
    cmd = [hipcc, *cxxflags(), "-I", CSRC, "-shared", SRC, "-o", LIB]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True)
    except OSError as e:
        raise ProbeBuildError(f"no current {LIB} and hipcc could not be run ({e})") from e
    if r.returncode != 0:
        raise ProbeBuildError(f"no current {LIB} and hipcc failed:\n{' '.join(cmd)}\n{r.stderr[-4000:]}")
    return LIB


@functools.lru_cache(maxsize=None)
def _lib():
    lib = ctypes.CDLL(build())
    lib.math_probe_run.restype = ctypes.c_int
    lib.math_probe_run.argtypes = [ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 5
    return lib


def call(fn, x, y=None, z=None):
    """(out0, out1) of the device function ``fn`` at x[i] (and y[i], z[i])."""
    arrs = [None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in (x, y, z)]
    n = arrs[0].size
    assert all(a is None or a.shape == (n,) for a in arrs)
    o0, o1 = np.full(n, np.nan), np.full(n, np.nan)
    ptr = [None if a is None else a.ctypes.data for a in arrs]
    rc = _lib().math_probe_run(FN[fn], n, *ptr, o0.ctypes.data, o1.ctypes.data)
    if rc != 0:
        raise RuntimeError(f"math_probe_run({fn}) returned HIP error {rc}")
    return o0, o1


# ---------------------------------------------------------------- references as hi + lo
class Ref:
    def __init__(self, vals):
        import mpmath as mp
        self.hi = np.array([float(v) for v in vals])
        self.lo = np.array([float(v - mp.mpf(h)) if np.isfinite(h) else 0.0 for v, h in zip(vals, self.hi)])

    def err(self, got):
        got = np.asarray(got, dtype=np.float64)
        e = np.abs((got - self.hi) - self.lo)
        return np.where(np.isfinite(got), e, np.inf)

    @property
    def abs(self):
        return np.abs(self.hi)

    @property
    def ulp(self):
        return np.spacing(np.abs(self.hi))


def ratio(err, gate):
    """err / gate per point; a zero gate admits a zero error only."""
    err, gate = np.asarray(err, dtype=np.float64), np.asarray(gate, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(gate > 0.0, err / np.where(gate > 0.0, gate, 1.0), np.where(err == 0.0, 0.0, np.inf))


def _ref(fn, *cols):
    import mpmath as mp
    with mp.workdps(DPS + 15):
        return Ref([fn(*(mp.mpf(float(v)) for v in p)) for p in zip(*cols)])


def _key(a):
    return np.ascontiguousarray(a, dtype=np.float64).tobytes()


def cached(fn):
    """Cache on the bytes of the float64 arguments: a reference is computed once per process and never changed."""
    store = {}

    @functools.wraps(fn)
    def wrapper(*arrs):
        k = tuple(_key(a) for a in arrs)
        if k not in store:
            store[k] = fn(*arrs)
        return store[k]
    return wrapper


@cached
def ref_bessel(x):
    import mpmath as mp
    return tuple(_ref(lambda v, n=n: mp.besselj(n, v), x) for n in (0, 1, 2))


@cached
def ref_i0e(x):
    import mpmath as mp
    return _ref(lambda v: mp.besseli(0, v) * mp.exp(-abs(v)), x)


@cached
def ref_sincos(x):
    import mpmath as mp
    return _ref(mp.sin, x), _ref(mp.cos, x)


@cached
def reduced_abs(x):
    """|x - k pi/2|, k the nearest integer to 2x/pi, rounded to float64."""
    import mpmath as mp
    with mp.workdps(DPS + 15):
        h = mp.pi / 2
        return np.array([float(abs(mp.mpf(float(v)) - mp.nint(mp.mpf(float(v)) / h) * h)) for v in x])


@cached
def ref_smyc(x, y):
    import mpmath as mp
    return _ref(lambda a, b: abs(mp.sin(a) - b * mp.cos(a)), x, y)


@cached
def ref_rcp(x):
    return _ref(lambda v: 1 / v, x)


@cached
def ref_sici(x):
    import mpmath as mp
    return _ref(mp.si, x), _ref(mp.ci, x)


@cached
def ref_aux(x):
    """f and g of Si = pi/2 - f cos - g sin, Ci = f sin - g cos (the cancellation in g costs log10 x digits of 65)."""
    import mpmath as mp
    f = _ref(lambda v: mp.ci(v) * mp.sin(v) + (mp.pi / 2 - mp.si(v)) * mp.cos(v), x)
    g = _ref(lambda v: -mp.ci(v) * mp.cos(v) + (mp.pi / 2 - mp.si(v)) * mp.sin(v), x)
    return f, g


@cached
def ref_log(x):
    import mpmath as mp
    return _ref(mp.log, x)


@cached
def ref_exp(x):
    import mpmath as mp
    return _ref(mp.exp, x)


@cached
def ref_log1p(x):
    import mpmath as mp
    return _ref(mp.log1p, x)


@cached
def ref_gnfw(t, a, e):
    import mpmath as mp
    g = mp.mpf(GNFW_GAMMA)
    return _ref(lambda t_, a_, e_: t_ ** g * (1 + t_ ** a_) ** (-e_), t, a, e)


def _hyp_or_closed(x, hyp, closed):
    import mpmath as mp
    if x < 50:
        return hyp(x, -x * x / 4)
    return closed(x, mp.besselj(0, x), mp.besselj(1, x))


@cached
def ref_nodes(x):
    """g, H1, H2, F1, F2 of kernels/hankel.hpp: the hypergeometric forms below 50, the closed forms in 65-digit J0 and
    J1 above (not the expression the kernel evaluates on either side of its switches)."""
    import mpmath as mp
    forms = {
        "g": (lambda x, w: x ** 4 / 8 * mp.hyp0f1(3, w), lambda x, a, b: x * (2 * b - x * a)),
        "h1": (lambda x, w: x ** 4 / 32 * mp.hyp1f2(2, 3, 3, w), lambda x, a, b: 2 * (1 - a) - x * b),
        "h2": (lambda x, w: x ** 6 / 192 * mp.hyp1f2(2, 3, 4, w),
               lambda x, a, b: x * x - 2 * x * b - x * (2 * b - x * a)),
        "f1": (lambda x, w: x ** 6 / 2304 * mp.hyp1f2(3, 4, 5, w), lambda x, a, b: 4 + 8 * a + x * b - 24 * b / x),
        "f2": (lambda x, w: x ** 8 / 18432 * mp.hyp1f2(3, 5, 5, w),
               lambda x, a, b: 2 * x * x + 8 * x * b + x * (2 * b - x * a) + 24 * (a - 1)),
    }
    return {k: _ref(lambda v, h=h, c=c: _hyp_or_closed(v, h, c), x) for k, (h, c) in forms.items()}


@cached
def ref_panel(th):
    """S = sin(th)/th = 0F1(; 3/2; -th^2/4) and G = 3 (sin th - th cos th)/th^3 = 0F1(; 5/2; -th^2/4)."""
    import mpmath as mp

    def S(t):
        return mp.hyp0f1(mp.mpf(3) / 2, -t * t / 4) if t < 50 else mp.sin(t) / t

    def G(t):
        return mp.hyp0f1(mp.mpf(5) / 2, -t * t / 4) if t < 50 else 3 * (mp.sin(t) - t * mp.cos(t)) / t ** 3
    return _ref(S, th), _ref(G, th)


@cached
def ref_moments(t):
    import mpmath as mp

    def M(n):
        h = n + mp.mpf("0.5")
        return lambda v: mp.mpf(1) / (2 * n + 1) if v == 0 else mp.gammainc(h, 0, v) / (2 * v ** h)
    return tuple(_ref(M(n), t) for n in range(3))


# ---------------------------------------------------------------- point sets (seeded, fixed)
def _sides(v):
    return [np.nextafter(v, 0.0), v, np.nextafter(v, np.inf)]


@functools.lru_cache(maxsize=None)
def bessel_points():
    """x >= 0: 0, tiny, each side of the switches 2 and 5, the first 40 zeros of J0 and of J1 with both float neighbours,
    a ladder across [4, 6] (a switch moved off 5.0 puts a form where it was not fitted), random points of each range,
    log-uniform points to 1e9 and (library reduction) to 1e15."""
    from scipy.special import jn_zeros
    rng = np.random.default_rng(20261021)
    zeros = np.concatenate([jn_zeros(0, 40), jn_zeros(1, 40)])
    pts = [[0.0, 1e-300, 1e-8], _sides(5.0), _sides(2.0), [5.0 * (1 - 1e-6), 5.0 * (1 + 1e-6)], np.linspace(4.0, 6.0, 41),
           zeros, np.nextafter(zeros, 0.0), np.nextafter(zeros, np.inf),
           rng.uniform(0.0, 5.0, 300), rng.uniform(5.0, 200.0, 300), 10 ** rng.uniform(2, 9, 300),
           10 ** rng.uniform(9, 15, 100)]
    return np.concatenate([np.asarray(p, dtype=np.float64) for p in pts])


@functools.lru_cache(maxsize=None)
def bessel_signed_points():
    """bessel_points and the negatives of a spread of them (the parities of j0.hpp and j1.hpp)."""
    x = bessel_points()
    return np.concatenate([x, -x[::7], -np.asarray(_sides(5.0) + _sides(2.0))])


@functools.lru_cache(maxsize=None)
def j01_points():
    """bessel_points and the hand-over from sincos_fast to the library at chi = x - pi/4 = 2^30."""
    h = 2.0 ** 30
    edge = [h, h * (1 - 2.0 ** -40), h * (1 + 2.0 ** -40)] + _sides(h + 0.7853981633974483) + _sides(h)
    return np.concatenate([bessel_points(), np.asarray(edge)])


@functools.lru_cache(maxsize=None)
def i0e_points():
    rng = np.random.default_rng(20261022)
    x = np.concatenate([[0.0, 1e-300, 1e-8], _sides(8.0), rng.uniform(0.0, 8.0, 400), 10 ** rng.uniform(np.log10(8.0), 9, 400)])
    return np.concatenate([x, -x[::5]])


# k whose nearest double to k pi/2 lies within 4e-16 (k < 1e6), 1e-14 (k < 1e8) and 1e-13 (k < 6.8e8) of it: the ten
# smallest |fl(k pi/2) - k pi/2| of 9e5, 4e6 and 4e6 random k of each range (exact products by Dekker's splitting; the
# closest, k = 347177659, is 1.5e-15 away).  There the third Cody-Waite term, k x 1.5e-33, is up to 5e5 spacings of the
# reduced argument, which is the whole sine (or cosine).
NEAR_K = [14479, 14848, 29327, 58285, 58654, 145897, 204551, 263205, 554999, 818204, 1167176, 1991284, 2134229, 3329994,
          4211280, 5876277, 12193197, 24631887, 25725104, 61668902, 132496843, 150680673, 151528397, 161679967, 238219486,
          238777596, 274442339, 285441633, 347177659, 580600415]


@functools.lru_cache(maxsize=None)
def sincos_points():
    """[0, 2^30): random points and the doubles nearest to k pi/2, k up to 6.8e8, where the reduced argument is smallest
    (NEAR_K: where the third Cody-Waite term decides the leading digits)."""
    rng = np.random.default_rng(20261023)
    k = np.unique(np.concatenate([np.arange(1, 65), (10 ** rng.uniform(2, np.log10(6.8e8), 600)).astype(np.int64), NEAR_K]))
    near = k.astype(np.float64) * (np.pi / 2)
    near = near[near < 2.0 ** 30]
    return np.concatenate([[0.0, 1e-300, 1e-8, np.nextafter(2.0 ** 30, 0.0)], rng.uniform(0.0, 2.0 ** 30, 500),
                           rng.uniform(0.0, 10.0, 300), 10 ** rng.uniform(-6, 9, 300), near])


@functools.lru_cache(maxsize=None)
def xi_sincos_points():
    h = 2.0 ** 30
    rng = np.random.default_rng(20261024)
    return np.concatenate([sincos_points()[::3], _sides(h), [h * (1 - 2.0 ** -40), h * (1 + 2.0 ** -40)],
                           10 ** rng.uniform(np.log10(h), 15, 100)])


@functools.lru_cache(maxsize=None)
def smyc_points():
    """x = y = k R as the sigma^2 contraction has them: k from 1e-4 to 1e2 h/Mpc against R from 0.1 to 50 Mpc/h."""
    rng = np.random.default_rng(20261025)
    x = np.concatenate([10 ** rng.uniform(-5, np.log10(5e3), 1500), np.arange(1, 200) * (np.pi / 2), [1e-8, 4.493409457909064]])
    return x, x.copy()


@functools.lru_cache(maxsize=None)
def rcp_points():
    rng = np.random.default_rng(20261026)
    x = np.ldexp(rng.uniform(1.0, 2.0, 2000), rng.integers(-1000, 1000, 2000))
    x = np.concatenate([x, [1.0, 2.0, 3.0, np.nextafter(2.0, 0.0), np.nextafter(1.0, 2.0), 1e-300, 1e300]])
    return np.concatenate([x, -x[::4]])


@functools.lru_cache(maxsize=None)
def sici_points():
    rng = np.random.default_rng(20261027)
    return np.concatenate([_sides(4.0), _sides(8.0), _sides(64.0), [1e-3, 1e-8], rng.uniform(0.0, 4.0, 300),
                           rng.uniform(4.0, 8.0, 300), rng.uniform(8.0, 64.0, 300), rng.uniform(64.0, 256.0, 200),
                           10 ** rng.uniform(-3, 8, 300)])


@functools.lru_cache(maxsize=None)
def aux_points():
    x = sici_points()
    return x[x > 4.0]


@functools.lru_cache(maxsize=None)
def fastmath_points():
    """The sets of tests/test_fastmath_cpu.py (same generator, same seed), every 80th point and the special values."""
    rng = np.random.default_rng(1)
    x = np.concatenate([10 ** rng.uniform(-300, 300, 100000), rng.uniform(0.5, 2.0, 100000),
                        1 + rng.uniform(-1e-3, 1e-3, 50000)])
    y = np.concatenate([rng.uniform(-700, 700, 100000), rng.uniform(-1, 1, 100000), rng.uniform(-1e-8, 1e-8, 1000)])
    a = np.concatenate([10 ** rng.uniform(-300, 300, 100000), rng.uniform(0, 3, 100000)])
    return {"log": np.concatenate([x[::80], [1.0, 0.5, 2.0, np.sqrt(0.5), np.nextafter(np.sqrt(0.5), 1.0)]]),
            "exp": np.concatenate([y[::80], [0.0, 699.9, -699.9]]),
            "log1p": np.concatenate([a[::80], [1e-17, 2.0 ** -53, 2.0 ** -52, 0.0]])}


@functools.lru_cache(maxsize=None)
def gnfw_points():
    """tests/test_fastmath_cpu.py's integrand set (seed 2), every 8th point; and a set with alpha = 1 for the member."""
    rng = np.random.default_rng(2)
    t = 10 ** rng.uniform(-4, 1.5, 20000)
    a, e = rng.uniform(0.5, 2.5, t.size), rng.uniform(1.0, 6.0, t.size)
    return t[::8].copy(), a[::8].copy(), e[::8].copy()


@functools.lru_cache(maxsize=None)
def node_points():
    """x of the node functions: each side of the switches 2 and 5 (and 1 -+ 1e-6 of them), random points below,
    between and above, x down to 1e-8 and up to 1e6."""
    rng = np.random.default_rng(20261028)
    pts = [_sides(2.0), _sides(5.0), [2.0 * (1 - 1e-6), 2.0 * (1 + 1e-6), 5.0 * (1 - 1e-6), 5.0 * (1 + 1e-6)],
           [1e-8, 1e-6, 1e-3, 1e6], rng.uniform(0.0, 2.0, 200), rng.uniform(2.0, 5.0, 200), rng.uniform(5.0, 60.0, 200),
           10 ** rng.uniform(-8, 0, 150), 10 ** rng.uniform(1, 6, 250)]
    return np.concatenate([np.asarray(p, dtype=np.float64) for p in pts])


@functools.lru_cache(maxsize=None)
def panel_points():
    rng = np.random.default_rng(20261029)
    pts = [[0.0, 1e-300, 1e-8], _sides(0.5), [0.5 * (1 - 1e-6), 0.5 * (1 + 1e-6)], rng.uniform(0.0, 0.5, 300),
           rng.uniform(0.5, 20.0, 300), 10 ** rng.uniform(-8, 6, 300)]
    return np.concatenate([np.asarray(p, dtype=np.float64) for p in pts])


@functools.lru_cache(maxsize=None)
def moment_points():
    """moment_grid of tests/test_rsd_cpu.py."""
    special = [0.0, 1e-300, 1e-8, np.nextafter(1.0, 0.0), 1.0, np.nextafter(1.0, 2.0), np.nextafter(2.0, 0.0), 2.0, 50.0,
               1e5, 1e8]
    return np.concatenate([special, np.geomspace(1e-8, 1e5, 521), np.linspace(0.5, 4.0, 141)])


# ---------------------------------------------------------------- gates
def envelope(x):
    return np.sqrt(2.0 / (np.pi * np.maximum(np.abs(x), 5.0)))


def phase_term(x):
    """[|x| > 5] sqrt(2/(pi x)) (spacing(x)/2 + 2e-16): the argument of the Hankel form rounded once, and sincos_fast's
    absolute term."""
    ax = np.abs(x)
    return np.where(ax > 5.0, envelope(ax) * (0.5 * np.spacing(ax) + 2e-16), 0.0)


def dJ(x, order, c=C_J):
    """The gate of J0 (order 0: s = 1) and J1 (order 1: s = min(1, |x|))."""
    ax = np.abs(x)
    s = 1.0 if order == 0 else np.minimum(1.0, ax)
    return c * U * s + phase_term(ax)


def j2_gate(x, j2_abs):
    """Above the switch that of 2 J1/x - J0 with one rounding of each term; below it C_J2_SERIES u relative."""
    ax = np.abs(x)
    safe = np.maximum(ax, 2.0)
    return np.where(ax < 2.0, C_J2_SERIES * U * j2_abs, 2.0 * dJ(safe, 1) / safe + dJ(safe, 0) + 4.0 * U * j2_abs)


def i0e_gate(ref_abs):
    return C_I0E * 2.0 ** -52 * ref_abs


def sincos_gate(x, ref):
    """1 ulp of the result + the reduction's term.  The header claimed 2e-16 absolute for the reduction; under that no
    test can see the third Cody-Waite term (at most 1e-24).  What the reduction can promise is tighter: below 2^30 the
    first step x - k c1 is exact, the second and third round once each at the size of the reduced argument r, so r is
    off by at most one spacing of r and the result (slope at most 1 in r) by as much: min(2e-16, 2 spacing(r)), a factor 2
    to spare.  From 2^30 on (xi_sincos: the library's reduction) the term stays 2e-16."""
    red = np.where(np.abs(x) < 2.0 ** 30, np.minimum(2e-16, 2.0 * np.spacing(reduced_abs(x))), 2e-16)
    return ref.ulp + red


def smyc_gate(y, ref):
    """(1 + |y|) (1 ulp + 2e-16) for the sine and the cosine (an ulp of a value below 1 is at most 2^-53) and one ulp of
    the result."""
    return (1.0 + np.abs(y)) * (2.0 ** -53 + 2e-16) + ref.ulp


def sici_gate(x, ref):
    """1e-15 absolute (the header's notes) + the sine/cosine term (|f| + |g|)(1 ulp + 2e-16) <= (1/x + 1/x^2)(...)
    above 4 + one ulp of the result."""
    trig = np.where(x > 4.0, (1.0 / np.maximum(x, 4.0) + 1.0 / np.maximum(x, 4.0) ** 2) * (2.0 ** -53 + 2e-16), 0.0)
    return 1e-15 + trig + ref.ulp


# f and g of sici_aux, relative.  On [64, inf) twice the header's recorded 2.5e-16 and 4.2e-16.  Below 64 SciPy offers
# Si and Ci only, and f = Ci sin + (pi/2 - Si) cos, g = -Ci cos + (pi/2 - Si) sin formed from them in float64 carry the
# cancellation of pi/2 - Si (measured 40 and 2700 units of 2^-52 on the set below 64, and no digit at all at 1e8): a
# property of that combination, not of the rationals the device divides, so no constant can be "set as for C_J" from it.
# The independent side is instead the defining integrals by quadrature (``aux_quad``: inside 0.93 x 2^-52 of mpmath at
# every point), and the gate below 64 is the bound of the device's own operation count: per quotient two Horner chains
# in z <= 1/16 (1.1 u each), the factor x (1 u), the shared reciprocal of the product (1 + 2 u), two products (2 u) and
# z = rcp(x)^2 entering with a sensitivity below 1/8 (0.6 u): 9.8 u = 4.9 x 2^-52, and the published rationals' own
# error of 1e-16 relative: K_AUX = 8 units of 2^-52, a factor 1.4 to spare.
K_AUX = 8.0
AUX_ASYM = (2.0 * 2.5e-16, 2.0 * 4.2e-16)


def aux_gate(x, ref, which):
    return np.where(x >= 64.0, AUX_ASYM[which], K_AUX * 2.0 ** -52) * ref.abs


def aux_quad(x):
    """f = int_0^inf e^(-x t) / (1 + t^2) dt and g = int_0^inf t e^(-x t) / (1 + t^2) dt for x > 4 by Gauss-Legendre
    quadrature in s = x t (90 panels of 16 nodes on [0, 45]), taken as 1 - int e^(-s) q / (1 + q), q = (s/x)^2, so that
    the rounding of the weights enters through the small complement only; the tail beyond 45 is below 3e-20."""
    nodes, w = np.polynomial.legendre.leggauss(16)
    edges = np.arange(0.0, 45.0 + 1e-9, 0.5)
    s = (0.5 * (edges[:-1] + edges[1:])[:, None] + 0.25 * nodes[None, :]).ravel()
    e = np.exp(-s) * np.tile(0.25 * w, edges.size - 1)
    q = (s[None, :] / x[:, None]) ** 2
    c = q / (1.0 + q)
    return (1.0 - np.sum(c * e[None, :], axis=1)) / x, (1.0 - np.sum(c * (e * s)[None, :], axis=1)) / (x * x)


def node_coef(x):
    """The factor J0 and J1 carry in the closed forms of g, H1, H2, F1, F2 (zero where the series is evaluated)."""
    hk, ag = x >= 2.0, x >= 5.0
    xs = np.maximum(x, 1.0)
    return {"g": np.where(hk, x * x + 2 * x, 0.0), "h1": np.where(hk, 2.0 + x, 0.0),
            "h2": np.where(hk, x * x + 4 * x, 0.0), "f1": np.where(ag, 8.0 + x + 24.0 / xs, 0.0),
            "f2": np.where(ag, x * x + 10 * x + 24.0, 0.0)}


def node_gate(x, name, ref):
    """C2 u |value| + coef(x) dJ(x), as helpers/angcov_model.py writes it for G_mu, dJ the Bessel gate above."""
    return C2[name] * U * ref.abs + node_coef(x)[name] * dJ(np.maximum(x, 1.0), 0)


def panel_gate(th, which, ref):
    """C2 u |value| + the sine/cosine term of the closed forms above theta = 0.5: S: dT/theta, G: 3 (1 + theta) dT /
    theta^3, dT = 2^-53 + 2e-16."""
    dT = 2.0 ** -53 + 2e-16
    t = np.maximum(th, 0.5)
    coef = np.where(th >= 0.5, 1.0 / t if which == 0 else 3.0 * (1.0 + t) / t ** 3, 0.0)
    return C2["SG"[which]] * U * ref.abs + coef * dT


def moment_gate(m0_ref):
    """tests/test_rsd_cpu.py: MOMENT_ERR / 2 = 3 units of 2^-52 M_0."""
    return 3.0 * 2.0 ** -52 * m0_ref.abs


# ---------------------------------------------------------------- numpy restatements (the CPU test's independent side)
def _nested(y, n, ratio):
    """1 - y r_1 (1 - y r_2 (1 - ...)) through r_n; y is clipped where the series is not the branch that is read."""
    y = np.minimum(y, 8.0)
    s = np.ones_like(y)
    for j in range(n, 0, -1):
        s = 1.0 - y * ratio(j) * s
    return s


def j2_numpy(x):
    """jv(2, x) above the switch; below it the nested series (Cephes jv(2, x) is the recurrence there and cancels)."""
    from scipy.special import jv
    ax = np.abs(x)
    y = 0.25 * ax * ax
    return np.where(ax < 2.0, 0.5 * y * _nested(y, 12, lambda k: 1.0 / (k * (k + 2.0))), jv(2, ax))


def nodes_numpy(x):
    from scipy.special import j0, j1
    a, b = j0(x), j1(x)
    y = 0.25 * x * x
    hk, ag = x < 2.0, x < 5.0
    gc = x * (2.0 * b - x * a)
    xs = np.where(ag, 1.0, x)
    return {
        "g": np.where(hk, 2.0 * y * y * _nested(y, 10, lambda j: 1.0 / (j * (j + 2.0))), gc),
        "h1": np.where(hk, 0.5 * y * y * _nested(y, 10, lambda j: (j + 1.0) / (j * (j + 2.0) ** 2)), 2.0 * (1.0 - a) - x * b),
        "h2": np.where(hk, y ** 3 / 3.0 * _nested(y, 10, lambda j: (j + 1.0) / (j * (j + 2.0) * (j + 3.0))),
                       x * (x - 2.0 * b) - gc),
        "f1": np.where(ag, y ** 3 / 36.0 * _nested(y, 15, lambda j: (j + 2.0) / ((j + 3.0) * j * (j + 4.0))),
                       (x * b + (8.0 * a + 4.0)) - 24.0 * b / xs),
        "f2": np.where(ag, y ** 4 / 72.0 * _nested(y, 15, lambda j: (j + 2.0) / (j * (j + 4.0) ** 2)),
                       x * (8.0 * b + 2.0 * x) + (24.0 * (a - 1.0) + gc)),
    }


def panel_numpy(th):
    z = th * th
    s, c = np.sin(th), np.cos(th)
    ps = np.polyval([1 / 6227020800.0, -1 / 39916800.0, 1 / 362880.0, -1 / 5040.0, 1 / 120.0, -1 / 6.0, 1.0], z)
    pg = np.polyval([1 / 31135104000.0, -1 / 172972800.0, 1 / 1330560.0, -1 / 15120.0, 1 / 280.0, -1 / 10.0, 1.0], z)
    d = np.where(th < 0.5, 1.0, th)
    return np.where(th < 0.5, ps, s / d), np.where(th < 0.5, pg, 3.0 * (s - d * c) / d ** 3)


# ---------------------------------------------------------------- the comparisons, one per probe call
def _two_ulp(ref):
    return 2.0 * ref.ulp


def _banded(label, x, r, bands):
    """One entry per band of |x| (the ratio is reported as 0 outside it): a worst case of the phase term at 1e14 does
    not hide what the rational forms do below."""
    ax = np.abs(x)
    return {f"{label} {name}": np.where((ax >= lo) & (ax < hi), r, 0.0) for name, lo, hi in bands}


BESSEL_BANDS = (("|x|<=5", 0.0, np.nextafter(5.0, 9.0)), ("5<|x|<2^30", np.nextafter(5.0, 9.0), 2.0 ** 30),
                ("|x|>=2^30", 2.0 ** 30, np.inf))
NODE_BANDS = (("x<2", 0.0, 2.0), ("2<=x<5", 2.0, 5.0), ("x>=5", 5.0, np.inf))


def _bessel(name):
    def run(impl):
        x = j01_points() if name == "j01" else bessel_signed_points()
        r = ref_bessel(x)
        o0, o1 = impl(name, x)
        if name == "j01":
            return x, {**_banded("J0", x, ratio(r[0].err(o0), dJ(x, 0)), BESSEL_BANDS),
                       **_banded("J1", x, ratio(r[1].err(o1), dJ(x, 1)), BESSEL_BANDS)}
        if name == "j2":
            return x, _banded("J2", x, ratio(r[2].err(o0), j2_gate(x, r[2].abs)),
                              (("|x|<2", 0.0, 2.0), ("2<=|x|<=5", 2.0, BESSEL_BANDS[0][2])) + BESSEL_BANDS[1:])
        n = int(name[1])
        return x, _banded(name.upper(), x, ratio(r[n].err(o0), dJ(x, n)), BESSEL_BANDS)
    return run


def _i0e(impl):
    x = i0e_points()
    r = ref_i0e(x)
    return x, {"I0e": ratio(r.err(impl("i0e", x)[0]), i0e_gate(r.abs))}


def _sincos(name, points):
    def run(impl):
        x = points()
        rs, rc = ref_sincos(x)
        s, c = impl(name, x)
        return x, {"sin": ratio(rs.err(s), sincos_gate(x, rs)), "cos": ratio(rc.err(c), sincos_gate(x, rc))}
    return run


def _smyc(impl):
    x, y = smyc_points()
    r = ref_smyc(x, y)
    return x, {"|sin x - y cos x|": ratio(r.err(np.abs(impl("sin_minus_ycos", x, y)[0])), smyc_gate(y, r))}


def _rcp(name):
    def run(impl):
        x = rcp_points()
        r = ref_rcp(x)
        return x, {"1/x": ratio(r.err(impl(name, x)[0]), r.ulp)}
    return run


def _sici(impl):
    x = sici_points()
    rs, rc = ref_sici(x)
    si, ci = impl("sici", x)
    return x, {"Si": ratio(rs.err(si), sici_gate(x, rs)), "Ci": ratio(rc.err(ci), sici_gate(x, rc))}


def _aux(name):
    def run(impl):
        x = aux_points()
        rf, rg = ref_aux(x)
        f, g = impl(name, x)
        out = {"g": ratio(rg.err(g), aux_gate(x, rg, 1))}
        if name == "sici_aux_fg":
            out["f"] = ratio(rf.err(f), aux_gate(x, rf, 0))
        else:
            out["f == 0"] = np.where(f == 0.0, 0.0, np.inf)
        return x, out
    return run


def _fast(name, key, ref_fn, gate):
    def run(impl):
        x = fastmath_points()[key]
        r = ref_fn(x)
        return x, {name: ratio(r.err(impl(name, x)[0]), gate(r))}
    return run


def _gnfw(name):
    def run(impl):
        t, a, e = gnfw_points()
        if name == "gnfw_alpha1":
            a = np.ones_like(a)
        r = ref_gnfw(t, a, e)
        return t, {"rho": ratio(r.err(impl(name, t, a, e)[0]), 2e-14 * r.abs)}
    return run


def _nodes(name, first, second):
    def run(impl):
        x = node_points()
        r = ref_nodes(x)
        o = impl(name, x)
        out = {}
        for k, v in zip((first, second), o):
            if k:
                out.update(_banded(k, x, ratio(r[k].err(v), node_gate(x, k, r[k])), NODE_BANDS))
        return x, out
    return run


def _panel(impl):
    th = panel_points()
    rS, rG = ref_panel(th)
    S, G = impl("xi_panel", th)
    return th, {"S": ratio(rS.err(S), panel_gate(th, 0, rS)), "G": ratio(rG.err(G), panel_gate(th, 1, rG))}


def _gauss(name):
    def run(impl):
        t = moment_points()
        r = ref_moments(t)
        o = impl(name, t)
        ns = (0, 1) if name == "gauss_m0_m1" else (2,)
        return t, {f"M{n}": ratio(r[n].err(v), moment_gate(r[0])) for n, v in zip(ns, o)}
    return run


# name of the probe's function -> run(impl) -> (points, {label: err / gate at every point}); impl(name, x, y, z) returns
# the two outputs of the function on the device (``call``) or of the independent implementation
COMPARISONS = {
    "j0": _bessel("j0"), "j1": _bessel("j1"), "j2": _bessel("j2"), "j01": _bessel("j01"), "i0e": _i0e,
    "sincos_fast": _sincos("sincos_fast", sincos_points), "xi_sincos": _sincos("xi_sincos", xi_sincos_points),
    "sin_minus_ycos": _smyc, "rcp_fast": _rcp("rcp_fast"), "fm_rcp": _rcp("fm_rcp"), "sici": _sici,
    "sici_aux_fg": _aux("sici_aux_fg"), "sici_aux_g": _aux("sici_aux_g"),
    "log": _fast("log", "log", ref_log, _two_ulp), "exp_clamp": _fast("exp_clamp", "exp", ref_exp, _two_ulp),
    "exp_noclamp": _fast("exp_noclamp", "exp", ref_exp, _two_ulp),
    "log1p": _fast("log1p", "log1p", ref_log1p, _two_ulp),
    "log1p_abs": _fast("log1p_abs", "log1p", ref_log1p, lambda r: 1.2e-16 + 2.0 * r.ulp),
    "gnfw": _gnfw("gnfw"), "gnfw_alpha1": _gnfw("gnfw_alpha1"),
    "node_g_h2": _nodes("node_g_h2", "g", "h2"), "node_h1_g4": _nodes("node_h1_g4", "h1", "f1"),
    "node_f2": _nodes("node_f2", "f2", None), "xi_panel": _panel,
    "gauss_m0_m1": _gauss("gauss_m0_m1"), "gauss_m2": _gauss("gauss_m2"),
}
assert set(COMPARISONS) == set(FN)


def worst(points, ratios):
    """{label: (worst ratio, the point it is at)}; a NaN ratio counts as infinite."""
    out = {}
    for k, r in ratios.items():
        r = np.where(np.isnan(r), np.inf, r)
        i = int(np.argmax(r))
        out[k] = (float(r[i]), float(points[i]))
    return out


def report(name, points, ratios):
    w = worst(points, ratios)
    for k, (v, at) in w.items():
        print(f"    {name:15s} {k:20s} worst |got - ref| / gate = {v:8.4g} at {at!r}   ({points.size} points)")
    return w
