"""The one-point PDF, the parts that need no GPU: the transform against a closed form, the grid
in lambda and the ring rule, the ring rule's error on the truncated pressure profile (which sets the default number of
rings and the gate of the GPU end-to-end test), the ABI and the exports, and the argument checks."""
import inspect
import os
import re
import sys

import numpy as np
import pytest
from scipy.stats import norm, poisson

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import gas_profile_model as gm  # noqa: E402
import onepoint_model as om  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps
# the two pressure-like rows of tests/test_gpu_gas_profiles.py::ROWS, (alpha, eta, gamma)
PRESSURE_ROWS = [(1.0, 4.35, -0.3), (1.0, 6.0, -0.3)]
RING_XCUTS = (2.0, 4.0, 20.0)
RING_ERROR, RING_GATE = om.RING_ERROR, om.RING_GATE      # what test 3 measures, and the GPU gate built on it


# ---------------------------------------------------------------- 1. the transform against a closed form
def test_pdf_of_a_single_ring_is_the_poisson_mixture_of_gaussians():
    """A = mu (exp(i lambda s0) - 1): k ~ Poisson(mu) rings of signal s0 each, plus Gaussian noise."""
    from hmvec_amd import onepoint
    N, ds, mu = 256, 0.01, 1.7
    s0, sigma, smin = 7.3 * ds, 3 * ds, -20 * ds
    nl, dl = onepoint.lambda_grid(N, ds)
    lam = dl * np.arange(nl)
    s, p = onepoint.pdf_from_exponent(mu * (np.exp(1j * lam * s0) - 1.0), ds, smin=smin, noise_sigma=sigma)
    assert s.shape == p.shape == (N,) and np.array_equal(s, smin + ds * np.arange(N))
    ref = np.zeros(N)
    for k in range(120):
        for image in (-1, 0, 1):
            ref += ds * poisson.pmf(k, mu) * norm.pdf(s + image * N * ds, k * s0, sigma)
    print(f"max |dp| = {np.abs(p - ref).max():.2e}, sum p - 1 = {p.sum() - 1:.2e}, "
          f"sum p s - mu s0 = {np.sum(p * s) - mu * s0:.2e}")
    assert np.abs(p - ref).max() <= 1e-15
    assert abs(p.sum() - 1.0) <= 1e-14
    assert abs(np.sum(p * s) - mu * s0) <= 1e-9
    # the model's direct sum agrees with the FFT
    assert np.abs(om.pdf(mu * (np.exp(1j * lam * s0) - 1.0), ds, smin, sigma)[1] - p).max() <= 1e-15


# ---------------------------------------------------------------- 2. the grid in lambda and the ring rule
def test_lambda_grid_values_and_refusals():
    from hmvec_amd import onepoint
    nl, dl = onepoint.lambda_grid(512, 0.25)
    assert nl == 257 and dl == 2.0 * np.pi / (512 * 0.25)
    assert onepoint.lambda_grid(4, 1.0)[0] == 3
    assert onepoint.lambda_grid(onepoint.MAX_BINS, 1.0)[0] == onepoint.MAX_BINS // 2 + 1
    for bad in (3, 5, 2, 0, -4, onepoint.MAX_BINS + 2, 8.0, "8", None, True):
        with pytest.raises(ValueError, match="nbins"):
            onepoint.lambda_grid(bad, 1.0)
    for bad in (0.0, -1.0, np.nan, np.inf, None, "x"):
        with pytest.raises(ValueError, match="ds"):
            onepoint.lambda_grid(8, bad)


@pytest.mark.parametrize("ntheta", [8, 64])
def test_ring_rule_is_gauss_legendre_on_the_unit_interval(ntheta):
    from hmvec_amd import onepoint
    u, w = onepoint.ring_rule(ntheta)
    assert u.shape == w.shape == (ntheta,) and np.all(np.diff(u) > 0) and u[0] > 0 and u[-1] < 1 and np.all(w > 0)
    x, wx = np.polynomial.legendre.leggauss(ntheta)
    assert np.array_equal(u, 0.5 * (x + 1.0)) and np.array_equal(w, 0.5 * wx)
    assert abs(np.sum(2.0 * u * w) - 1.0) <= 4 * EPS            # the disc's area: sum a_t = pi theta_out^2
    assert abs(np.sum(u ** 3 * w) / 0.25 - 1.0) <= 4 * EPS      # int_0^1 u^3 du, exact for the rule


def test_ring_rule_refusals_and_default():
    from hmvec_amd import onepoint
    assert onepoint.ring_rule()[0].size == onepoint.DEFAULT_RINGS
    for bad in (1, 0, -3, onepoint.MAX_RINGS + 1, 64.0, None, True):
        with pytest.raises(ValueError, match="ntheta"):
            onepoint.ring_rule(bad)


def test_chain_length_mirrors_the_kernels_constants():
    from hmvec_amd import onepoint
    src = open(os.path.join(REPO, "hmvec_amd", "csrc", "kernels", "onepoint.hpp")).read()
    const = {k: int(v) for k, v in re.findall(r"constexpr int (OP_[A-Z]+) = (\d+);", src)}
    assert (const["OP_THREADS"], const["OP_RADIX"], const["OP_SLICE"], const["OP_MAXSPLIT"]) == \
        (onepoint._THREADS, onepoint._RADIX, onepoint._SLICE, onepoint._MAXSPLIT)
    assert onepoint._WAVES == onepoint._THREADS // 64
    # one sample: one addition on each of: the first rung, the three of the ladder's total, the four wavefronts'
    # three - against the moments' 1 + 3 + 8
    assert onepoint.chain_length(1, 1) == 12
    assert onepoint.chain_length(512, 64) == 8 + 8 + 8 + 2 + 3 + 3 + 7
    for nm, nt in ((1, 1), (5, 7), (16, 64), (67, 33), (130, 33), (3, 7), (1, 64), (65, 33)):
        assert onepoint.chain_length(nm, nt) <= 64
    with pytest.raises(ValueError):
        onepoint.chain_length(0, 4)


# ---------------------------------------------------------------- 3. the ring rule on the truncated pressure profile
def ring_error(ntheta):
    from hmvec_amd import onepoint
    u, w = onepoint.ring_rule(ntheta)
    worst = 0.0
    for alpha, eta, gamma in PRESSURE_ROWS:
        for xcut in RING_XCUTS:
            F = np.array([gm.F_proj(xcut * ut, alpha, gamma, eta, xcut) for ut in u])
            got = np.sum(2.0 * np.pi * xcut ** 2 * u * w * F)
            worst = max(worst, abs(got / gm.N_total(alpha, gamma, eta, xcut) - 1.0))
    return worst


def test_ring_rule_integrates_the_truncated_pressure_profile():
    """sum_t 2 pi xcut^2 u_t w_t F(xcut u_t) against N_total = 4 pi int_0^xcut x^2 f dx (the disc integral of the
    projection is the volume integral of the profile) for the two pressure-like rows at xcut in {2, 4, 20}.

    Measured worst relative error: 5.27e-7 with 64 rings, 4.70e-8 with 128, 5.91e-9 with 256.  F ends in a square root
    at the cut, so the rule converges like ntheta^-3 only; 64 rings alone miss 1e-8, and the default number of rings is
    therefore 256, the first power of two below it.  The gate of the end-to-end GPU test is
    min(1e-6, max(1e-10, 100 x 5.91e-9)) = 5.91e-7, the convention of tests/test_gpu_gas_profiles.py."""
    from hmvec_amd import onepoint
    e64, edef = ring_error(64), ring_error(onepoint.DEFAULT_RINGS)
    print(f"ring rule on the truncated pressure profile: 64 rings {e64:.3e}, {onepoint.DEFAULT_RINGS} rings {edef:.3e}")
    assert onepoint.DEFAULT_RINGS == 256
    assert edef <= 1e-8 < e64 <= 1e-6
    assert edef <= RING_ERROR * 1.01          # the figure the gate is built on is the measured one
    assert RING_GATE == pytest.approx(5.91e-7)


# ---------------------------------------------------------------- 4. ABI and exports
def test_entry_points_are_declared_and_bound_and_the_abi_version_stays():
    from hmvec_amd import _native as nat
    header = open(os.path.join(REPO, "include", "hmgrid.h")).read()
    for name, nargs in (("hmg_onepoint_exponent", 16), ("hmg_onepoint_moments", 14)):
        m = re.search(r"\bint " + name + r"\(hmg_ctx\* ctx, int nz, int nm, int nt, ([^;]*)\);", header)
        assert m, name
        declared = re.sub(r"/\*.*?\*/", "", m.group(0), flags=re.S)
        assert declared.count(",") + 1 == nargs == len(nat.SIGNATURES[name])
    assert nat.SIGNATURES["hmg_onepoint_exponent"][-4:-2] == [nat._I, nat._D]           # nlambda, dlambda
    assert int(re.search(r"#define HMG_ABI_VERSION (\d+)", header).group(1)) == 10 == nat.ABI_VERSION
    mk = open(os.path.join(REPO, "hmvec_amd", "csrc", "Makefile")).read()
    assert re.search(r"^KUNITS = .*\bonepoint\b", mk, flags=re.M) and re.search(r"^DEPS_onepoint\s*=", mk, flags=re.M)


def test_exports():
    import hmvec_amd
    from hmvec_amd import onepoint
    for name in ("char_exponent", "cumulants", "pdf_from_exponent", "lambda_grid", "ring_rule"):
        assert getattr(hmvec_amd, name) is getattr(onepoint, name) and name in hmvec_amd.__all__ and name in onepoint.__all__
    assert hmvec_amd.onepoint is onepoint and "onepoint" in hmvec_amd.__all__
    assert "chain_length" in onepoint.__all__ and "MAX_BINS" in onepoint.__all__
    for name in ("profile_char_exponent", "get_y_char_exponent", "get_y_pdf", "get_y_cumulants"):
        assert callable(getattr(hmvec_amd.HaloModel, name))
    tail = ["ntheta", "mmin", "mmax", "zweights", "per_z"]
    for name in ("profile_char_exponent", "get_y_char_exponent", "get_y_pdf", "get_y_cumulants"):
        par = inspect.signature(getattr(hmvec_amd.HaloModel, name)).parameters
        assert list(par)[-5:] == tail and par["ntheta"].default == onepoint.DEFAULT_RINGS and par["per_z"].default is False
    par = inspect.signature(onepoint.char_exponent).parameters
    assert list(par) == ["signal", "area", "nzm", "wm", "zw", "nlambda", "dlambda", "mwindow", "per_z", "ctx"]
    assert list(inspect.signature(onepoint.cumulants).parameters) == ["signal", "area", "nzm", "wm", "zw", "mwindow", "per_z",
                                                                     "ctx"]


# ---------------------------------------------------------------- 5. every refusal happens on the host
class _NoContext:
    """Stands where a context would: any use of it is a launch that should not have happened."""

    def __getattr__(self, name):
        raise AssertionError(f"the context was used ({name}) before the arguments were checked")


NZ, NM, NT = 2, 5, 4


def _good():
    rng = np.random.default_rng(3)
    return dict(signal=rng.uniform(0.1, 1, (NZ, NM, NT)), area=rng.uniform(0.1, 1, (NZ, NM, NT)),
                nzm=rng.uniform(0.1, 1, (NZ, NM)), wm=rng.uniform(0.1, 1, NM), zw=rng.uniform(0.1, 1, NZ))


BAD_ARRAYS = [
    dict(signal=np.ones((NZ, NM))), dict(signal=np.ones((NZ, NM, 0))), dict(area=np.ones((NZ, NM, NT + 1))),
    dict(nzm=np.ones((NZ, NM + 1))), dict(wm=np.ones(NM - 1)), dict(zw=np.ones(NZ + 1)), dict(zw=np.ones((NZ, 1))),
    dict(signal=np.full((NZ, NM, NT), np.nan)), dict(area=np.full((NZ, NM, NT), np.inf)),
    dict(nzm=np.full((NZ, NM), np.nan)), dict(wm=np.full(NM, np.inf)), dict(zw=np.full(NZ, np.nan)),
    dict(mwindow=(2, 2)), dict(mwindow=(3, 1)), dict(mwindow=(0, NM + 1)), dict(mwindow=(-1, 2)), dict(mwindow=(0.0, 2)),
    dict(mwindow=3), dict(mwindow=(0, 1, 2)),
]


@pytest.mark.parametrize("kw", BAD_ARRAYS)
def test_free_functions_refuse_bad_arrays_on_the_host(kw):
    from hmvec_amd import onepoint
    args = {**_good(), **kw}
    with pytest.raises(ValueError):
        onepoint.char_exponent(nlambda=5, dlambda=0.3, ctx=_NoContext(), **args)
    with pytest.raises(ValueError):
        onepoint.cumulants(ctx=_NoContext(), **args)


def test_free_functions_refuse_a_bad_grid_on_the_host_and_a_good_request_reaches_the_context():
    from hmvec_amd import onepoint
    for bad in (dict(nlambda=0), dict(nlambda=-1), dict(nlambda=2.0), dict(nlambda=onepoint.MAX_BINS),
                dict(dlambda=0.0), dict(dlambda=-0.1), dict(dlambda=np.nan), dict(dlambda=np.inf)):
        with pytest.raises(ValueError, match="lambda"):
            onepoint.char_exponent(ctx=_NoContext(), **{**_good(), **dict(nlambda=5, dlambda=0.3), **bad})
    with pytest.raises(AssertionError, match="the context was used"):
        onepoint.char_exponent(nlambda=5, dlambda=0.3, ctx=_NoContext(), **_good())
    with pytest.raises(AssertionError, match="the context was used"):
        onepoint.cumulants(ctx=_NoContext(), **_good())


def test_pdf_from_exponent_refusals():
    from hmvec_amd import onepoint
    A = np.zeros(9, dtype=complex)
    for bad in (dict(A=np.zeros((2, 9))), dict(A=np.zeros(2)), dict(A=np.array([0, np.nan, 0])), dict(ds=0.0),
                dict(ds=np.inf), dict(noise_sigma=-1.0), dict(noise_sigma=np.nan), dict(smin=np.inf)):
        with pytest.raises(ValueError):
            onepoint.pdf_from_exponent(**{**dict(A=A, ds=0.1), **bad})
    s, p = onepoint.pdf_from_exponent(A, 0.1)          # A = 0: no halo anywhere, all of the probability at s = 0
    assert p[0] == pytest.approx(1.0) and np.abs(p[1:]).max() < 1e-15


def _host_model():
    """A HaloModel without its constructor: the host attributes the argument checks read; whatever reaches the device
    (_main, _onepoint_launch) fails the test."""
    import hmvec_amd as hm
    h = hm.HaloModel.__new__(hm.HaloModel)
    h.zs, h.ms = np.array([0.2, 0.6]), np.geomspace(1e12, 1e15, NM)
    h.mdef, h.p, h.h, h.omm0 = "vir", dict(hm.default_params), 0.68, 0.31

    def launched(*a, **k):
        raise AssertionError("a refused request reached the launch")
    h._main = h._onepoint_launch = launched
    return h


COMMON_BAD = [dict(ntheta=1), dict(ntheta=5000), dict(ntheta=64.0), dict(mmin=1e16), dict(mmax=1e11), dict(mmin=2e13, mmax=1e13),
              dict(mmin=-1.0), dict(mmax=np.nan), dict(zweights=np.ones(3)), dict(zweights=[1.0, np.nan]),
              dict(zweights=np.ones((2, 1)))]


@pytest.mark.parametrize("kw", COMMON_BAD + [
    dict(nbins=7), dict(nbins=2), dict(nbins=256.0), dict(ds=0.0), dict(ds=np.nan),
    dict(profiles=np.ones((NZ, NM, 9))), dict(profiles=np.ones((NZ, NM))), dict(profiles=np.full((NZ, NM, 8), np.nan)),
    dict(theta_out=np.ones((NZ, NM + 1))), dict(theta_out=np.zeros((NZ, NM))), dict(theta_out=np.full((NZ, NM), np.inf)),
    dict(theta_out=-np.ones((NZ, NM)))])
def test_profile_char_exponent_refuses_on_the_host(kw):
    args = dict(profiles=np.ones((NZ, NM, 8)), theta_out=np.full((NZ, NM), 1e-3), nbins=64, ds=0.1, ntheta=8,
                zweights=np.ones(NZ))
    with pytest.raises(AssertionError, match="reached the launch"):      # (a good request gets as far as the launch)
        _host_model().profile_char_exponent(**args)
    with pytest.raises(ValueError):
        _host_model().profile_char_exponent(**{**args, **kw})


Y_BAD = COMMON_BAD + [dict(fwhm=-1e-4), dict(fwhm=np.nan), dict(truncate=0.0), dict(truncate=np.inf), dict(family="nosuch")]
GRID_BAD = [dict(nbins=7), dict(nbins=0), dict(dy=0.0), dict(dy=np.inf)]
PDF_BAD = [dict(noise_sigma=-1e-7), dict(noise_sigma=np.nan), dict(ymin=np.nan)]
Y_CASES = ([("get_y_cumulants", kw) for kw in Y_BAD] + [("get_y_char_exponent", kw) for kw in Y_BAD + GRID_BAD]
           + [("get_y_pdf", kw) for kw in Y_BAD + GRID_BAD + PDF_BAD])


@pytest.mark.parametrize("method,kw", Y_CASES)
def test_y_methods_refuse_on_the_host(method, kw):
    args = dict(ntheta=8, zweights=np.ones(NZ))
    if method != "get_y_cumulants":
        args.update(nbins=64, dy=1e-7)
    with pytest.raises((ValueError, KeyError)):
        getattr(_host_model(), method)(**{**args, **kw})


def test_one_redshift_needs_its_weight():
    h = _host_model()
    h.zs = np.array([0.4])
    with pytest.raises(ValueError, match="zweights"):
        h.profile_char_exponent(np.ones((1, NM, 8)), np.full((1, NM), 1e-3), 64, 0.1, ntheta=8)
    with pytest.raises(ValueError, match="zweights"):
        h.get_y_cumulants(ntheta=8)
