"""What keeps tests/test_gpu_math_probe.py honest, without a device.

* The probe (tests/hip/math_probe.hip) cross-compiles with the library's own flags: every header it includes still
  builds into it, and the .so is left next to the source for a run on the device.
* The point sets, 50-digit references and gates of helpers/math_probe.py, which the device test shares, are met at EVERY
  point by an implementation that owes nothing to the headers: SciPy's Cephes j0 / j1 / jv / i0e / sici, numpy's
  sin / cos / division, a quadrature of the integrals that define f and g, numpy restatements of the series and closed
  forms of the node functions, and the host builds of fastmath.hpp and gauss_moments.hpp (tests/cpp).  A reference or a
  gate that were wrong would fail here first.  (G_4 of kernels/bessel_g4.hpp is checked through the numpy restatement:
  the header's existing host build, tests/cpp/angcov_host.cpp, prints bin weights, not G_4.)
* The constants that were set as "twice what the independent implementation measures" are re-measured: the independent
  implementation stays inside half of them.

Worst |independent - mpmath| / gate, as this test prints them (2026-10-21, SciPy 1.15.3, mpmath 1.3.0):
    j0 (|x| <= 5, to 2^30, beyond) 0.344, 0.932, 0.937 - above 5 the phase term alone, x - pi/4 rounded once
    j1 0.210, 0.882, 0.956   j2 0.412 (series), 0.199, 0.221, 0.000   j01 as j0 and j1   i0e 0.414
    sincos_fast 0.488 / 0.499   xi_sincos 0.488 / 0.473   sin_minus_ycos 0.379   rcp 0.5   Si 0.485   Ci 0.490
    f 0.287   g 0.244 (quadrature)   log 0.353   exp 0.407   log1p 0.553   log1p_abs 0.925   gnfw 0.307   gnfw_alpha1 0.136
    (x < 2, to 5, beyond)  g 0.450, 0.126, 0.935   H2 0.483, 0.166, 0.918   H1 0.189, 0.095, 0.885
    F1 0.248, 0.336, 0.885   F2 0.413, 0.490, 0.878   S 0.414   G 0.543   M0 0.322   M1 0.128   M2 0.169
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import math_probe as mpb  # noqa: E402


@pytest.fixture(scope="module")
def fastmath(tmp_path_factory):
    out = tmp_path_factory.mktemp("probe_fastmath") / "libfastmath_host.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC",
                    os.path.join(HERE, "cpp", "fastmath_host.cpp"), "-o", str(out)], check=True)
    lib = ctypes.CDLL(str(out))

    def fm(name, x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        o = np.empty_like(x)
        getattr(lib, name)(ctypes.c_void_p(x.ctypes.data), ctypes.c_int(x.size), ctypes.c_void_p(o.ctypes.data))
        return o
    return fm


@pytest.fixture(scope="module")
def moments_host(tmp_path_factory):
    exe = tmp_path_factory.mktemp("probe_moments") / "gauss_moments_host"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", os.path.join(HERE, "cpp", "gauss_moments_host.cpp"),
                    "-o", str(exe)], check=True)

    def run(t):
        r = subprocess.run([str(exe)], input="".join(float(v).hex() + "\n" for v in t), capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        got = np.array([[float.fromhex(v) for v in line.split()] for line in r.stdout.splitlines()]).T
        assert got.shape == (3, len(t))
        return got
    return run


@pytest.fixture(scope="module")
def independent(fastmath, moments_host):
    """impl(name, x, y, z) -> (out0, out1) from code that shares nothing with the device headers (the two host builds
    share the SOURCE of fastmath.hpp and gauss_moments.hpp, not the device's reciprocal, inline assembly or contraction:
    they are the figures the headers' comments quote)."""
    from scipy import special as sp

    def impl(name, x, y=None, z=None):
        zero = np.zeros_like(x)
        if name in ("j0", "j1"):
            return getattr(sp, name)(x), zero
        if name == "j2":
            return mpb.j2_numpy(x), zero
        if name == "j01":
            return sp.j0(x), sp.j1(x)
        if name == "i0e":
            return sp.i0e(x), zero
        if name in ("sincos_fast", "xi_sincos"):
            return np.sin(x), np.cos(x)
        if name == "sin_minus_ycos":
            return np.sin(x) - y * np.cos(x), zero
        if name in ("rcp_fast", "fm_rcp"):
            return 1.0 / x, zero
        if name == "sici":
            return sp.sici(x)
        if name == "sici_aux_fg":
            return mpb.aux_quad(x)
        if name == "sici_aux_g":
            return zero, mpb.aux_quad(x)[1]
        host = {"log": "fm_log", "exp_clamp": "fm_exp", "exp_noclamp": "fm_exp_nc", "log1p": "fm_log1p",
                "log1p_abs": "fm_log1p_abs"}
        if name in host:
            return fastmath(host[name], x), zero
        if name in ("gnfw", "gnfw_alpha1"):
            lt = fastmath("fm_log", x)
            ta = x if name == "gnfw_alpha1" else fastmath("fm_exp_nc", y * lt)
            return fastmath("fm_exp_nc", mpb.GNFW_GAMMA * lt - z * fastmath("fm_log1p_abs", ta)), zero
        if name.startswith("node_"):
            n = mpb.nodes_numpy(x)
            return {"node_g_h2": (n["g"], n["h2"]), "node_h1_g4": (n["h1"], n["f1"]), "node_f2": (n["f2"], zero)}[name]
        if name == "xi_panel":
            return mpb.panel_numpy(x)
        m = moments_host(x)
        return (m[0], m[1]) if name == "gauss_m0_m1" else (m[2], zero)
    return impl


def test_the_probe_cross_compiles_and_loads():
    """With hipcc and the Makefile's flags; a stale or missing .so that cannot be rebuilt FAILS here (no skip)."""
    flags = mpb.cxxflags()
    assert "--offload-arch=gfx950" in flags and "-disable-machine-licm" in flags and "-O3" in flags
    path = mpb.build(force=True)
    assert path == mpb.LIB and os.path.getmtime(path) >= mpb._newest_source()
    assert mpb.build() == path                                        # current: not rebuilt
    lib = ctypes.CDLL(path)
    lib.math_probe_run.restype = ctypes.c_int
    # argument checks come before the first HIP call: no device is touched
    x = np.ones(4)
    assert lib.math_probe_run(len(mpb.FN), 4, ctypes.c_void_p(x.ctypes.data), None, None, ctypes.c_void_p(x.ctypes.data),
                              ctypes.c_void_p(x.ctypes.data)) == -1
    assert lib.math_probe_run(0, 0, None, None, None, None, None) == -1


def test_a_probe_that_cannot_be_built_is_an_error(monkeypatch, tmp_path):
    monkeypatch.setattr(mpb, "LIB", str(tmp_path / "libmathprobe.so"))
    monkeypatch.setenv("HIPCC", str(tmp_path / "no-such-hipcc"))
    with pytest.raises(mpb.ProbeBuildError, match="hipcc could not be run"):
        mpb.build()


def test_the_function_ids_are_the_probe_s():
    src = open(mpb.SRC).read()
    body = src[src.index("enum Fn : int {"):src.index("FN_COUNT")]
    ids = [t.split("=")[0].strip() for t in body.split("{")[1].replace("\n", " ").split(",") if t.strip()]
    want = {"j0": "FN_J0", "sin_minus_ycos": "FN_SIN_MINUS_YCOS", "sici": "FN_SICI", "exp_clamp": "FN_EXP_CLAMP",
            "gnfw_alpha1": "FN_GNFW_ALPHA1", "node_f2": "FN_NODE_F2", "gauss_m2": "FN_GAUSS_M2"}
    assert len(ids) == len(mpb.FN)
    for name, enum in want.items():
        assert ids[mpb.FN[name]] == enum
    assert f"GNFW_GAMMA = {mpb.GNFW_GAMMA}" in src


@pytest.mark.parametrize("name", list(mpb.COMPARISONS))
def test_independent_implementation_meets_every_gate(independent, name):
    points, ratios = mpb.COMPARISONS[name](independent)
    w = mpb.report(name, points, ratios)
    for k, r in ratios.items():
        assert r.shape == points.shape                                # every point is in the comparison
    assert all(v <= 1.0 for v, _ in w.values()), w


def test_the_measured_constants_hold():
    """Half of each gate that was set as twice a measurement, on the test's own sets (MEASURED is from denser ones)."""
    from scipy import special as sp
    x = mpb.bessel_signed_points()
    ax = np.abs(x)
    r = mpb.ref_bessel(x)
    for n, fn in ((0, sp.j0), (1, sp.j1)):
        s = np.ones_like(ax) if n == 0 else np.minimum(1.0, ax)
        over = np.maximum(r[n].err(fn(x)) - mpb.phase_term(x), 0.0)
        units = mpb.ratio(over, mpb.U * s)
        print(f"    scipy j{n}: worst {units.max():.3g} u s(x) beyond the phase term (C_J = {mpb.C_J})")
        assert units.max() <= mpb.C_J / 2 and mpb.MEASURED[f"j{n}"] <= mpb.C_J / 2
    below = ax < 2.0
    units = mpb.ratio(r[2].err(mpb.j2_numpy(x))[below], mpb.U * r[2].abs[below])
    print(f"    J2 series restated: worst {units.max():.3g} u (C_J2_SERIES = {mpb.C_J2_SERIES})")
    assert units.max() <= mpb.C_J2_SERIES / 2
    x = mpb.i0e_points()
    ri = mpb.ref_i0e(x)
    units = mpb.ratio(ri.err(sp.i0e(x)), 2.0 ** -52 * ri.abs)
    print(f"    scipy i0e: worst {units.max():.3g} x 2^-52 (C_I0E = {mpb.C_I0E})")
    assert units.max() <= mpb.C_I0E / 2
    x = mpb.node_points()
    rn, nn, coef = mpb.ref_nodes(x), mpb.nodes_numpy(x), mpb.node_coef(x)
    for k in ("g", "h2", "f2"):
        over = np.maximum(rn[k].err(nn[k]) - coef[k] * mpb.dJ(np.maximum(x, 1.0), 0), 0.0)
        units = mpb.ratio(over, mpb.U * rn[k].abs)
        print(f"    {k} restated: worst {units.max():.3g} u |value| beyond coef dJ (C2 = {mpb.C2[k]})")
        assert units.max() <= mpb.C2[k] / 2
    th = mpb.panel_points()
    for w, (rr, got) in enumerate(zip(mpb.ref_panel(th), mpb.panel_numpy(th))):
        k = "SG"[w]
        over = np.maximum(rr.err(got) - (mpb.panel_gate(th, w, rr) - mpb.C2[k] * mpb.U * rr.abs), 0.0)
        units = mpb.ratio(over, mpb.U * rr.abs)
        print(f"    {k} restated: worst {units.max():.3g} u |value| (C2 = {mpb.C2[k]})")
        assert units.max() <= mpb.C2[k] / 2


def test_exp_forms_agree_and_special_values(fastmath):
    y = mpb.fastmath_points()["exp"]
    assert np.all(np.abs(y) < 700.0)
    assert np.array_equal(fastmath("fm_exp_nc", y), fastmath("fm_exp", y))
    assert fastmath("fm_log1p", np.zeros(1))[0] == 0.0


def test_the_point_sets_hit_what_they_are_for():
    x = mpb.bessel_points()
    for v in (0.0, 1e-300, 2.0, 5.0, np.nextafter(5.0, 0.0), np.nextafter(5.0, 9.0), np.nextafter(2.0, 0.0)):
        assert v in x
    assert np.sum(x >= 2.0 ** 30) >= 100 and np.sum((x > 0) & (x <= 5)) >= 300
    assert np.sum(mpb.bessel_signed_points() < 0) >= 100
    j = mpb.j01_points()
    assert 2.0 ** 30 in j and np.sum((j - 0.7853981633974483 >= 2.0 ** 30) & (j < 2.0 ** 30 + 2)) >= 2
    s = mpb.sincos_points()
    assert s.min() == 0.0 and s.max() < 2.0 ** 30 and np.sum(s > 1e9) >= 10
    xs = mpb.xi_sincos_points()
    assert np.nextafter(2.0 ** 30, 0.0) in xs and 2.0 ** 30 in xs and xs.max() > 1e14
    a = mpb.aux_points()
    assert a.min() > 4.0 and all(v in a for v in (np.nextafter(8.0, 0.0), 8.0, np.nextafter(64.0, 0.0), 64.0))
    n = mpb.node_points()
    assert n.min() == 1e-8 and n.max() == 1e6
    sizes = {f.__name__: f()[0].size if isinstance(f(), tuple) else f().size
             for f in (mpb.bessel_signed_points, mpb.j01_points, mpb.i0e_points, mpb.sincos_points, mpb.xi_sincos_points,
                       mpb.smyc_points, mpb.rcp_points, mpb.sici_points, mpb.node_points, mpb.panel_points,
                       mpb.moment_points, mpb.gnfw_points)}
    assert max(sizes.values()) <= 4000, sizes                          # "a few thousand points" per probe call
    assert all(v.size <= 4000 for v in mpb.fastmath_points().values())
