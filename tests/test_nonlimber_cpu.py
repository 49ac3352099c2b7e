"""CPU checks of the non-Limber two-halo projection (hmvec_amd.nonlimber); no GPU.

The numpy restatement (tests/helpers/nonlimber_model.py) and the host build of hmvec_amd/csrc/sphbessel.hpp
(tests/cpp/sphbessel_host.cpp, plain and under AddressSanitizer + UBSan, a program of its own) are measured against
40-digit mpmath at the points the device test uses.  The worst constants of the restatement, in units of 2^-53:

    CJ_ABS = 100.6   |err| / max(|j_l|, min(1, 1/x))        (l = 193, x = 252.73, lmax = 256)
    CJ_REL =  75.6   |err| / |j_l| where x < l

(the host build of the header, with its fused steps: 75.6 and 44.5).  The device's gate is 4 CJ_ABS.  The Gaussian-window
case of the issue fixes the physics: the Limber-to-exact ratios, the convergence of coarse rules, the lensing kind's
Limber limit and the sign of the Kaiser term.  Then the exports, every refusal, the ABI and the launches of a request of
17 fields against the recording stand-in."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "helpers"))
import nonlimber_model as nlm  # noqa: E402
import recording_context as rc  # noqa: E402

import hmvec_amd  # noqa: E402
from hmvec_amd import _native as nat  # noqa: E402
from hmvec_amd import nonlimber  # noqa: E402

CJ_ABS, CJ_REL = 100.6, 75.6          # measured (this file's first test prints them); the gates below are these, rounded up
CJ_GATE = 101.0


# ---------------------------------------------------------------- 1. j_l against mpmath
def test_restatement_bessel_against_mpmath():
    worst_abs = worst_rel = 0.0
    for lmax in nlm.PROBE_LMAX:
        xs = nlm.probe_points(lmax)
        got = nlm.sph_bessel(lmax, xs)
        assert got.shape == (lmax + 1, xs.size) and np.all(np.isfinite(got))
        a, r, _ = nlm.bessel_errors(lmax, xs, got)
        print(f"lmax {lmax}: worst absolute constant {a:.1f}, relative (x < l) {r:.1f}")
        worst_abs, worst_rel = max(worst_abs, a), max(worst_rel, r)
    print(f"restatement: CJ_ABS {worst_abs:.1f}, CJ_REL {worst_rel:.1f}")
    assert worst_abs <= CJ_GATE and worst_rel <= CJ_GATE
    assert abs(worst_abs - CJ_ABS) < 0.5 and abs(worst_rel - CJ_REL) < 0.5          # the recorded constants are these
    # underflow: exact zeros, never NaN (x = 0.05: j_l is below the denormals from l = 102 on)
    col = nlm.sph_bessel(256, [0.05])[:, 0]
    assert np.all(col[102:] == 0.0) and np.all(col[:91] > 0.0) and np.all(np.diff(col[:103]) < 0)


@pytest.mark.parametrize("flags", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g")],
                         ids=["plain", "asan_ubsan"])
def test_header_host_build_against_mpmath(tmp_path, flags):
    exe = tmp_path / "sphbessel_host"
    src = os.path.join(HERE, "cpp", "sphbessel_host.cpp")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wno-unknown-pragmas", "-Werror", "-ffp-contract=off", *flags, src,
                    "-o", str(exe)], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1")
    worst = 0.0
    for lmax in nlm.PROBE_LMAX if not flags else (17, 256):
        xs = nlm.probe_points(lmax)
        lines = "".join(f"{float(lmax).hex()} {float(x).hex()}\n" for x in xs)
        r = subprocess.run([str(exe)], input=lines, env=env, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        got = np.array([[float.fromhex(v) for v in line.split()] for line in r.stdout.splitlines()]).T
        assert got.shape == (lmax + 1, xs.size)
        if not flags:
            a, rel, _ = nlm.bessel_errors(lmax, xs, got)
            print(f"header, lmax {lmax}: worst absolute constant {a:.1f}, relative {rel:.1f}")
            worst = max(worst, a)
            ref = nlm.sph_bessel(lmax, xs)
            env_ = np.maximum(np.abs(ref), np.minimum(1.0, 1.0 / xs)[None, :])
            assert np.all(np.abs(got - ref) <= 5.0 * CJ_GATE * nlm.U * env_)
    assert worst <= 4.0 * CJ_GATE


@pytest.mark.parametrize("l", [0, 1, 2, 3, 50])
def test_second_derivative_identity_against_mpmath(l):
    import mpmath as mp
    with mp.workdps(40):
        def j(n, x):
            return mp.sqrt(mp.pi / (2 * x)) * mp.besselj(n + mp.mpf(1) / 2, x)
        cm, c0, cp = (mp.mpf(float(c)) for c in nlm.jpp_coefficients(l))
        for x in (0.7, 5.3, 61.0):
            x = mp.mpf(x)
            want = mp.diff(lambda t: j(l, t), x, 2)
            got = (cm * j(l - 2, x) if l >= 2 else 0) - c0 * j(l, x) + cp * j(l + 2, x)
            assert abs(got - want) <= mp.mpf(10) ** -13 * max(abs(want), abs(j(l, x))), (l, x)
    cm, c0, cp = nlm.jpp_coefficients(np.arange(2))
    assert np.all(cm == 0.0)                                    # orders below 0 never enter


# ---------------------------------------------------------------- 2. the Gaussian-window case
REFERENCE_RULE = (385, 1537)          # its own error at l = 2 is (129, 513)'s 4e-5 shrunk by (3^10 =) 6e4: below 1e-9


def test_gaussian_window_limber_ratios_and_convergence():
    ref = nlm.toy_cl(*REFERENCE_RULE)
    ratio = nlm.toy_limber() / ref
    for l, r in zip(nlm.ELLS, ratio):
        print(f"l = {l}: C_l(Limber) / C_l(exact) = {r:.4f}")
        assert abs(r - nlm.LIMBER_RATIO[l]) <= 1e-3
    coarse = np.abs(nlm.toy_cl(129, 513) / ref - 1.0)
    fine = np.abs(nlm.toy_cl(257, 1025) / ref - 1.0)
    print("relative error of the (129, 513) rule:", coarse, "\nof the (257, 1025) rule:", fine)
    assert 4.0e-5 / 4.0 <= coarse[0] <= 4.0e-5 * 4.0 and np.all(coarse[1:] < 1e-11)
    assert 4.0e-8 / 4.0 <= fine[0] <= 4.0e-8 * 4.0 and np.all(fine[1:] < 1e-11)


def test_lensing_kind_tends_to_its_limber_value():
    ells = np.array(nlm.ELLS, dtype=np.float64)
    fac = (ells * (ells + 1.0) / (ells + 0.5) ** 2) ** 2
    ratio = nlm.toy_cl(257, 1025, kind=1) / (nlm.toy_limber() * fac)
    print("lensing kind, C_l / (Limber times [l (l + 1) / (l + 1/2)^2]^2):", ratio)
    off = np.abs(ratio - 1.0)
    assert np.all(np.diff(off) < 0) and off[-1] < 0.03 and off[0] > 0.5


def test_kaiser_term_raises_the_quadrupole():
    plain, rsd = nlm.toy_cl(257, 1025), nlm.toy_cl(257, 1025, growth=0.8)
    print("C_l with the Kaiser term / without:", rsd / plain)
    assert rsd[0] > 1.5 * plain[0] and np.all(rsd > plain) and abs(rsd[-1] / plain[-1] - 1.0) < 0.05


# ---------------------------------------------------------------- 3. exports, build, ABI
def test_exports_and_build_unit():
    for name in nonlimber.__all__:
        assert getattr(hmvec_amd, name) is getattr(nonlimber, name) and name in hmvec_amd.__all__
    assert hmvec_amd.nonlimber is nonlimber and "nonlimber" in hmvec_amd.__all__
    for name in ("spherical_bessel", "nonlimber_transfer", "nonlimber_transfer_device", "nonlimber_cl", "nonlimber_cl_device",
                 "refine_gzs", "nonlimber_k_rule"):
        assert name in nonlimber.__all__
    with open(os.path.join(REPO, "hmvec_amd", "csrc", "Makefile")) as f:
        mk = f.read()
    assert re.search(r"^KUNITS = .*\bnonlimber\b", mk, flags=re.M)
    assert re.search(r"^DEPS_nonlimber\s*=\s*kernels/nonlimber\.hpp sphbessel\.hpp", mk, flags=re.M)
    assert re.search(r"^#\s+nonlimber\s", mk, flags=re.M)


def test_abi_symbols_declared_once_and_bound():
    with open(os.path.join(REPO, "include", "hmgrid.h")) as f:
        header = f.read()
    for name in ("hmg_sph_bessel", "hmg_nonlimber_transfer", "hmg_nonlimber_cl"):
        assert len(re.findall(r"^int\s+" + name + r"\s*\(", header, re.M)) == 1
        assert name in nat.SIGNATURES and nat.PARAMS[name][0] == "ctx"
    assert nat.PARAMS["hmg_sph_bessel"] == ("ctx", "lmax", "nx", "d_xs", "d_out")
    assert nat.PARAMS["hmg_nonlimber_transfer"] == ("ctx", "F", "ngz", "nkq", "lmax", "d_kq", "d_chis", "d_src", "d_out")
    assert nat.PARAMS["hmg_nonlimber_cl"] == ("ctx", "F", "nkq", "lmax", "np", "h_pairs", "d_pairs", "d_kq", "d_wk", "d_T",
                                             "d_out")
    assert nonlimber.fmax() == 16 and nat.DEFINES["HMG_NONLIMBER_THREADS"] == 256 and nat.DEFINES["HMG_NONLIMBER_TILE"] == 16
    with open(os.path.join(REPO, "hmvec_amd", "csrc", "kernels", "nonlimber.hpp")) as f:
        hpp = f.read()
    assert "atomic" not in hpp.replace("no atomics", "")


# ---------------------------------------------------------------- 4. refusals
def test_free_function_refusals():
    ctx = rc.recording_context()
    kq, chis = np.linspace(0.01, 0.1, 5), np.linspace(100.0, 110.0, 11)
    src = np.ones((2, 11, 5))
    bad = [
        lambda: nonlimber.spherical_bessel(-1, [1.0], ctx=ctx),
        lambda: nonlimber.spherical_bessel(2.0, [1.0], ctx=ctx),
        lambda: nonlimber.spherical_bessel(2, [0.0], ctx=ctx),
        lambda: nonlimber.spherical_bessel(2, [np.nan], ctx=ctx),
        lambda: nonlimber.nonlimber_transfer(kq[::-1], chis, src, 3, ctx=ctx),
        lambda: nonlimber.nonlimber_transfer(kq, -chis, src, 3, ctx=ctx),
        lambda: nonlimber.nonlimber_transfer(kq, chis, src[:, :-1], 3, ctx=ctx),
        lambda: nonlimber.nonlimber_transfer(kq, chis, src * np.inf, 3, ctx=ctx),
        lambda: nonlimber.nonlimber_transfer(kq, chis, src, True, ctx=ctx),
        lambda: nonlimber.nonlimber_cl(kq, np.ones(4), np.ones((2, 4, 5)), [(0, 1)], ctx=ctx),
        lambda: nonlimber.nonlimber_cl(kq, np.ones(5), np.ones((2, 4, 5)), [(0, 2)], ctx=ctx),
        lambda: nonlimber.nonlimber_cl(kq, np.ones(5), np.ones((2, 4, 5)), [], ctx=ctx),
        lambda: nonlimber.nonlimber_cl(kq, np.ones(5), np.ones((2, 4, 6)), [(0, 1)], ctx=ctx),
        lambda: nonlimber.nonlimber_k_rule(10, 100.0, 50.0, 5.0),
        lambda: nonlimber.nonlimber_k_rule(10, 100.0, 150.0, 0.0),
    ]
    for call in bad:
        with pytest.raises(ValueError):
            call()
    with pytest.raises(ValueError, match="refine_gzs"):            # below Nyquist: kq[-1] dchi = 40 > pi
        nonlimber.nonlimber_transfer(kq, np.linspace(100.0, 4100.0, 11), src, 3, ctx=ctx)
    assert ctx.lib.calls == []                                     # nothing reached the library
    # the shape of a valid request: one launch per 16 fields
    nonlimber.nonlimber_transfer_device(kq, chis, np.ones((17, 11, 5)), 3, ctx=ctx)
    launches = [a for n, a in ctx.lib.calls if n == "hmg_nonlimber_transfer"]
    assert [a[1] for a in launches] == [16, 1] and launches[1][7] - launches[0][7] == 16 * 11 * 5 * 8
    assert launches[1][8] - launches[0][8] == 16 * 4 * 5 * 8


def test_k_rule_and_refine_gzs():
    kq, wk = nonlimber.nonlimber_k_rule(200, 1140.0, 1860.0, 60.0)
    assert kq[0] == 1e-4 and np.isclose(kq[-1], np.hypot(200.5 / 1140.0, 8.0 / 60.0)) and np.isclose(wk.sum(), kq[-1] - kq[0])
    assert np.pi / (1860.0 * 8) >= kq[1] - kq[0] > 0.9 * np.pi / (1860.0 * 8)
    kq2, _ = nonlimber.nonlimber_k_rule(200, 1140.0, 1860.0, 60.0, kmax=0.6, per_period=4)
    assert kq2[-1] == 0.6 and kq2.size < kq.size * 2

    class Flat:                                     # chi = 3000 z, H = 1/3000
        def comoving_radial_distance(self, z):
            return 3000.0 * np.asarray(z, dtype=np.float64)

        def h_of_z(self, z):
            return np.full(np.shape(z), 1.0 / 3000.0)
    gzs = nonlimber.refine_gzs(Flat(), 0.4, 0.6, 0.5, phase=0.5)
    chis = 3000.0 * gzs
    assert gzs[0] == 0.4 and gzs[-1] == 0.6 and np.all(np.diff(gzs) > 0)
    assert 0.5 * np.max(np.diff(chis)) <= 0.5 * (1 + 1e-12) and gzs.size == 601
    with pytest.raises(ValueError):
        nonlimber.refine_gzs(Flat(), 0.6, 0.4, 0.5)
