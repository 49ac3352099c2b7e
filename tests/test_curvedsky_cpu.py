"""Host-side checks of the curved-sky angular correlation functions; no GPU.  The 40-digit
references of tests/helpers/curvedsky_model.py - the textbook antiderivatives on 90-digit recurrences - are checked
against quadrature of the definitions in Jacobi form; the numpy restatement and the host build of
hmvec_amd/csrc/kernels/curvedsky.hpp (tests/cpp/curvedsky_host.cpp, plain and under AddressSanitizer + UBSan, a program
of its own) are measured against them at a = 1 arcmin with b/a = 1 + 2e-6, 1.001, 1.2 and 10, out to theta = pi, at
l theta from 2.9e-4 to 6e4, on both sides of every switch and at l = 2, 3: that measurement fixes the gate's constants
C2 and CR.  The covariance restatement is checked against the definition taken literally in 40 digits; the bindings,
the exports and every refusal of the Python layer on their own.

Measured (worst |got - mpmath| / gate with C2 = 16, CR = 1): restatement weights 0.46, host build of the header 0.37
(with C2 = 8: 0.62; with CR = 1/2: 0.74), a single G beside a switch 0.57, restatement covariance 0.35, bin-averaged
correlation function 0.018."""
import os
import subprocess
import sys

import numpy as np
import pytest

import hmvec_amd
from hmvec_amd import _native as nat
from hmvec_amd import curvedsky

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import angcov_model as acm  # noqa: E402
import curvedsky_model as csm  # noqa: E402


def worst(got, ref, gate, what):
    ratio = float(np.max(np.abs(got - ref) / np.maximum(gate, 1e-300)))
    print(f"{what}: worst |got - ref| / gate = {ratio:.3g}")
    return ratio


# ---------------------------------------------------------------- the weights
def test_the_points_cover_what_they_should():
    e = csm.POINT_EDGES["arcmin"]
    assert e[0] == csm.ARCMIN and e[-1] == np.pi
    assert np.allclose(e[1:5] / e[:4], [1 + 2e-6, 1.001, 1.2, 10.0], rtol=1e-12)
    x = csm.POINT_ELLS[:, None] * e[None, :]
    assert x.min() < 1e-3 and x.max() > 1e4
    assert {2.0, 3.0} <= set(csm.POINT_ELLS)
    for l in (3, 40, 1000):
        s, _, _ = csm.half_angle(csm.POINT_EDGES[f"switch{l}"])
        z = l * (l + 1.0) * s
        assert z[0] < 2.25 < z[1] and z[2] < 6.25 < z[3] and np.allclose(z, [2.25, 2.25, 6.25, 6.25], rtol=1e-5)


@pytest.mark.parametrize("kind", csm.KINDS)
def test_mpmath_antiderivative_is_the_quadrature(kind):
    """The reference of every weight check against 40-digit quadrature of sin(theta) d_kind^l(theta), d in Jacobi form."""
    for l, theta in [(2, 0.3), (2, 3.0), (3, 1.0), (3, 1e-2), (9, 0.5), (9, 3.1), (40, 0.2), (40, 2.0)]:
        ref = csm.g_mpmath([l], [theta], kind)[0, 0]
        quad = float(csm.g_quad(l, theta, kind))
        assert abs(quad - ref) <= 1e-13 * abs(ref), (l, theta, quad, ref)


@pytest.mark.parametrize("name", list(csm.POINT_EDGES))
def test_weights_of_the_restatement(name):
    ells, edges, ref = csm.point_ells(name), csm.POINT_EDGES[name], csm.point_reference(name)
    for kind in csm.KINDS:
        got = csm.weights_numpy(ells, edges, kind)
        assert np.all(np.isfinite(got)) and got.shape == ref[kind].shape == (ells.size, edges.size - 1)
        assert worst(got, ref[kind], csm.weights_gate(ells, edges, kind), f"restatement K_{kind}, {name}") <= 0.5


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "asan_ubsan"])
def test_weights_of_the_header(tmp_path, flags):
    """kernels/curvedsky.hpp's recurrence, series and closed forms as a host compiler builds them, in a program of its
    own: this is the measurement that fixes C2 and CR (the gate must hold with a headroom of at least 2)."""
    exe = tmp_path / "curvedsky_host"
    src = os.path.join(HERE, "cpp", "curvedsky_host.cpp")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-Werror", "-ffp-contract=off", *flags, src,
                    "-o", str(exe)], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1")
    for name, edges in csm.POINT_EDGES.items():
        ells, nt = csm.point_ells(name), edges.size - 1
        lines = "".join(f"{float(l).hex()} {float(edges[i]).hex()} {float(edges[i + 1]).hex()}\n"
                        for l in ells for i in range(nt))
        r = subprocess.run([str(exe)], input=lines, env=env, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        got = np.array([[float.fromhex(v) for v in line.split()] for line in r.stdout.splitlines()])
        assert got.shape == (ells.size * nt, 4)
        ref = csm.point_reference(name)
        for k, kind in enumerate(csm.KINDS):
            gate = csm.weights_gate(ells, edges, kind)
            assert worst(got[:, k].reshape(-1, nt), ref[kind], gate, f"header K_{kind}, {name}") <= 0.5


@pytest.mark.parametrize("l", [3, 40, 1000])
def test_series_and_closed_forms_meet(l):
    """G of the three spin-2 kinds a part in 1e6 either side of its switch, against mpmath, inside the gate dG of a
    single G (the factor 2 of headroom is asked of the weights at the sample points, where the constants were fixed);
    the two sides differ by what G itself changes over the step."""
    theta = csm.POINT_EDGES[f"switch{l}"]
    for kind in ("gammat", "xip", "xim"):
        pair = theta[2:] if kind == "xim" else theta[:2]
        s, _, _ = csm.half_angle(pair)
        z = l * (l + 1.0) * s
        assert z[0] < csm.SWITCH[kind] < z[1]
        got, ref = csm.g_numpy([l], pair, kind)[0], csm.g_mpmath([l], pair, kind)[0]
        gate = csm.dG([l], pair, kind)[0]
        print(f"G_{kind}(l = {l}) below / above its switch: error {np.abs(got - ref) / gate} of the gate")
        assert np.all(np.abs(got - ref) <= gate)
        assert abs((got[1] - got[0]) - (ref[1] - ref[0])) <= gate.sum()


def test_l2_weights_are_the_elementary_integrals():
    """d^2_{22} = ((1 + x)/2)^2, d^2_{2,-2} = ((1 - x)/2)^2, d^2_{02} = sqrt(6)/4 (1 - x^2)."""
    import mpmath as mp
    edges = np.array([csm.ARCMIN, 0.01, 0.5, 2.0, np.pi])
    with mp.workdps(40):
        x = [mp.cos(mp.mpf(float(v))) for v in edges]
        prim = {"xip": lambda v: (1 + v) ** 3 / 12, "xim": lambda v: -(1 - v) ** 3 / 12,
                "gammat": lambda v: mp.sqrt(6) / 4 * (v - v ** 3 / 3)}
        for kind, F in prim.items():
            want = np.array([float((F(x[i]) - F(x[i + 1])) / (x[i] - x[i + 1])) for i in range(4)])
            ref = csm.weights_mpmath([2.0], edges, kind)[0]
            assert np.allclose(ref, want, rtol=1e-15, atol=0)
            got, gate = csm.weights_numpy([2.0], edges, kind)[0], csm.weights_gate([2.0], edges, kind)[0]
            assert worst(got, want, gate, f"K_{kind}(l = 2) against its elementary integral") <= 0.5


@pytest.mark.parametrize("kind", csm.KINDS)
def test_bins_add_up_to_the_wide_bin(kind):
    """sum_i (cos a_i - cos b_i) K(l; i) = (cos a_0 - cos b_last) K(l; the wide bin) within the gates of both sides."""
    ells = np.array([2.0, 3.0, 17.0, 400.0, 3000.0])
    edges = np.geomspace(csm.ARCMIN, 2.0, 9)
    wide = edges[[0, -1]]
    cd = csm.cosdiff(edges[:-1], edges[1:])
    lhs = csm.weights_numpy(ells, edges, kind) @ cd
    rhs = csm.weights_numpy(ells, wide, kind)[:, 0] * csm.cosdiff(wide[0], wide[1])
    gate = csm.weights_gate(ells, edges, kind) @ cd + csm.weights_gate(ells, wide, kind)[:, 0] * csm.cosdiff(wide[0], wide[1])
    scale = np.abs(csm.weights_numpy(ells, edges, kind)) @ cd
    assert worst(lhs, rhs, gate + 12 * csm.U * scale, f"sum of the bins of K_{kind}") <= 1.0


# ---------------------------------------------------------------- the covariance
TINY_C = np.array([[[4e-7, 2.5e-7, 1e-7], [-1.5e-7, -1e-7, -3e-8]], [[-1.5e-7, -1e-7, -3e-8], [9e-8, 8e-8, 5e-8]]])
TINY_N = np.array([3e-8, 2e-9])
TINY_PROBES = [(0, 0, "w"), (0, 1, "gammat"), (1, 1, "xip"), (1, 1, "xim")]
TINY_EDGES = np.array([0.01, 0.03, 0.2])


@pytest.mark.parametrize("every_integer", [False, True], ids=["three_nodes", "every_integer"])
def test_covariance_of_the_restatement_against_the_definition(every_integer):
    """L = 2 .. 40, 2 fields, 4 probes, 2 bins: the einsum with the measure l + 1/2 and the noise products multiplied
    out against 1/(4 pi A) sum (2l + 1) K K (C^^ C^^ + C^^ C^^ - NN) taken literally in 40 digits."""
    nodes = np.array([2.0, 7.5, 40.0])
    C = TINY_C
    if every_integer:
        full = np.arange(2.0, 41.0)
        C = acm.interp(nodes, TINY_C, full)
        nodes = full
    assert np.array_equal(acm.multipoles(nodes), np.arange(2.0, 41.0))
    got, gate = csm.cov_numpy(nodes, C, TINY_N, TINY_EDGES, TINY_PROBES, 0.1, with_gate=True)
    ref = csm.cov_mpmath(nodes, C, TINY_N, TINY_EDGES, TINY_PROBES, 0.1)
    assert got.shape == (4, 2, 4, 2) and np.all(ref[0, 0, 0] != 0)
    assert worst(got, ref, gate, "restatement covariance") <= 0.5
    assert np.allclose(got, got.transpose(2, 3, 0, 1), rtol=1e-13, atol=0)
    # the closed-form noise term: on the diagonal of every auto block here, none between xip and xim
    noise = csm.noise_matrix(TINY_N, TINY_EDGES, TINY_PROBES, 0.1)
    assert np.count_nonzero(noise) == 8 and np.all(noise[2, :, 3, :] == 0)
    cd = np.cos(0.01) - np.cos(0.03)
    assert np.isclose(noise[0, 0, 0, 0], 2 * TINY_N[0] ** 2 / (4 * np.pi * 0.1 * 2 * np.pi * cd), rtol=1e-12)
    assert np.isclose(noise[1, 0, 1, 0], TINY_N[0] * TINY_N[1] / (4 * np.pi * 0.1 * 2 * np.pi * cd), rtol=1e-12)


@pytest.mark.parametrize("kind", csm.KINDS)
def test_binned_correlation_function_of_the_restatement(kind):
    """R_kind C / (2 pi) of a one-panel spectrum (nodes 2 and 60) against sum (2l + 1)/(4 pi) K C in 40 digits."""
    nodes, Cn = np.array([2.0, 60.0]), np.array([3e-7, -1e-7])
    edges = np.array([0.004, 0.02, 0.021, 0.4])
    got = csm.node_weights_numpy(nodes, edges, kind) @ Cn / (2 * np.pi)
    ref = csm.binned_mpmath(nodes, Cn, edges, kind)
    assert worst(got, ref, csm.binned_gate(nodes, Cn, edges, kind), f"restatement xi_{kind}") <= 0.5


def test_hats_and_nodes():
    """The hats are section 23's; with every integer a node R is (l + 1/2) K, and a spin-2 row of l = 1 is zero."""
    nodes = np.array([1.5, 4.0, 9.0, 9.5, 30.0])
    L = acm.multipoles(nodes)
    H = acm.hats(nodes, L)
    assert L[0] == 2 and L[-1] == 30 and np.allclose(H.sum(axis=1), 1.0, rtol=0, atol=2e-16) and np.all(H >= 0)
    full = np.arange(1.0, 31.0)
    edges = np.array([0.01, 0.1, 1.0])
    for kind in csm.KINDS:
        R = csm.node_weights_numpy(full, edges, kind)
        K = csm.weights_numpy(full, edges, kind)
        assert np.array_equal(R, ((full + 0.5)[:, None] * K).T)
        assert kind == "w" or np.all(K[0] == 0.0)
    # the flat-sky limit: K_w of a narrow bin at small angle is J0((l + 1/2) theta) to O(theta^2)
    from scipy.special import j0
    K = csm.weights_numpy([50.0, 200.0], np.array([0.01, 0.01 * (1 + 1e-4)]), "w")[:, 0]
    assert np.allclose(K, j0(np.array([50.5, 200.5]) * 0.01), rtol=0, atol=3e-4)


def test_shear_factor():
    l = np.array([1.0, 2.0, 10.0, 1e4])
    f = curvedsky.shear_factor(l)
    assert f[0] == 0.0 and f[1] == np.sqrt(4.0 / 6.0) and np.array_equal(f, csm.shear_factor(l)) and 1 - f[3] < 1.1e-8
    with pytest.raises(ValueError, match="at least 1"):
        curvedsky.shear_factor([0.5, 2.0])


# ---------------------------------------------------------------- bindings, exports, refusals
def test_bindings_and_exports():
    for name in ("hmg_curvedsky_weights", "hmg_curvedsky_gaussian", "hmg_curvedsky_node_weights",
                 "hmg_curvedsky_scale_spectra"):
        assert name in nat.SIGNATURES
    assert nat.PARAMS["hmg_curvedsky_gaussian"][-3:] == ("work_words", "d_work", "d_cov") and curvedsky.lmax() == 2 ** 24
    assert nat.PARAMS["hmg_curvedsky_weights"][-4:] == ("d_kw", "d_kg", "d_kp", "d_km")
    assert nat.PARAMS["hmg_curvedsky_scale_spectra"][-3:] == ("h_spins", "d_spins", "d_C")
    for name in curvedsky.__all__:
        assert getattr(hmvec_amd, name) is getattr(curvedsky, name) and name in hmvec_amd.__all__
    assert hmvec_amd.curvedsky is curvedsky and "curvedsky" in hmvec_amd.__all__
    assert curvedsky.KINDS == csm.KINDS and curvedsky.KIND_SPINS == csm.SPIN2
    e = np.array([0.01, 0.02, 3.0, np.pi])
    assert np.array_equal(curvedsky.cos_differences(e), csm.cosdiff(e[:-1], e[1:]))
    assert np.allclose(curvedsky.cos_differences(e), np.cos(e[:-1]) - np.cos(e[1:]), rtol=1e-12)


GOOD = dict(ells=np.array([2.0, 10.0, 50.0]), C=np.ones((2, 2, 3)) * 1e-7, noise=np.array([1e-9, 0.0]),
            theta_edges=np.array([0.01, 0.02, 0.05]), probes=[(0, 1, "gammat"), (1, 1, "xim")], fsky=0.3)


@pytest.mark.parametrize("change,match", [
    (dict(theta_edges=[0.01, 0.01, 0.05]), "strictly increasing"),
    (dict(theta_edges=[0.02, 0.01]), "strictly increasing"),
    (dict(theta_edges=[0.0, 0.01]), "positive"),
    (dict(theta_edges=[0.01, 3.2]), "pi"),
    (dict(ells=[2.0, 2.0, 50.0]), "strictly increasing"),
    (dict(ells=[0.5, 10.0, 50.0]), "at least 1"),
    (dict(noise=[1e-9, -1e-12]), "negative"),
    (dict(C=np.arange(12.0).reshape(2, 2, 3)), "symmetric"),
    (dict(probes=[(0, 1, "xi")]), "kind"),
    (dict(probes=[(0, 1, 2)]), "kind"),
    (dict(probes=[(0, 2, "w")]), "field"),
    (dict(probes=[(-1, 0, "w")]), "field"),
    (dict(probes=[]), "at least one"),
    (dict(fsky=0.0), "fsky"),
    (dict(spins=[0, 2], probes=[(0, 1, "xip")]), "spin"),
    (dict(spins=[0, 2], probes=[(1, 1, "w")]), "spin"),
    (dict(spins=[0, 2], probes=[(0, 0, "gammat")]), "spin"),
    (dict(spins=[0, 1]), "spins"),
    (dict(spins=[0, 2, 2]), "spins"),
])
def test_refusals_of_the_covariance(change, match):
    with pytest.raises(ValueError, match=match):
        curvedsky.curved_cov_gaussian(**dict(GOOD, **change))


def test_spins_accept_a_probe_spelled_either_way():
    pr = curvedsky.check_probes([(0, 1, "gammat"), (1, 0, "gammat"), (1, 1, "xip")], 2, spins=[0, 2])
    assert pr.tolist() == [[0, 1, 1], [1, 0, 1], [1, 1, 2]]


def test_refusals_of_the_other_entry_points():
    edges, ells = GOOD["theta_edges"], GOOD["ells"]
    with pytest.raises(ValueError, match="kind"):
        curvedsky.bin_averaged_wigner([2, 3], edges, "gamma")
    with pytest.raises(ValueError, match="kind"):
        curvedsky.bin_averaged_wigner([2, 3], edges, [])
    with pytest.raises(ValueError, match="integers"):
        curvedsky.bin_averaged_wigner([2.5, 3], edges, "w")
    with pytest.raises(ValueError, match="integers"):
        curvedsky.bin_averaged_wigner([0, 3], edges, "w")
    with pytest.raises(ValueError, match="pi"):
        curvedsky.bin_averaged_wigner([2, 3], [0.1, 4.0], "w")
    with pytest.raises(ValueError, match="largest multipole"):
        curvedsky.bin_averaged_wigner([2, curvedsky.lmax() + 1], edges, "w")
    with pytest.raises(ValueError, match="largest multipole"):
        curvedsky.curved_binned_from_cl([2.0, curvedsky.lmax() + 1.5], np.ones(2), edges, "w")
    with pytest.raises(ValueError, match="strictly increasing"):
        curvedsky.bin_averaged_wigner([2, 3], edges[::-1], "w")
    with pytest.raises(ValueError, match="kind"):
        curvedsky.curved_binned_from_cl(ells, np.ones(3), edges, 0)
    with pytest.raises(ValueError, match="at least 1"):
        curvedsky.curved_binned_from_cl([0.0, 5.0], np.ones(2), edges, "w")
    with pytest.raises(ValueError, match="shape"):
        curvedsky.curved_binned_from_cl(ells, np.ones(4), edges, "w")
    with pytest.raises(ValueError, match="pi"):
        curvedsky.curved_binned_from_cl(ells, np.ones(3), [0.1, 3.5], "w")
    with pytest.raises(ValueError, match="shape"):
        curvedsky.curved_project_cl_cov(np.ones((3, 2)), ells, edges, "w", "xim")
    with pytest.raises(ValueError, match="kind"):
        curvedsky.curved_project_cl_cov(np.ones((3, 3)), ells, edges, "w", 4)
    with pytest.raises(ValueError, match="strictly increasing"):
        curvedsky.curved_project_cl_cov(np.ones((3, 3)), ells[::-1], edges, "w", "xim")
    with pytest.raises(ValueError, match="spin"):
        curvedsky._split_fields({"a": ("g", np.ones(3), 0.0, 1)})
    with pytest.raises(ValueError, match="spin"):
        curvedsky._split_fields({"a": ("g", np.ones(3), 0.0)})
