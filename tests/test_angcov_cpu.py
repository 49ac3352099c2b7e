"""Host-side checks of the covariance of angular correlation functions; no GPU.  The numpy
restatement tests/helpers/angcov_model.py - the reference of tests/test_gpu_angcov.py at sizes where mpmath is slow - is
pinned against 40-digit mpmath: its weights K_mu at l theta from 1e-6 to 1e5, on both sides of the two series switches,
for narrow and wide bins; its covariance against a literal evaluation of the definition on a tiny case; its node
weights through the bin-averaged correlation function of a one-panel spectrum.  The weight functions of
hmvec_amd/csrc/kernels/angcov.hpp are built with a host compiler (tests/cpp/angcov_host.cpp, plain and under
AddressSanitizer + UBSan) and measured against the same mpmath values: that measurement fixes the constant C2 of the
gate.  The bindings, the exports and every refusal of the Python layer are checked on their own.

Measured (worst |got - mpmath| / gate with C1 = 16, C2 = 16): restatement weights 0.32, host build of the header
0.32, restatement covariance 0.030, bin-averaged correlation function 0.018."""
import os
import subprocess
import sys

import numpy as np
import pytest

import hmvec_amd
from hmvec_amd import _native as nat
from hmvec_amd import angcov

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import angcov_model as acm  # noqa: E402


def worst(got, ref, gate, what):
    ratio = float(np.max(np.abs(got - ref) / np.maximum(gate, 1e-300)))
    print(f"{what}: worst |got - ref| / gate = {ratio:.3g}")
    return ratio


# ---------------------------------------------------------------- the weights
def test_the_points_cover_what_they_should():
    x = acm.POINT_ELLS[:, None] * acm.POINT_EDGES[5][None, :]
    assert x.min() == 1e-6 and x.max() > 1e5
    for sw in (acm.SERIES_X[2], acm.SERIES_X[4]):
        assert np.any((x < sw) & (x > sw * (1 - 2e-6))) and np.any((x > sw) & (x < sw * (1 + 2e-6)))
    ratios = acm.POINT_EDGES[5][1:] / acm.POINT_EDGES[5][:-1]
    assert np.isclose(ratios[0], 1.001) and np.isclose(ratios[1], 10.0) and np.isclose(ratios[4], 10.0)
    assert np.isclose(acm.POINT_EDGES[1][1] / acm.POINT_EDGES[1][0], 1.001)


@pytest.mark.parametrize("order", acm.ORDERS)
def test_mpmath_antiderivative_is_the_quadrature(order):
    """The reference of every weight check - G_mu from its hypergeometric form and, above 50, the closed form - against
    40-digit quadrature of 2/(b^2 - a^2) int theta J_mu(l theta) dtheta where quadrature is affordable."""
    cases = [(1.0, 1e-6, 1.001e-6), (1.0, 1.001e-6, 1.001e-5), (3.0, 1.0 - 1e-6, 1.0 + 1e-6), (5.0, 1.0 - 1e-6, 1.0 + 1e-6),
             (5.0, 1.0 + 1e-6, 10.0 * (1.0 + 1e-6)), (40.0, 0.05, 0.05 * 1.001), (40.0, 0.5, 5.0), (3.0, 1e-3, 20.0)]
    for l, a, b in cases:
        ref = acm.weights_mpmath([l], [a, b], order)[0, 0]
        quad = acm.weights_quad(l, a, b, order)
        scale = abs(ref) + 1e-300
        assert abs(quad - ref) <= 1e-13 * scale, (l, a, b, quad, ref)


@pytest.mark.parametrize("nt", [1, 5])
def test_weights_of_the_restatement(nt):
    ref = acm.point_reference(nt)
    for order in acm.ORDERS:
        got = acm.weights_numpy(acm.POINT_ELLS, acm.POINT_EDGES[nt], order)
        gate = acm.weights_gate(acm.POINT_ELLS, acm.POINT_EDGES[nt], order)
        assert np.all(np.isfinite(got)) and got.shape == ref[order].shape == (acm.POINT_ELLS.size, nt)
        assert worst(got, ref[order], gate, f"restatement K_{order}, nt = {nt}") <= 0.5


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "asan_ubsan"])
def test_weights_of_the_header(tmp_path, flags):
    """kernels/angcov.hpp's weight functions as a host compiler builds them, in a program of its own: this is the
    measurement that fixes C2 (the gate must hold with a headroom of at least 2)."""
    exe = tmp_path / "angcov_host"
    src = os.path.join(HERE, "cpp", "angcov_host.cpp")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-Werror", "-ffp-contract=off", *flags, src,
                    "-o", str(exe)], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1")
    for nt in (1, 5):
        edges = acm.POINT_EDGES[nt]
        lines = "".join(f"{float(l).hex()} {float(edges[i]).hex()} {float(edges[i + 1]).hex()}\n"
                        for l in acm.POINT_ELLS for i in range(nt))
        r = subprocess.run([str(exe)], input=lines, env=env, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        got = np.array([[float.fromhex(v) for v in line.split()] for line in r.stdout.splitlines()])
        assert got.shape == (acm.POINT_ELLS.size * nt, 3)
        ref = acm.point_reference(nt)
        for k, order in enumerate(acm.ORDERS):
            gate = acm.weights_gate(acm.POINT_ELLS, edges, order)
            assert worst(got[:, k].reshape(-1, nt), ref[order], gate, f"header K_{order}, nt = {nt}") <= 0.5


def test_series_and_closed_forms_meet():
    """Both branches of G_2 and G_4 a rounding either side of their switch, against mpmath, in units of u |G|."""
    import mpmath as mp
    for order in (2, 4):
        sw = acm.SERIES_X[order]
        for x in (np.nextafter(sw, 0.0), sw):
            with mp.workdps(40):
                ref = float(acm.g_mpmath(mp.mpf(float(x)), order))
            err = abs(float(acm.g_fn(x, order)) - ref) / (acm.U * abs(ref))
            print(f"G_{order}({x!r}): error {err:.2f} u |G|")
            assert err <= acm.C2 / 2 + 8.0 * (x >= sw)          # (the closed form also carries J0 and J1's few u)


# ---------------------------------------------------------------- the covariance
TINY_C = np.array([[[4e-7, 2.5e-7, 1e-7], [-1.5e-7, -1e-7, -3e-8]], [[-1.5e-7, -1e-7, -3e-8], [9e-8, 8e-8, 5e-8]]])
TINY_N = np.array([3e-8, 0.0])
TINY_PROBES = [(0, 0, 0), (0, 1, 2), (1, 1, 4)]
TINY_EDGES = np.array([0.01, 0.03, 0.2])


@pytest.mark.parametrize("every_integer", [False, True], ids=["three_nodes", "every_integer"])
def test_covariance_of_the_restatement_against_the_definition(every_integer):
    """L = 2 .. 40, 2 fields, 3 probes, 2 bins: the einsum with the noise products multiplied out against the definition
    taken literally (C^^ C^^ + C^^ C^^ - NN) in 40 digits."""
    nodes = np.array([2.0, 7.5, 40.0])
    C = TINY_C
    if every_integer:
        full = np.arange(2.0, 41.0)
        C = acm.interp(nodes, TINY_C, full)
        nodes = full
    assert np.array_equal(acm.multipoles(nodes), np.arange(2.0, 41.0))
    got, gate = acm.cov_numpy(nodes, C, TINY_N, TINY_EDGES, TINY_PROBES, 0.1, with_gate=True)
    ref = acm.cov_mpmath(nodes, C, TINY_N, TINY_EDGES, TINY_PROBES, 0.1)
    assert got.shape == (3, 2, 3, 2) and np.all(ref[0, 0, 0] != 0)
    assert worst(got, ref, gate, "restatement covariance") <= 0.5
    assert np.allclose(got, got.transpose(2, 3, 0, 1), rtol=1e-13, atol=0)
    # the closed-form noise term is on the diagonal of the (0, 0, 0) auto block alone
    noise = acm.noise_matrix(TINY_N, TINY_EDGES, TINY_PROBES, 0.1)
    assert np.count_nonzero(noise) == 2 and noise[0, 0, 0, 0] > 0 and noise[0, 1, 0, 1] > 0
    assert noise[0, 0, 0, 0] == 2 * TINY_N[0] ** 2 / (4 * np.pi * 0.1 * np.pi * (0.03 - 0.01) * (0.03 + 0.01))


@pytest.mark.parametrize("order", acm.ORDERS)
def test_binned_correlation_function_of_the_restatement(order):
    """R_mu C / (2 pi) of a one-panel spectrum (nodes 2 and 60) against the sum over L in 40 digits."""
    nodes, Cn = np.array([2.0, 60.0]), np.array([3e-7, -1e-7])
    edges = np.array([0.004, 0.02, 0.021, 0.4])
    got = acm.node_weights_numpy(nodes, edges, order) @ Cn / (2 * np.pi)
    ref = acm.binned_mpmath(nodes, Cn, edges, order)
    assert worst(got, ref, acm.binned_gate(nodes, Cn, edges, order), f"restatement xi_{order}") <= 0.5


def test_hats_are_a_partition_and_hit_the_nodes():
    nodes = np.array([1.5, 4.0, 9.0, 9.5, 30.0])
    L = acm.multipoles(nodes)
    assert L[0] == 2 and L[-1] == 30
    H = acm.hats(nodes, L)
    assert np.allclose(H.sum(axis=1), 1.0, rtol=0, atol=2e-16) and np.all(H >= 0)
    assert H[list(L).index(4.0), 1] == 1.0 and H[list(L).index(9.0), 2] == 1.0 and H[-1, 4] == 1.0
    C = np.array([1.0, -2.0, 0.5, 3.0, 7.0])
    assert np.array_equal(acm.interp(nodes, C, np.array([4.0, 9.0, 30.0])), [-2.0, 0.5, 7.0])


# ---------------------------------------------------------------- bindings, exports, refusals
def test_bindings_and_exports():
    for name in ("hmg_angcov_weights", "hmg_angcov_gaussian", "hmg_angcov_node_weights"):
        assert name in nat.SIGNATURES
    assert nat.PARAMS["hmg_angcov_gaussian"][-3:] == ("work_words", "d_work", "d_cov")
    assert nat.DEFINES["HMG_ANGCOV_CHUNK"] == angcov.chunk() and nat.DEFINES["HMG_ANGCOV_TILE"] >= 2
    for name in angcov.__all__:
        assert getattr(hmvec_amd, name) is getattr(angcov, name) and name in hmvec_amd.__all__


GOOD = dict(ells=np.array([2.0, 10.0, 50.0]), C=np.ones((2, 2, 3)) * 1e-7, noise=np.array([1e-9, 0.0]),
            theta_edges=np.array([0.01, 0.02, 0.05]), probes=[(0, 1, 2), (1, 1, 4)], fsky=0.3)


@pytest.mark.parametrize("change,match", [
    (dict(theta_edges=[0.01, 0.01, 0.05]), "strictly increasing"),
    (dict(theta_edges=[0.02, 0.01]), "strictly increasing"),
    (dict(theta_edges=[0.0, 0.01]), "positive"),
    (dict(ells=[2.0, 2.0, 50.0]), "strictly increasing"),
    (dict(ells=[50.0, 10.0, 2.0]), "strictly increasing"),
    (dict(ells=[0.5, 10.0, 50.0]), "at least 1"),
    (dict(noise=[1e-9, -1e-12]), "negative"),
    (dict(C=np.arange(12.0).reshape(2, 2, 3)), "symmetric"),
    (dict(probes=[(0, 1, 1)]), "order"),
    (dict(probes=[(0, 1, 6)]), "order"),
    (dict(probes=[(0, 2, 0)]), "field"),
    (dict(probes=[(-1, 0, 0)]), "field"),
    (dict(fsky=0.0), "fsky"),
    (dict(fsky=-0.2), "fsky"),
])
def test_refusals_of_the_covariance(change, match):
    with pytest.raises(ValueError, match=match):
        angcov.real_cov_gaussian(**dict(GOOD, **change))


def test_refusals_of_the_other_entry_points():
    edges, ells = GOOD["theta_edges"], GOOD["ells"]
    with pytest.raises(ValueError, match="order"):
        angcov.bin_averaged_bessel([2, 3], edges, 3)
    with pytest.raises(ValueError, match="integers"):
        angcov.bin_averaged_bessel([2.5, 3], edges, 0)
    with pytest.raises(ValueError, match="strictly increasing"):
        angcov.bin_averaged_bessel([2, 3], edges[::-1], 0)
    with pytest.raises(ValueError, match="order"):
        angcov.binned_angular_from_cl(ells, np.ones(3), edges, 1)
    with pytest.raises(ValueError, match="at least 1"):
        angcov.binned_angular_from_cl([0.0, 5.0], np.ones(2), edges, 0)
    with pytest.raises(ValueError, match="shape"):
        angcov.binned_angular_from_cl(ells, np.ones(4), edges, 0)
    with pytest.raises(ValueError, match="shape"):
        angcov.project_cl_cov(np.ones((3, 2)), ells, edges, 0, 4)
    with pytest.raises(ValueError, match="order"):
        angcov.project_cl_cov(np.ones((3, 3)), ells, edges, 0, 5)
    with pytest.raises(ValueError, match="strictly increasing"):
        angcov.project_cl_cov(np.ones((3, 3)), ells[::-1], edges, 0, 4)
