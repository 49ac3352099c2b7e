"""GPU checks of the covariance of angular correlation functions (hmvec_amd.angcov: bin_averaged_bessel,
real_cov_gaussian, binned_angular_from_cl, project_cl_cov, angular_cov of a HaloModel; definition and gates in DESIGN.md
section 23).  The reference computes none of this, so there is no reference fixture: the device is pinned by 40-digit
mpmath where mpmath is affordable (the weights, a one-panel correlation function), elsewhere by the numpy restatement
that tests/test_angcov_cpu.py pins against mpmath, and by bit-identities.

The gate is derived (tests/helpers/angcov_model.py): a weight's error bound delta from C2 u (|G(l b)| + |G(l a)|) and
the J0 / J1 headers' bounds, per multipole l |G| (delta_i |K_j| + delta_j |K_i| + delta_i delta_j) + C1 u |t_l|, and
gamma_|L| sum |t_l| for the sum; C1 = 16 counts roundings, C2 = 16 was fixed on the CPU from the host build of the
header against mpmath (worst ratio 0.32).  Nothing of it is taken from the device's output.

Measured on an MI355X (worst |got - ref| / gate): weights against mpmath 0.34; Gaussian covariance against the
restatement 0.026; node weights 0.44 (nodes at every integer, where R is l K: a single weight against its own bound),
0.015 otherwise; one-panel correlation function against mpmath 0.012; projection of a rank-one matrix 0.048."""
import os
import sys

import numpy as np
import pytest

from hmvec_amd import _native as nat
from hmvec_amd import angcov

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import angcov_model as acm  # noqa: E402
from lensing_model import model  # noqa: E402

pytestmark = pytest.mark.gpu

CHUNK, TILE = nat.DEFINES["HMG_ANGCOV_CHUNK"], nat.DEFINES["HMG_ANGCOV_TILE"]
FSKY = 0.25


def within_gate(got, ref, gate, what):
    err = np.abs(got - ref)
    worst = float(np.max(err / np.maximum(gate, 1e-300)))
    print(f"{what}: worst |got - ref| / gate = {worst:.3g}")
    return bool(np.all(err <= gate)), worst


def edges_of(nt):
    return np.geomspace(2e-3, 0.3, nt + 1)


# ---------------------------------------------------------------- 1. the weights against mpmath
@pytest.mark.parametrize("nt", [1, 5])
def test_weights_against_mpmath(nt):
    edges, ref = acm.POINT_EDGES[nt], acm.point_reference(nt)
    got = angcov.bin_averaged_bessel(acm.POINT_ELLS, edges, acm.ORDERS)
    assert len(got) == 3
    for order, K in zip(acm.ORDERS, got):
        assert K.shape == (acm.POINT_ELLS.size, nt)
        ok, worst = within_gate(K, ref[order], acm.weights_gate(acm.POINT_ELLS, edges, order), f"K_{order}, nt = {nt}")
        assert ok, (order, worst)
        assert np.array_equal(angcov.bin_averaged_bessel(acm.POINT_ELLS, edges, order), K)        # alone: the same bits
    # a bin's weight depends on its own two edges alone
    if nt == 5:
        sub = angcov.bin_averaged_bessel(acm.POINT_ELLS[2:4], edges[1:4], 4)
        assert np.array_equal(sub, got[2][2:4, 1:3])


# ---------------------------------------------------------------- 2. the Gaussian covariance against the restatement
# L = 2 .. 2 CHUNK + 1 is two full chunks, L = 1 .. 2 CHUNK + 1 two chunks and one multipole more, L = 2 .. 300 lies
# inside one chunk.  The fields, the probes and what they cover: angcov_model.three_fields and PROBES.
LRANGES = {"two_chunks": (2, 2 * CHUNK + 1), "two_chunks_and_one": (1, 2 * CHUNK + 1), "one_chunk": (2, 300)}


def nodes_of(lrange, every_integer):
    lo, hi = LRANGES[lrange]
    return np.arange(lo, hi + 1, dtype=np.float64) if every_integer else np.geomspace(lo, hi, 17)


@pytest.mark.parametrize("nt", [1, 5, TILE + 1])
@pytest.mark.parametrize("every_integer", [True, False], ids=["every_integer", "17_nodes"])
@pytest.mark.parametrize("lrange", list(LRANGES))
def test_gaussian_against_the_numpy_restatement(lrange, every_integer, nt):
    nodes = nodes_of(lrange, every_integer)
    L = acm.multipoles(nodes)
    assert (L[0], L[-1]) == LRANGES[lrange] and (nodes.size == 17 or nodes.size == L.size)
    C, N = acm.three_fields(nodes)
    assert np.all(C[0, 1] < 0) and np.all(C[0, 2] == 0) and N[1] == 0
    assert {(min(p[2], q[2]), max(p[2], q[2])) for p in acm.PROBES for q in acm.PROBES} == \
        {(0, 0), (0, 2), (0, 4), (2, 2), (2, 4), (4, 4)}
    edges = edges_of(nt)
    got = angcov.real_cov_gaussian(nodes, C, N, edges, acm.PROBES, FSKY)
    ref, gate = acm.cov_numpy(nodes, C, N, edges, acm.PROBES, FSKY, with_gate=True)
    assert got.shape == (len(acm.PROBES), nt, len(acm.PROBES), nt) and np.all(np.isfinite(got))
    ok, worst = within_gate(got, ref, gate, f"cov, L {lrange}, nn {nodes.size}, nt {nt}")
    assert ok, worst
    # the block of (0, 1, 2) x (2, 1, 4) lives on its ad.bc term alone and is not zero
    assert np.all(got[1, :, 4, :] != 0)


# ---------------------------------------------------------------- 3. noise only
@pytest.mark.parametrize("nt", [1, 5])
def test_noise_only_is_the_closed_form_exactly(nt):
    nodes = nodes_of("one_chunk", False)
    N = np.array([2e-9, 0.0, 4e-10])
    edges = edges_of(nt)
    got = angcov.real_cov_gaussian(nodes, np.zeros((3, 3, nodes.size)), N, edges, acm.PROBES, FSKY)
    want = acm.noise_matrix(N, edges, acm.PROBES, FSKY)
    assert np.array_equal(got, want)
    # on the diagonal of blocks with equal orders and matching fields alone; (0, 0, 0) twice N^2, (1, 1, .) zero noise
    assert np.all(got[0, range(nt), 0, range(nt)] > 0) and np.all(got[2] == 0) and np.all(got[3] == 0)
    assert np.all(got[5, range(nt), 5, range(nt)] > 0) and np.count_nonzero(got) == 2 * nt


# ---------------------------------------------------------------- 4. identities, bit for bit
@pytest.fixture(scope="module")
def full():
    nodes = nodes_of("two_chunks", False)
    C, N = acm.three_fields(nodes)
    edges = edges_of(5)
    return nodes, C, N, edges, angcov.real_cov_gaussian(nodes, C, N, edges, acm.PROBES, FSKY)


def test_symmetry_and_repeat(full):
    nodes, C, N, edges, cov = full
    assert np.array_equal(cov, cov.transpose(2, 3, 0, 1))
    assert np.array_equal(angcov.real_cov_gaussian(nodes, C, N, edges, acm.PROBES, FSKY), cov)


def test_a_subset_returns_the_bits_of_the_full_call(full):
    nodes, C, N, edges, cov = full
    pick = [4, 1, 3]                                            # a subset of the probes, in another order
    sub = angcov.real_cov_gaussian(nodes, C, N, edges, [acm.PROBES[p] for p in pick], FSKY)
    assert np.array_equal(sub, cov[np.ix_(pick, range(5), pick, range(5))])
    one = angcov.real_cov_gaussian(nodes, C, N, edges, [acm.PROBES[3]], FSKY)
    assert np.array_equal(one[0, :, 0, :], cov[3, :, 3, :])
    bins = angcov.real_cov_gaussian(nodes, C, N, edges[1:4], acm.PROBES, FSKY)        # bins 1 and 2
    assert np.array_equal(bins, cov[:, 1:3][:, :, :, 1:3])


def test_swapping_the_fields_of_a_probe_changes_nothing(full):
    nodes, C, N, edges, cov = full
    swapped = [(g, f, mu) for f, g, mu in acm.PROBES]
    assert np.array_equal(angcov.real_cov_gaussian(nodes, C, N, edges, swapped, FSKY), cov)
    # (0, 1, 0) written as (1, 0, 0) is the same probe
    both = angcov.real_cov_gaussian(nodes, C, N, edges, [(0, 1, 0), (1, 0, 0)], FSKY)
    assert np.array_equal(both[0, :, 0, :], both[1, :, 1, :]) and np.array_equal(both[0, :, 0, :], both[0, :, 1, :])
    assert np.array_equal(both[0, :, 0, :], cov[6, :, 6, :])


# ---------------------------------------------------------------- 5. positive semi-definite
def test_a_full_data_vector_is_positive_semi_definite():
    """w(theta) of a lens sample, gamma_t about two source bins, xi+ and xi- of the source bins: 9 probes x 5 bins."""
    nodes = nodes_of("two_chunks", False)
    C, _ = acm.three_fields(nodes)
    N = np.array([2e-9, 1e-9, 4e-10])
    probes = [(0, 0, 0), (0, 1, 2), (0, 2, 2), (1, 1, 0), (1, 2, 0), (2, 2, 0), (1, 1, 4), (1, 2, 4), (2, 2, 4)]
    edges = edges_of(5)
    cov = angcov.real_cov_gaussian(nodes, C, N, edges, probes, FSKY).reshape(45, 45)
    _, gate = acm.cov_numpy(nodes, C, N, edges, probes, FSKY, with_gate=True)
    assert np.array_equal(cov, cov.T)
    low = float(np.linalg.eigvalsh(cov)[0])
    bound = float(np.max(np.sum(gate.reshape(45, 45), axis=1)))
    print(f"smallest eigenvalue {low:.3g}, largest {np.linalg.eigvalsh(cov)[-1]:.3g}, -(row sum of the gate) {-bound:.3g}")
    assert low >= -bound


# ---------------------------------------------------------------- 6. node weights, binned xi, projection
@pytest.mark.parametrize("every_integer", [True, False], ids=["every_integer", "17_nodes"])
@pytest.mark.parametrize("lrange", ["two_chunks_and_one", "one_chunk"])
def test_node_weights_against_the_restatement(lrange, every_integer):
    nodes = nodes_of(lrange, every_integer)
    L = acm.multipoles(nodes)
    edges = edges_of(5)
    ctx = nat.default_context(0)
    for order in acm.ORDERS:
        ref, gate = acm.node_weights_numpy(nodes, edges, order, with_gate=True)
        got = angcov.node_weights_device(ctx, nodes, int(L[0]), L.size, edges, order).numpy()
        ok, worst = within_gate(got, ref, gate, f"R_{order}, L {lrange}, nn {nodes.size}")
        assert ok, worst
        by_node = angcov.node_weights_device(ctx, nodes, int(L[0]), L.size, edges, order, by_node=True).numpy()
        assert np.array_equal(by_node.T, got)
        if every_integer:          # a node's hat is 1 at its own multipole and 0 elsewhere: R is l K
            K = angcov.bin_averaged_bessel(L, edges, order)
            assert np.array_equal(got, (L[:, None] * K).T)


@pytest.mark.parametrize("order", acm.ORDERS)
def test_binned_correlation_function_of_one_panel_against_mpmath(order):
    nodes, Cn = np.array([2.0, 60.0]), np.array([3e-7, -1e-7])
    edges = np.array([0.004, 0.02, 0.021, 0.4])
    got = angcov.binned_angular_from_cl(nodes, Cn, edges, order)
    assert got.shape == (3,)
    ok, worst = within_gate(got, acm.binned_mpmath(nodes, Cn, edges, order), acm.binned_gate(nodes, Cn, edges, order),
                            f"xi_{order} of one panel")
    assert ok, worst
    stack = angcov.binned_angular_from_cl(nodes, np.stack([Cn, 2.0 * Cn, np.zeros(2)]), edges, order)
    assert np.array_equal(stack[0], got) and np.array_equal(stack[1], 2.0 * got) and np.all(stack[2] == 0)


def test_projection_of_a_rank_one_matrix_is_the_outer_product():
    nodes = nodes_of("two_chunks_and_one", False)
    C, _ = acm.three_fields(nodes)
    u, v = C[0, 1], C[1, 1]                                      # one of them negative
    edges = edges_of(5)
    for o1, o2 in ((0, 0), (0, 4), (2, 4)):
        got = angcov.project_cl_cov(np.outer(u, v), nodes, edges, o1, o2)
        a, b = angcov.binned_angular_from_cl(nodes, u, edges, o1), angcov.binned_angular_from_cl(nodes, v, edges, o2)
        # both sides hold the same node weights; they differ by the rounding of sums of nn (and nn^2) products, bounded
        # with the restatement's |R| (nothing of the bound is the device's)
        A = np.abs(acm.node_weights_numpy(nodes, edges, o1)) @ np.abs(u) / (2 * np.pi)
        B = np.abs(acm.node_weights_numpy(nodes, edges, o2)) @ np.abs(v) / (2 * np.pi)
        gate = 2.0 * (2 * nodes.size + 8) * acm.U * np.outer(A, B)
        ok, worst = within_gate(got, np.outer(a, b), gate, f"projection of u v^T, orders {o1}, {o2}")
        assert got.shape == (5, 5) and ok, worst
    sym = np.outer(u, u)
    P = angcov.project_cl_cov(sym, nodes, edges, 2, 2)
    assert np.allclose(P, P.T, rtol=1e-12, atol=0)


# ---------------------------------------------------------------- 7. the facade
def test_facade_equals_the_free_function_on_its_own_spectra():
    zs = np.array([0.3, 0.6, 0.9])
    hm = model(zs)
    hm.add_hod("g", mthresh=10 ** 10.5 + zs * 0.0)
    before = hm.get_power("g", "nfw")
    win_g = np.array([1.0, 2.0, 0.5])
    win_s = np.array([0.002, 0.004, 0.003])
    fields = {"lens": ("g", win_g, 3e-8), "src": ("nfw", win_s, 1e-10)}
    probes = [("lens", "lens", 0), ("lens", "src", 2), ("src", "src", 0), ("src", "src", 4)]
    ells = np.geomspace(20.0, 3000.0, 12)
    edges = edges_of(4)
    cov = angcov.angular_cov(hm, edges, probes, fields, 0.1, ells)
    labels, Ctab, noise = angcov.angular_cov_spectra_device(hm, fields, ells)
    Cl = Ctab.numpy()
    assert labels == ["lens", "src"] and Cl.shape == (2, 2, 12) and np.array_equal(noise, [3e-8, 1e-10])
    assert np.array_equal(Cl, Cl.transpose(1, 0, 2)) and np.all(Cl[0, 0] > 0) and np.all(np.isfinite(Cl))
    # the facade's C_l are limber_integral's of its spectra
    want = hm.limber_integral(ells, zs, hm.ks, before, zs, win_g, win_s, hm.h_of_z(zs), hm.comoving_radial_distance(zs))
    assert np.array_equal(Cl[0, 1], want)
    idx = [(0, 0, 0), (0, 1, 2), (1, 1, 0), (1, 1, 4)]
    free = angcov.real_cov_gaussian(ells, Cl, noise, edges, idx, 0.1)
    assert cov.shape == (4, 4, 4, 4) and np.array_equal(cov, free)
    assert np.all(cov[range(4), :, range(4), :][:, range(4), range(4)] > 0)          # variances
    # cached spectra stay valid
    assert np.array_equal(hm.get_power("g", "nfw"), before)
    with pytest.raises(ValueError):
        angcov.angular_cov(hm, edges, [("lens", "nope", 0)], fields, 0.1, ells)
    with pytest.raises(ValueError):
        angcov.angular_cov(hm, edges, probes, fields, 0.1, ells, term="3h")
    one_halo = angcov.angular_cov(hm, edges, probes, fields, 0.1, ells, term="1h")
    assert one_halo.shape == cov.shape and not np.array_equal(one_halo, cov)
