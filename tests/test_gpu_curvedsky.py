"""GPU checks of the curved-sky angular correlation functions and their covariance (hmvec_amd.curvedsky:
bin_averaged_wigner, curved_cov_gaussian, curved_binned_from_cl, curved_project_cl_cov and the model-level functions;
definition and gates in DESIGN.md section 27).  The reference computes none of this: the device is pinned by 40-digit
mpmath where mpmath is affordable (the weights at chosen multipoles of every range, a one-panel correlation function),
elsewhere by the numpy restatement that tests/test_curvedsky_cpu.py pins against mpmath, and by bit-identities.

The gate is derived (tests/helpers/curvedsky_model.py): dG = C2 u |G| + (closed form's coefficients) x (CR u (l + 1) x
envelopes of P, D, P'), a weight's bound [dG(b) + dG(a)] / (cos a - cos b), the covariance's section 23's per-term bound
with l -> l + 1/2; C1 = 16 counts roundings, C2 = 16 and CR = 1 were fixed on the CPU from the host build of the header
against mpmath.  Nothing of it is taken from the device's output.

Measured on an MI355X (worst |got - ref| / gate): weights against mpmath 0.48; Gaussian covariance against the
restatement 0.026; node weights 0.055 (nodes at every integer), 0.013 otherwise; one-panel correlation function against
mpmath 0.018; projection of a rank-one matrix 0.019."""
import functools
import os
import sys

import numpy as np
import pytest

from hmvec_amd import _native as nat
from hmvec_amd import angcov, curvedsky

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import angcov_model as acm  # noqa: E402
import curvedsky_model as csm  # noqa: E402
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
    return np.geomspace(2e-3, 1.0, nt + 1)


# ---------------------------------------------------------------- 1. the weights against mpmath
# L = 1 .. 2049 is computed whole; mpmath walks its recurrences once per edge and the closed forms are compared at
# the first multipoles, around the kernel's 16-multipole stages and 256-multipole segments, and at the end.
ROWS = np.array([1, 2, 3, 4, 5, 9, 16, 17, 18, 100, 255, 256, 257, 258, 700, 1024, 1025, 1026, 2047, 2048, 2049])


@functools.lru_cache(maxsize=None)
def range_reference(nt):
    return {k: csm.weights_mpmath(ROWS.astype(float), edges_of(nt), k) for k in csm.KINDS}


@pytest.mark.parametrize("nt", [1, 5, TILE + 1])
def test_weights_against_mpmath(nt):
    L, edges = np.arange(1.0, 2050.0), edges_of(nt)
    got = curvedsky.bin_averaged_wigner(L, edges, csm.KINDS)
    ref = range_reference(nt)
    assert len(got) == 4
    for kind, K in zip(csm.KINDS, got):
        assert K.shape == (L.size, nt) and np.all(np.isfinite(K))
        ok, worst = within_gate(K[ROWS - 1], ref[kind], csm.weights_gate(ROWS.astype(float), edges, kind), f"K_{kind}, nt = {nt}")
        assert ok, (kind, worst)
        assert np.array_equal(curvedsky.bin_averaged_wigner(L, edges, kind), K)              # alone: the same bits
        if kind != "w":
            assert np.all(K[0] == 0.0)                                                       # spin 2 at l = 1
    if nt == 5:          # a value depends on its l and its two edges alone: other rows, other bins, another first multipole
        sub = curvedsky.bin_averaged_wigner([300, 301, 9, 2049], edges[1:4], "xim")
        assert np.array_equal(sub, got[3][[299, 300, 8, 2048], 1:3])


def test_weights_to_l_20000_against_mpmath():
    """6 edges from 1 arcmin to 1 radian, every multipole to 20000 on the device; compared at 40 of them."""
    edges = np.geomspace(csm.ARCMIN, 1.0, 6)
    rows = np.unique(np.concatenate([[1, 2, 3, 10], np.geomspace(30, 20000, 34).astype(int), [19999, 20000]]))
    got = curvedsky.bin_averaged_wigner(np.arange(1.0, 20001.0), edges, csm.KINDS)
    for kind, K in zip(csm.KINDS, got):
        ref = csm.weights_mpmath(rows.astype(float), edges, kind)
        ok, worst = within_gate(K[rows - 1], ref, csm.weights_gate(rows.astype(float), edges, kind), f"K_{kind} to l = 20000")
        assert ok, (kind, worst)


@pytest.mark.parametrize("name", list(csm.POINT_EDGES))
def test_weights_at_the_points_of_the_cpu_checks(name):
    """1 arcmin with b/a = 1 + 2e-6 .. 10, out to pi, l theta from 2.9e-4 to 6e4, both sides of every switch."""
    ells, edges, ref = csm.point_ells(name), csm.POINT_EDGES[name], csm.point_reference(name)
    got = curvedsky.bin_averaged_wigner(ells, edges, csm.KINDS)
    for kind, K in zip(csm.KINDS, got):
        ok, worst = within_gate(K, ref[kind], csm.weights_gate(ells, edges, kind), f"K_{kind}, points {name}")
        assert ok, (kind, worst)


# ---------------------------------------------------------------- 2. the Gaussian covariance against the restatement
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
    pairs = {tuple(sorted((p[2], q[2]))) for p in csm.PROBES for q in csm.PROBES}
    assert len(pairs) == 10                                          # all ten kind pairs the spins (0, 2, 2) allow
    edges = edges_of(nt)
    got = curvedsky.curved_cov_gaussian(nodes, C, N, edges, csm.PROBES, FSKY, spins=csm.SPINS)
    ref, gate = csm.cov_numpy(nodes, C, N, edges, csm.PROBES, FSKY, with_gate=True)
    assert got.shape == (len(csm.PROBES), nt, len(csm.PROBES), nt) and np.all(np.isfinite(got))
    ok, worst = within_gate(got, ref, gate, f"cov, L {lrange}, nn {nodes.size}, nt {nt}")
    assert ok, worst
    # the block of (0, 1, gammat) x (2, 1, xip) lives on its ad.bc term alone (C_02 = 0) and is not zero
    assert np.all(got[1, :, 5, :] != 0)


# ---------------------------------------------------------------- 3. noise only
@pytest.mark.parametrize("nt", [1, 5])
def test_noise_only_is_the_closed_form_exactly(nt):
    nodes = nodes_of("one_chunk", False)
    N = np.array([2e-9, 0.0, 4e-10])
    edges = edges_of(nt)
    got = curvedsky.curved_cov_gaussian(nodes, np.zeros((3, 3, nodes.size)), N, edges, csm.PROBES, FSKY, spins=csm.SPINS)
    want = csm.noise_matrix(N, edges, csm.PROBES, FSKY)
    assert np.array_equal(got, want)
    # (0, 0, w) twice N_0^2, (0, 2, gammat) N_0 N_2, (2, 2, xim) twice N_2^2; field 1 has no noise, so nothing else
    assert np.all(got[0, range(nt), 0, range(nt)] > 0) and np.all(got[6, range(nt), 6, range(nt)] > 0)
    assert np.all(got[2, range(nt), 2, range(nt)] > 0) and np.count_nonzero(got) == 3 * nt


# ---------------------------------------------------------------- 4. identities, bit for bit
@pytest.fixture(scope="module")
def full():
    nodes = nodes_of("two_chunks", False)
    C, N = acm.three_fields(nodes)
    edges = edges_of(5)
    return nodes, C, N, edges, curvedsky.curved_cov_gaussian(nodes, C, N, edges, csm.PROBES, FSKY)


def test_symmetry_and_repeat(full):
    nodes, C, N, edges, cov = full
    assert np.array_equal(cov, cov.transpose(2, 3, 0, 1))
    assert np.array_equal(curvedsky.curved_cov_gaussian(nodes, C, N, edges, csm.PROBES, FSKY), cov)


def test_a_subset_returns_the_bits_of_the_full_call(full):
    nodes, C, N, edges, cov = full
    pick = [4, 1, 3, 6]                                         # a subset of the probes, in another order
    sub = curvedsky.curved_cov_gaussian(nodes, C, N, edges, [csm.PROBES[p] for p in pick], FSKY)
    assert np.array_equal(sub, cov[np.ix_(pick, range(5), pick, range(5))])
    one = curvedsky.curved_cov_gaussian(nodes, C, N, edges, [csm.PROBES[3]], FSKY)
    assert np.array_equal(one[0, :, 0, :], cov[3, :, 3, :])
    bins = curvedsky.curved_cov_gaussian(nodes, C, N, edges[1:4], csm.PROBES, FSKY)        # bins 1 and 2
    assert np.array_equal(bins, cov[:, 1:3][:, :, :, 1:3])


def test_swapping_the_fields_of_a_probe_changes_nothing(full):
    nodes, C, N, edges, cov = full
    swapped = [(g, f, k) for f, g, k in csm.PROBES]
    assert np.array_equal(curvedsky.curved_cov_gaussian(nodes, C, N, edges, swapped, FSKY), cov)
    # (0, 1, gammat) written as (1, 0, gammat) is the same probe: PROBES[7] is PROBES[1]
    assert np.array_equal(cov[7, :, 7, :], cov[1, :, 1, :]) and np.array_equal(cov[1, :, 7, :], cov[1, :, 1, :])


# ---------------------------------------------------------------- 5. positive semi-definite
def test_a_full_data_vector_is_positive_semi_definite():
    """w of the lens sample, gamma_t about two source bins, xi+ and xi- of the source bins: 9 probes x 5 bins."""
    nodes = nodes_of("two_chunks", False)
    C, _ = acm.three_fields(nodes)
    N = np.array([2e-9, 1e-9, 4e-10])
    probes = [(0, 0, "w"), (0, 1, "gammat"), (0, 2, "gammat"), (1, 1, "xip"), (1, 2, "xip"), (2, 2, "xip"), (1, 1, "xim"),
              (1, 2, "xim"), (2, 2, "xim")]
    edges = edges_of(5)
    cov = curvedsky.curved_cov_gaussian(nodes, C, N, edges, probes, FSKY, spins=csm.SPINS).reshape(45, 45)
    _, gate = csm.cov_numpy(nodes, C, N, edges, probes, FSKY, with_gate=True)
    assert np.array_equal(cov, cov.T)
    eig = np.linalg.eigvalsh(cov)
    bound = float(np.max(np.sum(gate.reshape(45, 45), axis=1)))
    print(f"smallest eigenvalue {eig[0]:.3g}, largest {eig[-1]:.3g}, -(row sum of the gate) {-bound:.3g}")
    assert eig[0] >= -bound


# ---------------------------------------------------------------- 6. node weights, binned xi, projection
@pytest.mark.parametrize("every_integer", [True, False], ids=["every_integer", "17_nodes"])
@pytest.mark.parametrize("lrange", ["two_chunks_and_one", "one_chunk"])
def test_node_weights_against_the_restatement(lrange, every_integer):
    nodes = nodes_of(lrange, every_integer)
    L = acm.multipoles(nodes)
    edges = edges_of(5)
    ctx = nat.default_context(0)
    for kind in csm.KINDS:
        ref, gate = csm.node_weights_numpy(nodes, edges, kind, with_gate=True)
        got = curvedsky.node_weights_device(ctx, nodes, int(L[0]), L.size, edges, kind).numpy()
        ok, worst = within_gate(got, ref, gate, f"R_{kind}, L {lrange}, nn {nodes.size}")
        assert ok, worst
        by_node = curvedsky.node_weights_device(ctx, nodes, int(L[0]), L.size, edges, kind, by_node=True).numpy()
        assert np.array_equal(by_node.T, got)
        if every_integer:          # a node's hat is 1 at its own multipole and 0 elsewhere: R is (l + 1/2) K
            K = curvedsky.bin_averaged_wigner(L, edges, kind)
            assert np.array_equal(got, ((L + 0.5)[:, None] * K).T)


@pytest.mark.parametrize("kind", csm.KINDS)
def test_binned_correlation_function_of_one_panel_against_mpmath(kind):
    nodes, Cn = np.array([2.0, 60.0]), np.array([3e-7, -1e-7])
    edges = np.array([0.004, 0.02, 0.021, 0.4])
    got = curvedsky.curved_binned_from_cl(nodes, Cn, edges, kind)
    assert got.shape == (3,)
    ok, worst = within_gate(got, csm.binned_mpmath(nodes, Cn, edges, kind), csm.binned_gate(nodes, Cn, edges, kind),
                            f"xi_{kind} of one panel")
    assert ok, worst
    stack = curvedsky.curved_binned_from_cl(nodes, np.stack([Cn, 2.0 * Cn, np.zeros(2)]), edges, kind)
    assert np.array_equal(stack[0], got) and np.array_equal(stack[1], 2.0 * got) and np.all(stack[2] == 0)


def test_projection_of_a_rank_one_matrix_is_the_outer_product():
    nodes = nodes_of("two_chunks_and_one", False)
    C, _ = acm.three_fields(nodes)
    u, v = C[0, 1], C[1, 1]                                      # one of them negative
    edges = edges_of(5)
    for k1, k2 in (("w", "w"), ("w", "xim"), ("gammat", "xip")):
        got = curvedsky.curved_project_cl_cov(np.outer(u, v), nodes, edges, k1, k2)
        a, b = curvedsky.curved_binned_from_cl(nodes, u, edges, k1), curvedsky.curved_binned_from_cl(nodes, v, edges, k2)
        # both sides hold the same node weights; they differ by the rounding of sums of nn (and nn^2) products, bounded
        # with the restatement's |R| (nothing of the bound is the device's)
        A = np.abs(csm.node_weights_numpy(nodes, edges, k1)) @ np.abs(u) / (2 * np.pi)
        B = np.abs(csm.node_weights_numpy(nodes, edges, k2)) @ np.abs(v) / (2 * np.pi)
        gate = 2.0 * (2 * nodes.size + 8) * csm.U * np.outer(A, B)
        ok, worst = within_gate(got, np.outer(a, b), gate, f"projection of u v^T, kinds {k1}, {k2}")
        assert got.shape == (5, 5) and ok, worst


# ---------------------------------------------------------------- 7. the model level
def test_model_level_equals_the_free_functions_on_its_own_spectra():
    zs = np.array([0.3, 0.6, 0.9])
    hm = model(zs)
    hm.add_hod("g", mthresh=10 ** 10.5 + zs * 0.0)
    win_g, win_s = np.array([1.0, 2.0, 0.5]), np.array([0.002, 0.004, 0.003])
    fields = {"lens": ("g", win_g, 3e-8, 0), "src": ("nfw", win_s, 1e-10, 2)}
    probes = [("lens", "lens", "w"), ("lens", "src", "gammat"), ("src", "src", "xip"), ("src", "src", "xim")]
    idx = [(0, 0, "w"), (0, 1, "gammat"), (1, 1, "xip"), (1, 1, "xim")]
    ells = np.geomspace(20.0, 3000.0, 12)
    edges = edges_of(4)
    labels, Ctab, noise, spins = curvedsky.curved_angular_spectra_device(hm, fields, ells)
    Cl = Ctab.numpy()
    assert labels == ["lens", "src"] and spins == [0, 2] and np.array_equal(noise, [3e-8, 1e-10])
    # the spin-2 entries are the f-scaled entries of the flat path's table, bit for bit
    _, flat, _ = angcov.angular_cov_spectra_device(hm, {k: v[:3] for k, v in fields.items()}, ells)
    flat = flat.numpy()
    f = curvedsky.shear_factor(ells)
    assert np.array_equal(Cl[0, 0], flat[0, 0]) and np.array_equal(Cl[0, 1], flat[0, 1] * f)
    assert np.array_equal(Cl[1, 0], Cl[0, 1])
    assert np.array_equal(Cl[1, 1], flat[1, 1] * (((ells + 2.0) * (ells - 1.0)) / (ells * (ells + 1.0))))
    assert np.all(Cl[0, 1] != flat[0, 1])
    _, plain, _, _ = curvedsky.curved_angular_spectra_device(hm, fields, ells, shear_factor=False)
    assert np.array_equal(plain.numpy(), flat)
    cov = curvedsky.curved_angular_cov(hm, edges, probes, fields, 0.1, ells)
    assert cov.shape == (4, 4, 4, 4)
    assert np.array_equal(cov, curvedsky.curved_cov_gaussian(ells, Cl, noise, edges, idx, 0.1, spins=spins))
    assert np.all(cov[range(4), :, range(4), :][:, range(4), range(4)] > 0)          # variances
    xi = curvedsky.curved_angular_binned(hm, edges, probes, fields, ells)
    assert xi.shape == (4, 4)
    for row, (a, b, kind) in zip(xi, idx):
        assert np.array_equal(row, curvedsky.curved_binned_from_cl(ells, Cl[a, b], edges, kind))
    with pytest.raises(ValueError):
        curvedsky.curved_angular_cov(hm, edges, [("lens", "src", "xip")], fields, 0.1, ells)       # spins 0 and 2
    with pytest.raises(ValueError):
        curvedsky.curved_angular_cov(hm, edges, [("lens", "nope", "w")], fields, 0.1, ells)
    one_halo = curvedsky.curved_angular_cov(hm, edges, probes, fields, 0.1, ells, term="1h")
    assert one_halo.shape == cov.shape and not np.array_equal(one_halo, cov)
