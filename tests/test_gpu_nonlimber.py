"""GPU checks of the non-Limber projection (hmvec_amd.nonlimber: spherical_bessel, nonlimber_transfer, nonlimber_cl;
definitions and gates in DESIGN.md section 29).  The reference computes none of this: the
device's j_l is pinned by 40-digit mpmath, the transfers and spectra by the numpy restatement that
tests/test_nonlimber_cpu.py pins against mpmath, the rest by bit-identities.

Gates, none taken from the device's output.  j_l: c 2^-53 max(|j_l|, min(1, 1/x)) with c = 4 CJ_ABS, CJ_ABS = 100.6 the
restatement's worst constant (the CPU test measures it); the factor 4 is for the device libm's sin and cos and the fused
steps.  Transfers: device and restatement are each within (4 CJ, CJ) 2^-53 envelope of the true j_l, and a sum of ngz
products rounds at most ngz + 2 times on each side: [5 CJ + 2 (ngz + 2)] 2^-53 sum_g |src| max(|j_l|, min(1, 1/x))
(nonlimber_model.transfer).  Spectra: 2 (nkq + 4) 2^-53 (2/pi) sum |w T_a T_b| for the k sum's roundings, plus the
transfers' bounds propagated through the product (nonlimber_model.cl)."""
import os
import sys

import numpy as np
import pytest

from hmvec_amd import _native as nat
from hmvec_amd import nonlimber

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import nonlimber_model as nlm  # noqa: E402

pytestmark = pytest.mark.gpu

CJ = 101.0                                   # CJ_ABS = 100.6 of tests/test_nonlimber_cpu.py, rounded up
WIDTH, TILE, FMAX = (nat.DEFINES["HMG_NONLIMBER_" + n] for n in ("THREADS", "TILE", "FMAX"))


def within_gate(got, ref, gate, what):
    err = np.abs(got - ref)
    worst = float(np.max(err / np.maximum(gate, 1e-300)))
    print(f"{what}: worst |got - ref| / gate = {worst:.3g}")
    return bool(np.all(err <= gate)) and bool(np.all(np.isfinite(got))), worst


# ---------------------------------------------------------------- 1. j_l against mpmath
@pytest.mark.parametrize("lmax", nlm.PROBE_LMAX)
def test_sph_bessel_against_mpmath(lmax):
    xs = nlm.probe_points(lmax)
    got = nonlimber.spherical_bessel(lmax, xs)
    assert got.shape == (lmax + 1, xs.size) and np.all(np.isfinite(got))
    worst, rel, frac = nlm.bessel_errors(lmax, xs, got)
    print(f"lmax {lmax}: worst constant {worst:.1f} of the gate's {4 * CJ:.0f} ({worst / (4 * CJ):.3f}); relative, x < l: {rel:.1f}")
    assert np.all(frac <= 4.0 * CJ)
    assert np.array_equal(nonlimber.spherical_bessel(lmax, xs), got)
    assert np.array_equal(nonlimber.spherical_bessel(lmax, xs[3:5]), got[:, 3:5])      # a value depends on its x and lmax
    if lmax == 256:                          # underflow: exact zeros (x = 0.05: below the denormals from l = 102 on)
        col = got[:, list(xs).index(0.05)]
        assert np.all(col[102:] == 0.0) and np.all(col[:91] > 0.0)


# ---------------------------------------------------------------- 2. transfers and spectra against the restatement
def rule(ngz, nkq, kmax=0.05):
    """chi nodes on [1400, 1600] (one node: 1500) and k nodes up to kmax, capped where the chi rule is at Nyquist / 1.05."""
    chis = np.linspace(1400.0, 1600.0, ngz) if ngz > 1 else np.array([1500.0])
    top = min(kmax, 3.0 / (chis[1] - chis[0])) if ngz > 1 else kmax
    return (np.linspace(1e-3, top, nkq) if nkq > 1 else np.array([top])), chis


def sources_of(F, ngz, nkq, seed=7):
    return np.random.default_rng(seed).normal(size=(F, ngz, nkq))


# (F, ngz, nkq, lmax): every F of {1, 3, 16, 17}, ngz of {1, 2, W - 1, W, W + 1, 2 W + 1}, nkq of {1, 2, 65}, lmax of
# {0, 1, T - 1, T, T + 1, 40}; x = kq chi runs from 1.4 to 80, so lmax = 40 has k nodes on both branches
CASES = [(1, 1, 1, 0), (3, 2, 2, 1), (16, WIDTH - 1, 65, TILE - 1), (17, WIDTH, 2, TILE), (3, WIDTH + 1, 65, TILE + 1),
         (1, 2 * WIDTH + 1, 65, 40), (16, 2 * WIDTH + 1, 2, 40), (17, WIDTH + 1, 1, 40), (3, 1, 65, 40)]


@pytest.mark.parametrize("F, ngz, nkq, lmax", CASES)
def test_transfer_against_the_restatement(F, ngz, nkq, lmax):
    kq, chis = rule(ngz, nkq)
    src = sources_of(F, ngz, nkq)
    got = nonlimber.nonlimber_transfer(kq, chis, src, lmax)
    ref, gate = nlm.transfer(kq, chis, src, lmax, with_gate=True, cj=CJ)
    assert got.shape == (F, lmax + 1, nkq)
    ok, worst = within_gate(got, ref, gate, f"T, F {F}, ngz {ngz}, nkq {nkq}, lmax {lmax}")
    assert ok, worst


def test_transfer_one_workgroup_on_both_branches():
    """k chi from 37.4 to 42.7 at lmax = 40: lanes of one chunk walk upwards, their neighbours downwards."""
    kq, chis = np.array([0.0267]), np.linspace(1400.0, 1600.0, WIDTH)
    x = kq[0] * chis
    assert x.min() < 40 <= x.max() and 50 < np.count_nonzero(x >= 40) < WIDTH - 50
    src = sources_of(3, WIDTH, 1, seed=11)
    got = nonlimber.nonlimber_transfer(kq, chis, src, 40)
    ref, gate = nlm.transfer(kq, chis, src, 40, with_gate=True, cj=CJ)
    ok, worst = within_gate(got, ref, gate, "T, one chunk on both branches")
    assert ok, worst
    # the lanes of one branch alone (the others' sources zero): the two parts add up to the whole within the gate
    up = np.where((x >= 40)[None, :, None], src, 0.0)
    parts = nonlimber.nonlimber_transfer(kq, chis, up, 40) + nonlimber.nonlimber_transfer(kq, chis, src - up, 40)
    assert np.all(np.abs(parts - got) <= gate)


def test_transfer_tiny_arguments_give_exact_zeros():
    kq, chis = np.array([5e-3 / 1500.0]), np.array([1500.0])
    got = nonlimber.nonlimber_transfer(kq, chis, np.full((2, 1, 1), 3.0), 200)
    ref, gate = nlm.transfer(kq, chis, np.full((2, 1, 1), 3.0), 200, with_gate=True, cj=CJ)
    assert np.all(np.isfinite(got)) and np.all(got[:, 90:] == 0.0) and np.all(got[:, :70] > 0.0)
    ok, worst = within_gate(got, ref, gate, "T at kq chi = 5e-3, lmax 200")
    assert ok, worst


def test_transfer_of_a_unit_source_is_the_probe():
    """One chi node with source 1: T_l(k) = j_l(k chi), the bits of hmg_sph_bessel - the kernel's tiled walk is sb_all's."""
    for lmax in (0, TILE - 1, TILE, 40):
        kq, chis = rule(1, 65, kmax=0.06)
        got = nonlimber.nonlimber_transfer(kq, chis, np.ones((1, 1, 65)), lmax)
        assert np.array_equal(got[0], nonlimber.spherical_bessel(lmax, kq * chis[0]))


@pytest.mark.parametrize("F, nkq, lmax", [(1, 1, 0), (3, 65, TILE + 1), (17, 200, 40)])
def test_cl_against_the_restatement(F, nkq, lmax):
    rng = np.random.default_rng(5)
    kq = np.linspace(1e-3, 0.1, nkq) if nkq > 1 else np.array([0.02])
    wk = rng.uniform(0.5, 1.5, nkq)
    T = rng.normal(size=(F, lmax + 1, nkq))
    pairs = [(a, b) for a in range(F) for b in range(a, F)][:40] + [(F - 1, 0)]
    got = nonlimber.nonlimber_cl(kq, wk, T, pairs)
    ref, gate = nlm.cl(kq, wk, T, pairs, with_gate=True)
    assert got.shape == (len(pairs), lmax + 1)
    ok, worst = within_gate(got, ref, gate, f"C_l, F {F}, nkq {nkq}, lmax {lmax}")
    assert ok, worst


# ---------------------------------------------------------------- 3. identities, bit for bit
@pytest.fixture(scope="module")
def full():
    kq, chis = rule(2 * WIDTH + 1, 65)
    src = sources_of(17, 2 * WIDTH + 1, 65, seed=3)
    return kq, chis, src, nonlimber.nonlimber_transfer(kq, chis, src, 40)


def test_repeat_and_device_input(full):
    kq, chis, src, T = full
    assert np.array_equal(nonlimber.nonlimber_transfer(kq, chis, src, 40), T)
    ctx = nat.default_context(0)
    dev = nonlimber.nonlimber_transfer_device(kq, chis, ctx.upload(src), 40, ctx=ctx)
    assert isinstance(dev, nat.DeviceArray) and np.array_equal(dev.numpy(), T)
    wk = np.linspace(1.0, 2.0, kq.size)
    pairs = [(0, 1), (16, 16), (3, 9)]
    C = nonlimber.nonlimber_cl(kq, wk, T, pairs)
    assert np.array_equal(nonlimber.nonlimber_cl_device(kq, wk, dev, pairs, ctx=ctx).numpy(), C)
    assert np.array_equal(nonlimber.nonlimber_cl(kq, wk, T, pairs), C)


def test_a_field_alone_and_a_field_among_sixteen(full):
    kq, chis, src, T = full
    for f in (0, 5, 15, 16):                 # 16 is the field the split puts into a launch of its own
        assert np.array_equal(nonlimber.nonlimber_transfer(kq, chis, src[f:f + 1], 40)[0], T[f])
    assert np.array_equal(nonlimber.nonlimber_transfer(kq, chis, src[[9, 2, 4]], 40), T[[9, 2, 4]])


def test_a_k_node_alone_and_a_k_node_among_65(full):
    kq, chis, src, T = full
    for i in (0, 17, 64):
        alone = nonlimber.nonlimber_transfer(kq[i:i + 1], chis, np.ascontiguousarray(src[:3, :, i:i + 1]), 40)
        assert np.array_equal(alone[:, :, 0], T[:3, :, i])


def test_pair_order_and_pair_subsets(full):
    kq, _, _, T = full
    wk = np.linspace(1.0, 2.0, kq.size)
    pairs = [(a, b) for a in range(5) for b in range(5)]
    C = nonlimber.nonlimber_cl(kq, wk, T, pairs).reshape(5, 5, -1)
    assert np.array_equal(C, C.transpose(1, 0, 2))                                  # C[(a, b)] is C[(b, a)]
    assert np.array_equal(nonlimber.nonlimber_cl(kq, wk, T, pairs[::-1]).reshape(5, 5, -1), C[::-1, ::-1])
    assert np.array_equal(nonlimber.nonlimber_cl(kq, wk, T, [(3, 1)])[0], C[1, 3])
    assert np.all(C[range(5), range(5)] > 0)
