"""GPU checks of the halo-model bispectrum of three tracers (HaloModel.get_bispectrum / bispectrum_device, hmg_bispectrum)
and of its Limber projection hmvec_amd.bispectrum.cl_bispectrum; contract and gates in DESIGN.md section 16.  The
reference computes no bispectrum, so the device is compared with the numpy restatement of the contract on the model's
own host tensors (tests/helpers/bispectrum_model.py, pinned by tests/test_bispectrum_cpu.py), every quantity at its
derived tol.

The model is section 15's, the smallest on which the kernel can still go wrong: three redshifts across the HOD's
z <= 0.8 split, 48 wavenumbers, 37 masses - the triangle kernel stages min(32, 2048 // n) masses at a time, so 37 is one
chunk of 32 and one of 5 at n = 48 and n = 1, one of 29 and one of 8 at n = 70.  A workgroup owns a block of 1024
triangles (256 threads x 4): the node list has 1674 - the 1664 closing i <= j <= l of the grid (equilateral, isosceles,
near-folded, the most squeezed closing one, the last node among them), the other five orders of a scalene one, a
duplicate and a few isosceles in other orders - and the 70-sample list 1500: a full block and a partial one each.

Measured on an MI355X (worst |got - ref| / tol): node mode B1h 0.036, B2h 0.026, B3h 0.023, J 0.023 over the six triples;
70 interpolated samples B1h 0.039, B2h 0.023, B3h 0.024, J 0.022; n = 1 at most 0.018; Pzk J_a J_b against get_power_2halo
0.0098 of twice the tol, J against two_halo_terms 0.015 of it, two_halo_terms' own I and C against the restatement 0.051;
leg permutations 0.030; Bz 0.028 against the restatement and 0.61 of 3 2^-53 sum|g B| against the sum of the device's own
per-z values; cl_bispectrum 0.0078; damping B1h 0 (the bits of undamped x D), B2h on the equilateral triangles 0.17 of the
6 ulp, B3h the same bits.  Non-vacuity: tol <= 1e-10 |ref| on 100 % of the entries of every term, node mode and n = 70."""
import ctypes as C
import itertools
import os
import sys

import numpy as np
import pytest

from hmvec_amd import _native as nat
from hmvec_amd import bispectrum as bs
from hmvec_amd.cov import limber_samples

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import bispectrum_model as bm  # noqa: E402
from lensing_model import model  # noqa: E402

pytestmark = pytest.mark.gpu

NM, NK = 37, 48
TRIPLES = [("nfw", "nfw", "nfw"), ("g", "nfw", "nfw"), ("nfw", "g", "electron"), ("y", "y", "y"), ("y", "y2", "nfw"),
           ("gc", "y", "electron")]
NON_VACUOUS = [("nfw", "nfw", "nfw"), ("g", "nfw", "nfw")]
SCALENE = (20, 22, 23)
TERMS = ("B1h", "B2h", "B3h")


@pytest.fixture(scope="module")
def h():
    zs = np.array([0.2, 0.8, 1.4])
    m = model(zs, ks=np.geomspace(1e-3, 30, NK), ms=np.geomspace(1e11, 10 ** 15.5, NM))
    m.add_battaglia_profile("electron", family="AGN", xmax=20, nxs=512)
    m.add_battaglia_pres_profile("y", family="pres", xmax=5, nxs=512)
    m.add_battaglia_pres_profile("y2", family="pres", xmax=3, nxs=512, param_override={"battaglia_pres_gamma": -0.5})
    m.add_hod("g", mthresh=10 ** 10.5 + zs * 0.0)
    m.add_hod("gc", mthresh=10 ** 11.0 + zs * 0.0, central_profile_name="electron")
    return m


@pytest.fixture(scope="module")
def node_triangles(h):
    """All closing i <= j <= l of the 48 nodes, then the other orders of a scalene one, a duplicate, isosceles in other
    orders: 1674 triangles = a block of 1024 and one of 650."""
    base = bs.default_triangles(h.ks[None, :])
    assert base.shape == (1664, 3)
    ratio = h.ks[base[:, 2]] / h.ks[base[:, 0]]
    assert ratio.max() > 1.5e4 and np.any(np.all(base == 47, axis=1)) and np.any(np.all(base == SCALENE, axis=1))
    near_folded = h.ks[base[:, 2]] / (h.ks[base[:, 0]] + h.ks[base[:, 1]])
    assert near_folded.max() > 0.97
    extra = [p for p in itertools.permutations(SCALENE) if p != SCALENE] + [SCALENE, (30, 30, 10), (30, 10, 30), (47, 46, 47),
                                                                              (3, 47, 47)]
    tri = np.concatenate([base, np.array(extra, dtype=np.int32)])
    assert tri.shape == (1674, 3)
    return tri


@pytest.fixture(scope="module")
def tables70(h):
    """70 Limber samples per redshift - k = (l + 1/2) / chi of 70 multipoles in any order, so a triangle that closes at
    one redshift closes at all - with section 15's special entries: the last node with f = 0, an interior node with
    f = 0, a fraction close to 1, a zero and a negative scale; and 1500 of the triangles that close at every redshift."""
    rng = np.random.default_rng(11)
    ells = rng.permutation(np.geomspace(30.0, 12000.0, 70))
    idx, frac = limber_samples(ells, np.array([800.0, 2800.0, 4200.0]), h.ks)
    idx, frac = idx.astype(np.int64), frac.copy()
    scale = rng.uniform(0.5, 2.0, (3, 70))
    idx[:, 5], frac[:, 5] = 47, 0.0
    idx[1, 64], frac[1, 64] = 47, 0.0
    frac[:, 9] = 0.0
    frac[0, 66] = 1.0 - 2.0 ** -30
    scale[:, 13] = 0.0
    scale[2, 69] = 0.0
    scale[:, 21] = -1.25
    close = bs.default_triangles(bs.sample_wavenumbers(h.ks, idx, frac))
    assert close.shape[0] > 3000
    tri = close[rng.permutation(close.shape[0])[:1500]]
    tri = tri[np.arange(1500)[:, None], rng.permuted(np.tile(np.arange(3), (1500, 1)), axis=1)]       # legs in any order
    assert np.any(tri == 13) and np.any(tri == 5) and np.any(tri == 21)
    return idx, frac, scale, tri


def device(h, names, tri, **kw):
    """(B (3, nz, nt), J (3, nz, n)) on the host."""
    B, _, J = h._bispectrum(*names, tri, kw.pop("kindex", None), kw.pop("damping", True), kw.pop("idx", None),
                            kw.pop("frac", None), kw.pop("scale", None), None, True, want_J=True)
    assert not kw
    return B.numpy(), J.numpy()


@pytest.fixture(scope="module")
def nodes(h, node_triangles):
    """Per triple: the device's (B, J) at the node triangles with damping, and the restatement.  Shared, never changed."""
    return {t: device(h, t, node_triangles) + (bm.bispectrum(h, t, node_triangles),) for t in TRIPLES}


def within(got, ref, tol, what):
    err = np.abs(got - ref)
    worst = float(np.max(np.where(err == 0, 0.0, err / np.maximum(tol, 1e-300))))
    print(f"{what}: worst |got - ref| / tol = {worst:.3g}")
    return bool(np.all(err <= tol)), worst


def check_terms(B, J, ref, what):
    assert np.all(np.isfinite(B)) and np.all(np.isfinite(J))
    for i, key in enumerate(TERMS):
        ok, worst = within(B[i], ref[key][0], ref[key][1], f"{what} {key}")
        assert ok, (key, worst)
    ok, worst = within(J, ref["J"][0], ref["J"][1], f"{what} J")
    assert ok, worst


def non_vacuous(ref, what):
    """The condition of section 16: each term's tol is <= 1e-10 |ref| on at least 95 % of the (z, t) entries."""
    for key in TERMS:
        share = float(np.mean(ref[key][1] <= 1e-10 * np.abs(ref[key][0])))
        print(f"{what} {key}: tol <= 1e-10 |ref| on {100 * share:.1f} % of the entries")
        assert share >= 0.95, (key, share)


# ---------------------------------------------------------------- 1. the terms against the restatement
@pytest.mark.parametrize("triple", TRIPLES)
def test_nodes_against_the_restatement(h, nodes, node_triangles, triple):
    B, J, ref = nodes[triple]
    assert B.shape == (3, 3, 1674) and J.shape == (3, 3, 48) and np.any(B != 0)
    check_terms(B, J, ref, f"{triple} nodes")
    if triple in NON_VACUOUS:
        non_vacuous(ref, f"{triple} nodes")
    # through the public calls: the same bits
    got = h.get_bispectrum(*triple, triangles=node_triangles, term="2h")
    assert np.array_equal(got, B[1])
    assert np.array_equal(h.get_bispectrum(*triple, triangles=node_triangles), B[0] + B[1] + B[2])


@pytest.mark.parametrize("triple", TRIPLES)
def test_interpolated_samples(h, tables70, triple):
    idx, frac, scale, tri = tables70
    for damping in (True, False):
        B, J = device(h, triple, tri, idx=idx, frac=frac, scale=scale, damping=damping)
        ref = bm.bispectrum(h, triple, tri, idx=idx, frac=frac, scale=scale, damping=damping)
        assert B.shape == (3, 3, 1500) and J.shape == (3, 3, 70)
        check_terms(B, J, ref, f"{triple} n = 70 damping={damping}")
        zero = np.any(scale[:, tri] == 0, axis=2)
        assert zero.any() and np.all(B[:, zero] == 0) and np.all(B[0][~zero] != 0)         # a zero scale: an exact zero
        if triple in NON_VACUOUS:
            non_vacuous(ref, f"{triple} n = 70 damping={damping}")


@pytest.mark.parametrize("triple", TRIPLES)
def test_one_triangle_and_one_sample(h, nodes, node_triangles, triple):
    B, J, ref = nodes[triple]
    t = 1664                                                    # a permutation of the scalene triangle
    one, _ = device(h, triple, node_triangles[t:t + 1])
    assert one.shape == (3, 3, 1) and np.array_equal(one[:, :, 0], B[:, :, t])
    # n = 1: the only triangle is the equilateral one of that sample
    eq = int(np.flatnonzero(np.all(node_triangles == 17, axis=1))[0])
    B1, J1 = device(h, triple, np.array([[0, 0, 0]]), kindex=np.array([17]))
    assert B1.shape == (3, 3, 1) and J1.shape == (3, 3, 1)
    ref1 = bm.bispectrum(h, triple, np.array([[0, 0, 0]]), kindex=np.array([17]))
    check_terms(B1, J1, ref1, f"{triple} n = 1")
    assert np.array_equal(B1[:, :, 0], B[:, :, eq]) and np.array_equal(J1[:, :, 0], J[:, :, 17])
    default = h.get_bispectrum(*triple, kindex=np.array([17]), term="1h")
    assert default.shape == (3, 1) and np.array_equal(default, B1[0])


# ---------------------------------------------------------------- 2. the tie to the gated two-point code
def test_two_halo_bracket_against_the_power_spectra(h, nodes):
    """At the nodes Pzk J_a J_b is get_power_2halo(a, b), and J is (I + b) - C of two_halo_terms."""
    J = {"nfw": nodes[("g", "nfw", "nfw")], "g": nodes[("g", "nfw", "nfw")], "y": nodes[("y", "y", "y")]}
    leg = {"nfw": 1, "g": 0, "y": 0}

    def bracket(name):          # (device J, restatement (value, tol)) of one name, (nz, 48)
        _, Jd, ref = J[name]
        return Jd[leg[name]], (ref["J"][0][leg[name]], ref["J"][1][leg[name]])

    P = (h.Pzk, 3 * bm.EPS * np.abs(h.Pzk))
    for a, b in (("nfw", "g"), ("y", "nfw"), ("g", "g")):
        (Ja, ra), (Jb, rb) = bracket(a), bracket(b)
        tol = bm.prod(P, ra, rb)[1]
        got = h.Pzk * Ja * Jb
        ok, worst = within(got, h.get_power_2halo(a, b), 2 * tol, f"Pzk J_{a} J_{b} against get_power_2halo (of twice the tol)")
        assert ok, worst
    for name in ("nfw", "y", "g"):
        Jd, (rv, rt) = bracket(name)
        I1, C1, _, _ = h.two_halo_terms(name)
        ref = nodes[("g", "nfw", "nfw")][2] if name != "y" else nodes[("y", "y", "y")][2]
        bias = ref["b"][0][leg[name]][:, None]
        want = (I1 + bias) - C1
        ok, worst = within(Jd, want, 2 * rt, f"J_{name} against two_halo_terms (of twice the tol)")
        assert ok, worst
        ok, worst = within(I1, ref["I"][0][leg[name]], ref["I"][1][leg[name]], f"I_{name} of two_halo_terms against the restatement")
        assert ok, worst
        ok, worst = within(C1[:, 0], ref["C"][0][leg[name]], ref["C"][1][leg[name]], f"C_{name} of two_halo_terms against the restatement")
        assert ok, worst


# ---------------------------------------------------------------- 3. permutations of the legs
def test_leg_permutations(h, nodes, node_triangles):
    triple = ("nfw", "g", "electron")
    B, _, ref = nodes[triple]
    for perm in itertools.permutations(range(3)):
        names = tuple(triple[i] for i in perm)
        Bp, _ = device(h, names, np.ascontiguousarray(node_triangles[:, perm]))
        for i, key in enumerate(TERMS):
            ok, worst = within(Bp[i], B[i], ref[key][1], f"{names} {key} against {triple}")
            assert ok, (perm, key, worst)
    # the six orders of the scalene triangle in one list: six different values of a triple of three different tracers,
    # one value (within the gate) of a triple of one tracer
    rows = [1664 + i for i in range(5)] + [int(np.flatnonzero(np.all(node_triangles == SCALENE, axis=1))[0])]
    assert len({float(v) for v in B[0][0, rows]}) == 6
    Bn, _, refn = nodes[("nfw", "nfw", "nfw")]
    for i, key in enumerate(TERMS):
        assert np.all(np.abs(Bn[i][:, rows] - Bn[i][:, rows[:1]]) <= refn[key][1][:, rows])
    assert np.array_equal(Bn[:, :, 1669], Bn[:, :, rows[5]])                      # the duplicate: the same bits


# ---------------------------------------------------------------- 4. determinism and independence
def shifted(t, z, nm, nk):
    """The hmg_tracer of redshift z alone: every pointer moved to that redshift's slice."""
    o = nat.Tracer()
    C.memmove(C.byref(o), C.byref(t), C.sizeof(nat.Tracer))
    for field, step in (("d_prof", nm * nk), ("d_cprof", nm * nk), ("d_Nc", nm), ("d_Ns", nm), ("d_NcNs", nm),
                        ("d_NsNsm1", nm), ("d_ngal", 1)):
        p = getattr(o, field)
        if p:
            setattr(o, field, p + 8 * z * step)
    return o


def test_determinism_and_independence(h, nodes, node_triangles, tables70):
    triple = ("gc", "y", "electron")
    B, J, _ = nodes[triple]
    again, Jagain = device(h, triple, node_triangles)
    assert np.array_equal(again, B) and np.array_equal(Jagain, J)                                # repeat
    sub = np.array([3, 700, 1023, 1024, 1500, 1673])           # from both blocks, alone in one (other threads, too)
    part, _ = device(h, triple, node_triangles[sub])
    assert np.array_equal(part, B[:, :, sub])
    idx, frac, scale, tri = tables70
    full, Jfull = device(h, triple, tri, idx=idx, frac=frac, scale=scale)
    part, _ = device(h, triple, tri[1000:1100], idx=idx, frac=frac, scale=scale)
    assert np.array_equal(part, full[:, :, 1000:1100])
    # one redshift alone: the entry point on that redshift's slices of every array
    nz, n, nt = 3, 70, 1500
    ctx = h._ctx()
    tr = [h._tracer(r, 1) for r in h._resolve(*triple)]
    d_tri = ctx.upload_int32(tri)
    for z in range(nz):
        tz = [shifted(t, z, NM, NK) for t in tr]
        d_idx, d_frac, d_scale = ctx.upload_int32(idx[z]), ctx.upload(frac[z]), ctx.upload(scale[z])
        out, outJ = ctx.empty((3, 1, nt)), ctx.empty((3, 1, n))
        ctx.call("hmg_bispectrum", 1, NM, NK, n, nt, *(C.byref(t) for t in tz), h._d_nzm.ptr + 8 * z * NM,
                 h._d_bh.ptr + 8 * z * NM, h._d_ms().ptr, h._d_wm().ptr, h._d_ks().ptr, h._d_Pzk().ptr + 8 * z * NK,
                 h._rho_m0(), float(h.p["kstar_damping"]), d_idx.ptr, d_frac.ptr, d_scale.ptr, d_tri.ptr, None, out.ptr,
                 None, outJ.ptr)
        assert np.array_equal(out.numpy()[:, 0], full[:, z]), z
        assert np.array_equal(outJ.numpy()[:, 0], Jfull[:, z]), z


# ---------------------------------------------------------------- 5. the z sum
def test_z_sum(h, tables70):
    triple = ("g", "nfw", "nfw")
    idx, frac, scale, tri = tables70
    g = np.array([0.7, -1.3, 2.1])
    B, Bz = h.bispectrum_device(*triple, triangles=tri, idx=idx, frac=frac, scale=scale, zweights=g)
    B, Bz = B.numpy(), Bz.numpy()
    assert Bz.shape == (3, 1500)
    # against the sum of the device's own per-z values: nz roundings of the running sum
    absum = np.einsum("z,kzt->kt", np.abs(g), np.abs(B))
    exact = np.einsum("z,kzt->kt", g.astype(np.longdouble), B.astype(np.longdouble))          # (no rounding of its own)
    ok, worst = within(Bz, exact.astype(np.float64), 3 * 2.0 ** -53 * absum, "Bz against sum_z g B (of 3 2^-53 sum|g B|)")
    assert ok, worst
    ref = bm.bispectrum(h, triple, tri, idx=idx, frac=frac, scale=scale)
    for i, key in enumerate(TERMS):
        want, tol = bm.zsum(g, ref[key])
        ok, worst = within(Bz[i], want, tol, f"Bz {key} against the restatement")
        assert ok, worst
    # asked for alone (the per-z terms then live in a temporary block): the same bits
    none, alone = h.bispectrum_device(*triple, triangles=tri, idx=idx, frac=frac, scale=scale, zweights=g, per_z=False)
    assert none is None and np.array_equal(alone.numpy(), Bz)


# ---------------------------------------------------------------- 6. the Limber projection
@pytest.mark.parametrize("triple", [("y", "y", "y"), ("g", "nfw", "nfw")])
def test_cl_bispectrum(h, triple):
    ell = np.array([[200.0, 1000.0, 1000.0], [3000.0, 3000.0, 200.0], [1000.0, 3000.0, 2500.0]])
    W = (np.array([0.5, 1.0, 0.8]), 1.5, np.array([2.0, 1.0, 0.5]))
    tri, idx, frac, g = bs.limber_tables(h, ell, *W)
    ref = bm.bispectrum(h, triple, tri, idx=idx, frac=frac, damping=True)
    parts = []
    for key, term in zip(TERMS, ("1h", "2h", "3h")):
        got = bs.cl_bispectrum(h, ell, *triple, W1=W[0], W2=W[1], W3=W[2], term=term)
        assert got.shape == (3,) and np.all(got != 0)
        want, tol = bm.zsum(g, ref[key])
        ok, worst = within(got, want, tol, f"cl_bispectrum {triple} {term}")
        assert ok, worst
        parts.append(got)
    total = bs.cl_bispectrum(h, ell, *triple, W1=W[0], W2=W[1], W3=W[2])
    absum = sum(np.abs(p) for p in parts)
    ok, worst = within(total, parts[0] + parts[1] + parts[2], 3 * bm.EPS * absum, "the terms' sum against total (of 3 EPS)")
    assert ok, worst
    undamped = bs.cl_bispectrum(h, ell, *triple, W1=W[0], W2=W[1], W3=W[2], term="1h", damping=False)
    assert np.all(np.abs(undamped) >= np.abs(parts[0]))          # (D <= 1; exactly 1 where k is far above kstar)


# ---------------------------------------------------------------- 7. damping
def test_damping_is_a_factor_per_leg(h, nodes, node_triangles):
    """B1h(damped) = B1h(undamped) D_1 D_2 D_3 and, on the equilateral triangles, where the three pieces share D_s^2,
    B2h(damped) = B2h(undamped) D_s^2, within 6 ulp; B3h carries no damping: the same bits.  (B2h comes back as one sum:
    which D pair multiplies which piece on the other triangles is checked against the restatement alone, at its tol.)"""
    D = bs.damping(h.ks, h.p["kstar_damping"])
    s1, s2, s3 = node_triangles.T
    eq = (s1 == s2) & (s2 == s3)
    assert eq.sum() == 48
    for triple in NON_VACUOUS:
        Bd, Jd, _ = nodes[triple]
        Bu, Ju = device(h, triple, node_triangles, damping=False)
        assert np.all(Jd > 0)                                # (the pieces of B2h have one sign: its ulp count holds)
        want = Bu[0] * (D[s1] * D[s2] * D[s3])[None, :]
        ok, worst = within(Bd[0], want, 6 * bm.EPS * np.abs(want), f"{triple} B1h damping (of 6 ulp)")
        assert ok, worst
        want = Bu[1][:, eq] * (D[s1[eq]] * D[s1[eq]])[None, :]
        ok, worst = within(Bd[1][:, eq], want, 6 * bm.EPS * np.abs(want), f"{triple} B2h damping, equilateral (of 6 ulp)")
        assert ok, worst
        assert np.array_equal(Bd[2], Bu[2]) and np.array_equal(Jd, Ju)
        assert np.all(np.abs(Bd[1]) <= np.abs(Bu[1]))


# ---------------------------------------------------------------- 8. refusals, all before a launch
def test_errors(h, node_triangles):
    with pytest.raises(NotImplementedError, match=r"\('g', 'gc', 'nfw'\).*third factorial moments"):
        h.get_bispectrum("g", "gc", "nfw")
    with pytest.raises(NotImplementedError, match=r"\('nfw', 'g', 'g'\)"):
        h.bispectrum_device("nfw", "g", "g")
    with pytest.raises(NotImplementedError):
        h.get_bispectrum("g")
    with pytest.raises(ValueError, match=r"t = 1 does not close at z = 0\.2"):
        h.get_bispectrum("nfw", triangles=np.array([[0, 0, 0], [0, 1, 40]]))
    idx = np.tile(np.array([10, 10, 10]), (3, 1))
    frac = np.array([[0.0, 0.5, 0.9], [0.0, 0.5, 0.9], [0.0, 0.5, 0.9]])
    idx[2, 2] = 30
    with pytest.raises(ValueError, match=r"t = 0 does not close at z = 1\.4"):
        h.bispectrum_device("nfw", triangles=np.array([[0, 1, 2]]), idx=idx, frac=frac)
    with pytest.raises(ValueError, match=r"t = 1 names sample .*n - 1 = 47"):
        h.get_bispectrum("nfw", triangles=np.array([[0, 0, 0], [1, 48, 1]]))
    with pytest.raises(ValueError, match=r"n - 1 = 1"):
        h.get_bispectrum("nfw", kindex=np.array([3, 4]), triangles=np.array([[0, 1, 2]]))
    with pytest.raises(ValueError, match="at most 256"):
        h.get_bispectrum("nfw", kindex=np.zeros(257, dtype=int))
    with pytest.raises(ValueError, match="nosuch"):
        h.get_bispectrum("nosuch")
    with pytest.raises(ValueError, match="nosuch"):
        h.get_bispectrum("nfw", "y", "nosuch")
    with pytest.raises(ValueError, match="frac = 0"):
        h.bispectrum_device("nfw", idx=np.array([47]), frac=np.array([0.5]))
    with pytest.raises(ValueError, match="term"):
        h.get_bispectrum("nfw", term="4h")
    with pytest.raises(ValueError, match="ell = 200000.0"):
        bs.cl_bispectrum(h, [[500.0, 200000.0, 200000.0]], "nfw")
    # the entry point itself refuses bad tables and triangles before it reads anything through them
    ctx = h._ctx()
    t = h._tracer(h._resolve("nfw")[0], 1)
    g = h._tracer(h._resolve("g")[0], 1)
    ones, zeros = ctx.upload(np.ones(6)), ctx.upload(np.zeros(6))
    d_idx = ctx.upload_int32(np.array([3, 4, 4, 5, 40, 41]))
    d_tri, out = ctx.upload_int32(np.array([[0, 1, 1]])), ctx.empty((3, 3, 1))

    def call(n, nt, a, b, c, d_idx, d_frac, d_tri, d_g, d_B, d_Bz):
        ctx.call("hmg_bispectrum", 3, NM, NK, n, nt, C.byref(a), C.byref(b), C.byref(c), h._d_nzm.ptr, h._d_bh.ptr,
                 h._d_ms().ptr, h._d_wm().ptr, h._d_ks().ptr, h._d_Pzk().ptr, h._rho_m0(), 0.01, d_idx.ptr, d_frac.ptr,
                 ones.ptr, d_tri.ptr, nat.ptr(d_g), nat.ptr(d_B), nat.ptr(d_Bz), None)

    call(2, 1, t, t, t, d_idx, zeros, d_tri, None, out, None)                    # (good arguments; each call below has one bad one)
    with pytest.raises(nat.NativeError, match="does not close"):                 # the second redshift: nodes (40, 3, 3)
        call(2, 1, t, t, t, ctx.upload_int32(np.array([3, 4, 40, 3, 4, 5])), zeros, d_tri, None, out, None)
    with pytest.raises(nat.NativeError, match="outside 0 .. n-1"):
        call(2, 1, t, t, t, d_idx, zeros, ctx.upload_int32(np.array([[0, 2, 1]])), None, out, None)
    with pytest.raises(nat.NativeError, match="outside 0 .. n-1"):
        call(2, 1, t, t, t, d_idx, zeros, ctx.upload_int32(np.array([[-1, 0, 1]])), None, out, None)
    with pytest.raises(nat.NativeError, match="nk-1"):
        call(2, 1, t, t, t, ctx.upload_int32(np.array([3, 4, 4, 3, 47, 47])), ctx.upload(np.array([0, 0, 0, 0, 0, 0.5])),
             d_tri, None, out, None)
    with pytest.raises(nat.NativeError, match="nk-1"):
        call(2, 1, t, t, t, ctx.upload_int32(np.array([3, 4, 4, 3, 48, 47])), zeros, d_tri, None, out, None)
    with pytest.raises(nat.NativeError, match="no output"):
        call(2, 1, t, t, t, d_idx, zeros, d_tri, None, None, None)
    with pytest.raises(nat.NativeError, match="d_zweights"):
        call(2, 1, t, t, t, d_idx, zeros, d_tri, None, None, out)
    with pytest.raises(nat.NativeError, match="no sample"):
        call(0, 1, t, t, t, d_idx, zeros, d_tri, None, out, None)
    with pytest.raises(nat.NativeError, match="no triangles"):
        call(2, 0, t, t, t, d_idx, zeros, d_tri, None, out, None)
    with pytest.raises(nat.NativeError, match="256 samples"):
        call(257, 1, t, t, t, d_idx, zeros, d_tri, None, out, None)
    with pytest.raises(nat.NativeError, match="HOD tracers"):
        call(2, 1, g, t, g, d_idx, zeros, d_tri, None, out, None)
    call(2, 1, t, t, t, d_idx, zeros, d_tri, None, out, None)                    # and the context is as good as before
    assert np.all(np.isfinite(out.numpy()))
