"""Pins helpers/profile_model.py - the 40-digit discrete reference of the radial-profile transform, its error scale, its
row sets and the constants K of the gate in tests/test_gpu_profile_rows.py - without a device:
the model against itself at 60 digits and against an mpmath-only direct sum, the float64 numpy restatement and the
oracle inside the gate, every row set on the branches it claims, the fills and ties against numpy's own."""
import os
import sys

import mpmath as mp
import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import profile_model as pm  # noqa: E402

def test_forty_and_sixty_digits_agree():
    for name in ("rt30-T1", "rocfft45-T2", "rt16-nonorm-post-logx", "table1000-r8-T2"):
        c = pm.CASES[name]
        a, b = pm.reference(c, 40), pm._reference(c, 60)
        scale = np.where(a["S"] > 0, a["S"], 1.0)
        assert np.max(np.abs((a["hi"] - b["hi"]) + (a["lo"] - b["lo"])) / scale) < 1e-30, name
        assert np.array_equal(a["S"] == 0, b["S"] == 0) and np.allclose(a["S"], b["S"], rtol=1e-12, atol=0)


@pytest.mark.parametrize("N,nn", [(16, 16), (30, 17), (45, 45), (600, 431), (5000, 1500), (7000, 90)])
def test_integer_sums_and_transform_equal_the_mpmath_direct_sum(N, nn):
    rng = np.random.default_rng(N)
    with mp.workdps(60):
        y = [mp.mpf(float(v)) * mp.exp(mp.mpf(-3 * n) / N) / 3 for n, v in enumerate(rng.standard_normal(nn))]
        modes = sorted({0, 1, 2, N // 3, N // 2 - 1, N // 2})
        want = pm.sine_sums_mpmath(y, N, modes, 60)
        l1 = mp.fsum(abs(v) for v in y)
        for method in ("direct", "fft"):
            got = pm.sine_sums(y, N, modes, 40, method)
            assert max(abs(g - w) for g, w in zip(got, want)) < mp.mpf(10) ** -38 * l1, (N, method)
        if N % 2 == 0:
            assert pm.sine_sums(y, N, [N // 2], 40, "direct")[0] == 0       # sin(pi n): exactly zero


def test_restatement_sits_inside_its_constants():
    """The numpy restatement's worst ratio per route: inside K / 4 and above K / 16, so that no literal goes stale; the
    oracle (its own power-law form of the family) inside K; every K below the operation-count bound."""
    worst, worst_oracle, uniform = {}, {}, {}
    # one reference per row set (a "-T3" grid and the aliases share their T2's rows, targets and reference)
    for name in [n for n, c in pm.CASES.items() if not c.same_as]:
        c = pm.CASES[name]
        ref = pm.reference(c)
        out, cc = pm.restatement(c)
        r = max(float(pm.ratios(out, ref["hi"], ref["lo"], ref["S"]).max()),
                float(pm.ratios(cc, ref["u1hi"], ref["u1lo"], ref["S1"]).max()))
        if name.endswith("-T1") and c.nxs % 2 == 0 and c.route in ("spec2500", "ct", "rt", "table"):
            # the one-row kernels' own output side (modes at j k_lo, every T1 target on a knot): inside the gate as well
            ru = float(pm.ratios(pm.restatement(c, uniform=True)[0], ref["hi"], ref["lo"], ref["S"]).max())
            uniform[name] = round(ru, 4)
            assert ru <= pm.K[c.route] / 2, (name, ru)
        ro = float(pm.ratios(pm.oracle_call(c), ref["hi"], ref["lo"], ref["S"]).max())
        # the aliases of a reference are gated with their own route's K: chirp30000-T2 with pruned30000-T2's rows
        for route in {c.route} | {a.route for a in pm.CASES.values() if a.same_as == name}:
            worst[route] = max(worst.get(route, 0.0), r)
            worst_oracle[route] = max(worst_oracle.get(route, 0.0), ro)
            assert pm.K[route] < pm.count_bound(c.nxs), (route, name)
    for n in pm.SINE_LENGTHS:
        ref = pm.sine_reference(n)
        r = float(pm.ratios(pm.sine_restatement(n), ref["hi"], ref["lo"], ref["S"]).max())
        worst["sine"] = max(worst.get("sine", 0.0), r)
        assert pm.K["sine"] < pm.count_bound(n)
    print({k: round(v, 4) for k, v in worst.items()})
    print("uniform grid", uniform)
    print("oracle", {k: round(v, 4) for k, v in worst_oracle.items()})
    assert set(worst) == set(pm.K)
    for route, r in worst.items():
        assert pm.K[route] / 16 < r <= pm.K[route] / 4, (route, r, pm.K[route])
    for route, r in worst_oracle.items():
        assert r <= pm.K[route], (route, r)


def test_every_row_set_hits_what_it_claims():
    assert tuple(pm.CASES) == pm.CASE_NAMES
    claimed = 0
    for c in pm.CASES.values():
        nz, nm = c.shape
        assert nz == 2 and nz * nm <= 8 and c.ks.size in (pm.NK2, c.nxs // 2)
        missing = set(c.claims) - pm.claims_hit(c)
        assert not missing, (c.name, missing)
        claimed += len(c.claims)
    assert claimed > 60
    # the edges by name: the 2500 plan's lead3 edge with the sample at equality, both sides of its pruned edge
    c = pm.CASES["spec2500-gas-T2"]
    xs = c.xs
    assert pm.plan_radices(2500) == (4, 5, 5, 5, 5) and pm.plan_radices(7) == () and pm.plan_radices(3500) == ()
    kept = [int(np.count_nonzero(pm.kept(xs, v))) for v in c.cmax.ravel()]
    assert kept[:5] == [749, 750, 750, 1250, 1251] and kept[-1] == 5000
    pr = [pm.input_predicates(xs, v, 5000) for v in c.cmax.ravel()]
    assert [p["lead3"] for p in pr[:5]] == [True, True, True, False, False]
    assert [p["pruned"] for p in pr[:5]] == [True, True, True, True, False]
    # long grids: the support fits a compiled sub-transform; chirp rows need <= 590 modes; the band rows fill the grid
    for name, lp in (("pruned30000-T2", 1000), ("pruned25000-T2", 1250), ("pruned10000-T1", 1000)):
        c = pm.CASES[name]
        assert max((int(np.count_nonzero(pm.kept(c.xs, v))) + 1) // 2 for v in c.cmax.ravel()) <= lp
    c = pm.CASES["band30000-T2"]
    jn = [pm.output_predicates(c.kts, c.rss[i, 0], c.zs[i], c.ks, c.nxs, True)["jn"] for i in range(2)]
    assert max(2 * j + 2 for j in jn) <= 1000 and np.all(c.cmax >= c.xs[-1])
    # T2 starts its odd rows off a 16-byte boundary
    assert pm.NK2 % 2 == 1


def test_fills_and_ties_match_numpy():
    """Equality at cmax keeps the sample (np.where(|x| > cmax, 0, 1)); a target at fl(kout_1), one ulp to either side of it,
    at fl(kout_M) and one ulp beyond: the model takes np.interp's side of every tie."""
    xs, kts = pm._grid(16, 20.0)
    assert np.array_equal(pm.kept(xs, xs[5]), np.where(np.abs(xs) > xs[5], 0, 1).astype(bool))
    assert int(np.count_nonzero(pm.kept(xs, xs[5]))) == 6 and int(np.count_nonzero(pm.kept(xs, pm._below(xs[5])))) == 5
    rng = np.random.default_rng(3)
    rss, zs = np.array([[0.7], [1.9]]), np.array([0.25, 1.5])
    for nxs in (16, 45):                   # (odd length: the last mode is not zero, the right fill is a jump)
        xs, kts = pm._grid(nxs, 20.0)
        M = nxs // 2
        kf = pm.kout_float(kts, rss[1, 0], zs[1])
        ks = np.array([0.5 * kf[1], pm._below(kf[1]), kf[1], pm._above(kf[1]), kf[3], pm._below(kf[M]), kf[M],
                       pm._above(kf[M]), 2 * kf[M]])
        c = pm.Case(name="ties", route="table", nxs=nxs, xmax=20.0, cmax=np.array([[xs[5]], [xs[nxs - 3]]]), rss=rss, zs=zs,
                    ks=ks, hints=False, table=rng.uniform(0.1, 1.0, (1, nxs)), do_norm=1)
        ref = pm.reference(c)
        out, c1 = pm.restatement(c)
        assert float(pm.ratios(out, ref["hi"], ref["lo"], ref["S"]).max()) <= pm.K["table"]
        row = ref["hi"][1, 0]
        assert row[0] == row[1] == ref["u1hi"][1, 0] and out[1, 0, 2] == c1[1, 0]
        # (at fl(kout_1) itself the model interpolates from the exact kout_1: u_1 but for the rounding of kout_1)
        assert abs(row[2] - ref["u1hi"][1, 0]) <= pm.EPS * ref["S"][1, 0, 2]
        assert row[7] == 0.0 and row[8] == 0.0 and np.all(ref["S"][1, 0, 7:] == 0) and np.all(out[1, 0, 7:] == 0)
        assert ref["S"][1, 0, 6] > 0                                      # at fl(kout_M): still interpolated
        if nxs % 2 == 0:                                                  # u_M = 0: nothing but the rounding of kout_M
            assert abs(row[6]) <= pm.EPS * ref["S"][1, 0, 6]
        # a wrong value beyond the last mode has no tolerance at all
        assert np.isinf(pm.ratios(np.array([1e-300]), np.zeros(1), np.zeros(1), np.zeros(1))[0])
