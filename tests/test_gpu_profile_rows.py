"""Every route of hmg_profile_fft, hmg_profile_fft_table and hmg_sine_transform against the 40-digit discrete reference
of helpers/profile_model.py:  |out - ref| <= K[route] 2^-52 S(k) |post|  at every point, exact
zeros beyond the last mode, the hint arrays within the same gate, the reversed target grid without hints within it.

The entry points are called directly through hmvec_amd._native.  Every test also shows that it ran the route it
names: a second context with that route's switch off must give other last bits (for the lengths only rocFFT takes: the
same bits), so a call that silently fell back to rocFFT fails its test instead of passing under the wrong name.  The
off-route output is the rocFFT route's (or, for the chirp rows, the pruned decomposition's) and is held to that
route's own K.

A "-T3" grid (its T2 reversed, no hint arrays: the per-target path; for the table entry point, which takes no hints,
the same targets descending) runs inside its T2's test in a context with the same switches; it takes no switch-off
proof of its own - its T2 has given it - and must sit inside the gate itself and within the gate of T2 reversed.

Each test prints its worst ratio / K.  Measured on an MI355X, worst ratio per route (K): spec2500 0.294 (0.876), ct 0.264
(0.600), rt 0.307 (0.628), pruned 0.271 (0.792), chirp 0.176 (0.552), band 0.089 (0.196), rocfft 0.259 (1.040), table
1.720 (3.932), sine 0.681 (2.140).  The table rows' 1.72 is the one-row kernels' mode grid j k_lo on T1, whose targets
all sit on knots of a non-smooth spectrum: the numpy restatement of that grid has 1.72 there too.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import profile_model as pm  # noqa: E402

pytestmark = pytest.mark.gpu


def _context(monkeypatch, switches):
    """A context under the default routes (the `default_routes` fixture has cleared every switch) plus `switches`."""
    from conftest import ROUTE_SWITCHES
    from hmvec_amd import _native as nat
    assert all(k in ROUTE_SWITCHES for k in switches)
    for sw in ROUTE_SWITCHES:
        monkeypatch.delenv(sw, raising=False)
    for k, v in switches.items():
        monkeypatch.setenv(k, v)
    return nat.Context(0)                     # the switches are read when a context is created


def _run(ctx, case):
    """(out (nz, nm, nk), nconst or None, cconst or None) of one call of the entry point the case names."""
    nz, nm = case.shape
    rows, nk, nxs = nz * nm, case.ks.size, case.nxs
    up = lambda a: None if a is None else ctx.upload(np.asarray(a, dtype=np.float64))
    d_xs, d_kts = up(case.xs), up(case.kts)
    d_cmax, d_rss, d_zs, d_ks = up(case.cmax), up(case.rss), up(case.zs), up(case.ks)
    out = ctx.empty((nz, nm, nk))
    ctx.write(out, np.full((nz, nm, nk), np.nan))
    p = lambda d: None if d is None else d.ptr
    if case.table is not None:
        d_tab = up(case.table)
        ctx.call("hmg_profile_fft_table", nz, nm, nk, nxs, case.step, d_xs.ptr, d_kts.ptr, d_tab.ptr,
                 int(case.table.shape[0]), d_cmax.ptr, d_rss.ptr, d_zs.ptr, d_ks.ptr, int(case.do_norm), out.ptr)
        return out.numpy(), None, None
    d_amp, d_xc, d_al, d_ex, d_post = up(case.amp), up(case.xc), up(case.alpha), up(case.expo), up(case.post)
    d_n = ctx.empty(((rows + 1) // 2,)) if case.hints else None
    d_c = ctx.empty((rows,)) if case.hints else None
    d_lx = None
    if case.logx:
        d_lx = ctx.empty((nxs,))
        ctx.call("hmg_profile_fft_logx", nxs, d_xs.ptr, d_lx.ptr)
    ctx.call("hmg_profile_fft", nz, nm, nk, nxs, case.step, d_xs.ptr, d_kts.ptr, p(d_amp), p(d_xc), p(d_al), p(d_ex),
             float(case.amp_c), float(case.xc_c), float(case.alpha_c), float(case.expo_c), float(case.gamma),
             d_cmax.ptr, d_rss.ptr, d_zs.ptr, d_ks.ptr, int(case.do_norm), p(d_post), out.ptr, p(d_n), p(d_c), p(d_lx))
    got = out.numpy()
    if not case.hints:
        return got, None, None
    return got, d_n.numpy().view(np.int32)[:rows].reshape(nz, nm).copy(), d_c.numpy().reshape(nz, nm)


def _gate(case, got, cconst, K, what):
    ref = pm.reference(case)
    assert np.all(np.isfinite(got)), what
    r = pm.ratios(got, ref["hi"], ref["lo"], ref["S"])
    beyond = ref["S"] == 0
    assert np.all(got[beyond] == 0.0), (what, "non-zero beyond the last mode")
    worst = float(r.max())
    if cconst is not None:
        worst = max(worst, float(pm.ratios(cconst, ref["u1hi"], ref["u1lo"], ref["S1"]).max()))
    print(f"{what}: worst ratio {worst:.3f}  / K = {worst / K:.3f}  (K = {K}, {got.size} points, {int(beyond.sum())} beyond)")
    assert K < pm.count_bound(case.nxs)
    assert worst <= K, (what, worst, K, np.unravel_index(np.argmax(r), r.shape))
    return worst


ROUTE_CASES = [n for n in pm.CASE_NAMES if not n.endswith("-T3")]      # (a T3 grid runs inside its T2 test)


@pytest.mark.parametrize("name", ROUTE_CASES)
def test_route_against_the_discrete_reference(default_routes, name):
    monkeypatch = default_routes
    case = pm.CASES[name]
    K = pm.K[case.route]
    ctx = _context(monkeypatch, case.env)
    got, nconst, cconst = _run(ctx, case)
    _gate(case, got, cconst, K, f"{name} [{case.route}]")
    if nconst is not None:      # the prefix the hints describe holds the left-fill value, bit for bit
        nz, nm = case.shape
        for i in range(nz):
            for j in range(nm):
                assert np.all(got[i, j, :nconst[i, j]] == cconst[i, j])
    ctx.close()
    # the route: the same call in a context with the route's switch off
    ctx_off = _context(monkeypatch, case.off)
    other, _, c_off = _run(ctx_off, case)
    ctx_off.close()
    if case.off_equal:
        assert np.array_equal(other, got), "this length has one route: rocFFT"
    else:
        assert not np.array_equal(other, got), f"{name}: the {case.route} route did not take the call"
        off_route = "pruned" if case.route == "chirp" else "table" if case.table is not None else "rocfft"
        _gate(case, other, c_off, pm.K[off_route], f"{name} [switch off: {off_route}]")
    # T3: the reversed grid without hint arrays, the per-target path, on the same route
    t3 = pm.CASES.get(name[:-3] + "-T3") if name.endswith("-T2") else None
    if t3 is not None:
        ctx3 = _context(monkeypatch, case.env)
        back, _, _ = _run(ctx3, t3)
        ctx3.close()
        ref = pm.reference(case)
        rev = back[..., ::-1]
        r = pm.ratios(rev, ref["hi"], ref["lo"], ref["S"])
        # without hints the long-grid rows cannot bound the modes they need: every row takes the decomposition
        K3 = pm.K["pruned" if case.route == "chirp" else case.route]
        print(f"{t3.name}: worst ratio {float(r.max()):.3f} / K = {float(r.max()) / K3:.3f}")
        assert np.all(np.isfinite(back)) and r.max() <= K3, (t3.name, float(r.max()))
        assert np.all(rev[ref["S"] == 0] == 0.0)
        assert np.all(np.abs(rev - got) <= max(K, K3) * pm.EPS * ref["S"])


@pytest.mark.parametrize("n", pm.SINE_LENGTHS)
def test_sine_transform_against_the_discrete_reference(n):
    from hmvec_amd import _native as nat
    ctx = nat.Context(0)
    x, y = pm.sine_rows(n)
    d_x, d_y = ctx.upload(x), ctx.upload(y)
    out = ctx.empty((2, n // 2 + 1))
    ctx.write(out, np.full((2, n // 2 + 1), np.nan))
    ctx.call("hmg_sine_transform", 2, n, d_x.ptr, d_y.ptr, out.ptr)
    got = out.numpy()
    ctx.close()
    ref = pm.sine_reference(n)
    assert np.all(np.isfinite(got))
    r = pm.ratios(got, ref["hi"], ref["lo"], ref["S"])
    K = pm.K["sine"]
    print(f"hmg_sine_transform n = {n}: worst ratio {float(r.max()):.3f} / K = {float(r.max()) / K:.3f}")
    assert K < pm.count_bound(n) and r.max() <= K
