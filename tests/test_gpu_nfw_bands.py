"""GPU checks of the analytic NFW kernel (hmg_nfw_analytic -> nfw_rows, hmvec_amd/csrc/kernels/nfw.hpp) form by form
against the closed form at 40 digits.  The gate is relative where u is small - |u_gpu - u_mpmath| <= K[band] B with
B = 2^-52 (|u| + |x du/dx| + |c du/dc|), in the closed band K S with S the size of the terms that form subtracts - and
every number in it comes from the reference side (helpers/nfw_model.py; tests/test_nfw_cpu.py checks it without a
device).  The 1e-12 absolute gate against the float64 oracle that the rest of the suite uses cannot tell a wrong
coefficient of the asymptotic series or of the 32-term tail from rounding; this one can.

Measured on an MI355X with the kernel as it stands - nfw_series_row taking the low moments of rows with c < 1.5 from
quadrature - (worst |u_gpu - u_mpmath| / unit per band over the point set, as test_each_band_against_mpmath prints it):
    s5         0.2498   (K = 8, 234 points)
    s8         0.2494   (K = 8, 85 points)
    s16        0.4516   (K = 8, 70 points)
    s32         31.15   (K = 104, 80 points)
    col<8       101.7   (K = 368, 34 points)
    col<64       81.1   (K = 353, 104 points)
    col≥64      25.34   (K = 102, 720 points)
    mixed        18.5   (K = 105, 62 points)
    closed      2.594   (K = 25, 224 points)
and 0.39 S over the 20 points with xc >= 1e9.  With the forward recurrence alone (before the quadrature) the same run
gave s5 0.2498, s8 0.285, s16 0.8439, s32 31.15 - the series bands are the only ones the coefficients enter, and their
worst s8 and s16 points were at c = 0.5 - and the other five bands the same figures.  The restatement's own figures are
in helpers/nfw_model.py.
"""
import os
import sys

import numpy as np
import pytest

from hmvec_amd import _native as nat

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import nfw_model as nm  # noqa: E402

pytestmark = pytest.mark.gpu


def nfw(cs, rss, zs, ks, series=None):
    """u[nz, nm, nk] of hmg_nfw_analytic; series: the rows of hmg_halo_stage, or None to let the call build them."""
    cs, rss = np.atleast_2d(cs), np.atleast_2d(rss)
    (nz, nm), nk = cs.shape, len(ks)
    assert rss.shape == (nz, nm) and len(zs) == nz
    ctx = nat.Context(0)
    d_cs, d_rs, d_zs, d_ks = (ctx.upload(a) for a in (cs, rss, zs, ks))
    d_ser = None if series is None else ctx.upload(series)
    out = ctx.empty((nz, nm, nk))
    ctx.call("hmg_nfw_analytic", nz, nm, nk, d_cs.ptr, d_rs.ptr, d_zs.ptr, d_ks.ptr,
             None if d_ser is None else d_ser.ptr, out.ptr)
    u = out.numpy()
    ctx.close()
    return u


@pytest.fixture(scope="module")
def tab():
    return nm.table()


@pytest.fixture(scope="module")
def on_the_set(tab):
    """The kernel at every point of the set: one row per concentration, rs = 1 and z = 0 so that x is ks[k] itself,
    ks the sorted union of the set's x."""
    cs, ks = np.array(nm.CS), np.unique(tab.x)
    u = nfw(cs[None, :], np.ones((1, len(cs))), np.zeros(1), ks)
    assert np.array_equal(ks * 1.0 * (1.0 + 0.0), ks)
    return u[0, np.searchsorted(cs, tab.c), np.searchsorted(ks, tab.x)]


def test_each_band_against_mpmath(tab, on_the_set):
    worst = tab.worst(on_the_set)
    for b in nm.BANDS:
        print(f"    {b:7s} {worst[b]:9.4g}   (K = {nm.K[b]}, {int(np.sum(tab.band == b))} points)")
    assert np.all(np.isfinite(on_the_set))
    bad = [b for b in nm.BANDS if not worst[b] <= nm.K[b]]
    assert not bad, {b: worst[b] for b in bad}


def test_rows_and_redshifts_land_where_they_belong():
    """Three redshifts, five masses with a (c, rs) of their own each, 4100 wavenumbers: two k tiles, the second with four
    points; rows of 4100 doubles start off a 16-byte boundary; workgroups take the masses of a redshift in reverse
    (row_order), so the row a workgroup reads and writes is not the one its index names.  A row, redshift or tile taken
    for another misses by many orders of K.  (row_order itself is only a dispatch order: with the identity in its place
    the results are the same bits, and this test passes - as it should.)"""
    nz, nm_, nk = 3, 5, 4100
    zs = np.array([0.0, 0.7, 2.5])
    cs = np.array([0.3, 0.8, 1.9, 3.1, 4.4, 5.7, 7.3, 9.0, 12.0, 17.0, 26.0, 41.0, 0.45, 63.0, 95.0]).reshape(nz, nm_)
    rss = np.geomspace(0.004, 3.0, nz * nm_)[::-1].reshape(nz, nm_).copy()
    ks = np.geomspace(1e-4, 3e3, nk)
    u = nfw(cs, rss, zs, ks)
    assert np.all(np.isfinite(u))
    pick = np.unique(np.concatenate([[0, 4095, 4096, 4099], np.linspace(1, 4098, 60).astype(int)]))
    assert len(pick) == 64
    hit = set()
    for z in range(nz):
        for m in range(nm_):
            x = ks[pick] * rss[z, m] * (1.0 + zs[z])
            ref, gate, bd = nm.reference(np.full(len(pick), cs[z, m]), x)
            err = nm.table().err(u[z, m, pick], ref)
            hit |= set(bd)
            assert np.all(err <= gate), (z, m, pick[err > gate], (err / gate).max())
    assert hit == set(nm.BANDS), hit


def test_series_flag_edge(tab):
    """c = 0.5 is the first row whose series is on, the double below it the last that takes the closed form for x <= 4.
    u is continuous in c: the two rows stay within their own gates and within the larger of the two of each other."""
    at = tab.c == 0.5
    ks = tab.x[at]
    below = float(np.nextafter(0.5, 0.0))
    u = nfw(np.array([[0.5, below]]), np.ones((1, 2)), np.zeros(1), ks)[0]
    ref, gate, bd = nm.reference(np.full(len(ks), below), ks)
    gate_on = tab.K[at] * tab.unit[at]
    series = {"s5", "s8", "s16", "s32"}
    assert set(tab.band[at][1.5 * ks <= 10.0]) == series and not series & set(tab.band[at][1.5 * ks > 10.0])
    assert set(bd[ks <= 4.0]) == {"closed"} and set(bd[ks > 4.0]) == {"col<8", "col<64", "col≥64"}
    assert np.all(tab.err(u[0], [r for r, a in zip(tab.u, at) if a]) <= gate_on)
    assert np.all(tab.err(u[1], ref) <= gate)
    assert np.all(np.abs(u[0] - u[1]) <= np.maximum(gate_on, gate))


def test_beyond_the_cody_waite_range(tab, on_the_set):
    """xc >= 1e9 leaves sincos_fast's reduction for the library's: finite, and within the closed form's gate."""
    far = (1.0 + tab.c) * tab.x >= 1e9
    assert far.sum() >= 3 and np.all(tab.band[far] == "closed")
    assert np.all(np.isfinite(on_the_set[far]))
    ratio = tab.err(on_the_set)[far] / tab.S[far]
    print(f"xc >= 1e9: {far.sum()} points, worst |u_gpu - u_mpmath| / S = {ratio.max():.4g}")
    assert np.all(ratio <= nm.K["closed"])


def test_series_row_from_the_halo_stage_gives_the_same_bits():
    """hmgrid.h: the series rows of hmg_halo_stage and the ones hmg_nfw_analytic builds for itself are interchangeable."""
    import hmvec_amd as hm
    zs, ms = np.array([0.1, 1.3, 3.0]), np.geomspace(1e10, 3e16, 11)
    h = hm.HaloModel(zs, np.geomspace(1e-3, 30, 17), ms=ms, accuracy="low", engine="analytic")
    cs, rss, series = h._d_cs.numpy(), h._d_rs.numpy(), h._d_nfw_series.numpy()
    assert series.shape == (3, 11, nat.NFW_SERIES_STRIDE)
    ks = np.geomspace(1e-5, 1e6, 777)
    x = ks[None, None, :] * rss[..., None] * (1.0 + zs[:, None, None])
    # every form that a model's rows reach: the closed one and col<8 need c < 0.5 and c < 1, below Duffy's concentrations
    assert {nm.BANDS[i] for i in np.unique(nm.bands(cs[..., None], x))} == set(nm.BANDS) - {"closed", "col<8"}
    own, brought = nfw(cs, rss, zs, ks), nfw(cs, rss, zs, ks, series)
    assert np.all(np.isfinite(own)) and np.array_equal(own, brought)
