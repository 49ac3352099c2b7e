"""Row groups of the NFW role in the tensor-group launch (kernels/nfw.hpp: nfw_row_group).

From 24 rows per compute unit on (6144 rows on the 256 units of an MI355X) a workgroup of the role serves two consecutive
rows of the heavy-first order, a sub-group of four wavefronts each, and the last workgroup of a grid with an odd number of
rows is ragged; below that a workgroup serves one row.  Every wavenumber is still evaluated by nfw_rows, so the tensor
must equal the one the stand-alone kernel (hmg_nfw_analytic, one launch per stage) writes, bit for bit - with series
deferral on (after the fill) and off (whole rows written).

Grids: 2 x 5 and 3 x 7 rows (10 and 21: divisible by neither 2 nor 4; one row per workgroup) and 3 x 2049 (6147 rows: the
row groups, the last one with one row), nk = 300 (no multiple of 64, 128 or 512) and 640; k from 0.05 to 5 and masses
from 1e9 to 1e16, so that the light rows lie in the short-series band whole (nser == nk: the row loop has nothing to do)
and the heaviest have fewer than one tile of it (nser < 128: nothing deferred).  The test works the counts out on the
host and asserts that the grid is that wide.

A skipped row shows because the tensor is poisoned with NaN before the pass.  A row served twice means another row is
skipped (there are as many sub-groups as rows).  A count that was not written shows in
test_every_count_is_rewritten_by_the_pass: the pass before it runs with the wavenumbers scaled down until every count
is nk, so a stale count makes the fill overwrite a whole row with short-series values."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PAIRS = [("nfw", "nfw"), ("electron", "electron"), ("g", "g"), ("nfw", "electron"), ("g", "nfw"), ("g", "electron")]
TILE = 128                      # HMG_PREFIX_TILE
XS2 = 0.8                       # NFW_XS2: (1+c) x below this takes a short form of the series
SHAPES = {"2x5": (2, 5), "3x7": (3, 7), "3x2049": (3, 2049)}


def grid(shape, nk):
    nz, nm = SHAPES[shape]
    return np.linspace(0.0, 0.5, nz), np.geomspace(1e9, 1e16, nm), np.geomspace(0.05, 5.0, nk)


def build(monkeypatch, grouped, defer, zs, ms, ks):
    import hmvec_amd as hm
    monkeypatch.delenv("HMG_NO_HINTS", raising=False)
    monkeypatch.delenv("HMG_PB_THIN", raising=False)
    monkeypatch.setenv("HMG_NO_GROUPS", "0" if grouped else "1")
    monkeypatch.setenv("HMG_NO_PREFIX_DEFERRAL", "0" if defer else "1")
    h = hm.HaloModel(zs, ks, ms=ms, accuracy="low", engine="analytic")
    assert h._groups == grouped and h.prefix_deferral == defer
    step(h)
    return h


def step(h):
    """One pass of the facade up to (not including) the spectra; buffers are reused from the second call on."""
    h.init_mass_function(h.ms)
    h.add_nfw_profile("nfw", ignore_existing=True)
    h.add_battaglia_profile("electron", family="AGN", xmax=20, nxs=1000, ignore_existing=True)
    h.add_hod("g", mthresh=10 ** 10.5 + h.zs * 0.0, ignore_existing=True)


def nfw_dev(h):
    return h.uk_profiles.dev("nfw", fill=False)


def poison(h):
    d = nfw_dev(h)
    h._ctx().write(d, np.full(d.shape, np.nan))


def pending(h):
    ctx = h._ctx()
    ctx.flush()
    n = C.c_int()
    assert ctx.lib.hmg_prefix_pending(ctx.handle, nfw_dev(h).ptr, C.byref(n)) == 0
    return n.value


def spectra(h):
    o1, o2 = h.power_device_batch(PAIRS)
    return [a.numpy() for a in o1] + [a.numpy() for a in o2]


def series_counts(h):
    """nser of every row as nfw_series_count defines it: the k with opc * (ks[k] * rs * z1) <= 0.8, in that order of operations."""
    cs, rs = h._d_cs.numpy().reshape(h.zs.size, -1), h._d_rs.numpy().reshape(h.zs.size, -1)
    z1 = (1.0 + h.zs)[:, None, None]
    xc = (1.0 + cs)[:, :, None] * (h.ks[None, None, :] * rs[:, :, None] * z1)
    return np.where(cs >= 0.5, (xc <= XS2).sum(axis=-1), 0)


_REF = {}


def reference(monkeypatch, shape, nk):
    """The model with one launch per stage (the stand-alone NFW kernel), its spectra and its NFW tensor: once per grid."""
    if (shape, nk) not in _REF:
        ref = build(monkeypatch, False, False, *grid(shape, nk))
        _REF[shape, nk] = (spectra(ref), ref.uk_profiles["nfw"].copy(), series_counts(ref))
    return _REF[shape, nk]


def same(got, want):
    assert len(got) == len(want) == 12
    for p, a, b in zip(PAIRS + PAIRS, got, want):
        assert np.all(np.isfinite(a)), p
        assert np.array_equal(a, b), p


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("nk", [300, 640])
def test_the_grid_reaches_both_ends_of_the_band(default_routes, shape, nk):
    _, want_t, cnt = reference(default_routes, shape, nk)
    assert np.all(np.isfinite(want_t))
    assert cnt.max() == nk                                  # light rows: the whole row is in the band
    assert 0 < cnt.min() < TILE                             # heaviest rows: in the band, but no whole tile of it
    assert np.unique(cnt // TILE).size >= 3                 # and rows with different numbers of deferred tiles between


@pytest.mark.parametrize("defer", [True, False])
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("nk", [300, 640])
def test_grouped_rows_equal_the_stand_alone_kernel(default_routes, shape, nk, defer):
    """Ragged last workgroup, deferral on and off: tensor (after the fill) and spectra, bit for bit."""
    want, want_t, _ = reference(default_routes, shape, nk)
    h = build(default_routes, True, defer, *grid(shape, nk))
    poison(h)
    step(h)
    same(spectra(h), want)
    assert pending(h) == (1 if defer else 0)                # the tensor-group route ran, and deferred or not as asked
    full = nfw_dev(h).numpy()                               # a host copy fills first (hmg_prefix_fill)
    assert pending(h) == 0
    assert not np.isnan(full).any()
    assert np.array_equal(full, want_t)


@pytest.mark.parametrize("shape,nk", [("3x7", 300), ("3x2049", 300)])
def test_every_count_is_rewritten_by_the_pass(default_routes, shape, nk):
    """The counts of a pass replace those of the pass before, row by row: the earlier pass has nser == nk everywhere."""
    want, want_t, _ = reference(default_routes, shape, nk)
    zs, ms, ks = grid(shape, nk)
    h = build(default_routes, True, True, zs, ms, ks)
    ctx = h._ctx()
    ctx.write(h._d_ks(), ks * 1e-6)
    step(h)
    spectra(h)
    assert pending(h) == 1
    small = nfw_dev(h).numpy()
    assert np.all(np.isfinite(small)) and not np.array_equal(small, want_t)
    ctx.write(h._d_ks(), ks)
    poison(h)
    step(h)
    same(spectra(h), want)
    assert pending(h) == 1
    assert np.array_equal(nfw_dev(h).numpy(), want_t)


def test_default_context_through_the_facade(default_routes):
    """2 x 5 x 300 under the environment as it is but for the route pins: the six spectra of a grouped pass equal those of
    the pass with one launch per stage, and so does the tensor a host read gets."""
    zs, ms, ks = grid("2x5", 300)
    want, want_t, _ = reference(default_routes, "2x5", 300)
    import hmvec_amd as hm
    default_routes.delenv("HMG_NO_GROUPS", raising=False)
    default_routes.delenv("HMG_NO_PREFIX_DEFERRAL", raising=False)
    h = hm.HaloModel(zs, ks, ms=ms, accuracy="low", engine="analytic")
    for _ in range(2):                                      # (the second pass is the one issued as front | tensor group | integrals)
        step(h)
        same(spectra(h), want)
    assert np.array_equal(h.uk_profiles["nfw"], want_t)
    for (a, b), p1, p2 in zip(PAIRS, want[:6], want[6:]):
        assert np.array_equal(h.get_power_1halo(a, b), p1) and np.array_equal(h.get_power_2halo(a, b), p2), (a, b)
