"""Series deferral of the analytic NFW tensor (include/hmgrid.h: hmg_prefix_deferral).

Under deferral the NFW rows of the tensor-group launch leave the whole HMG_PREFIX_TILE-wide tiles of every row's
short-series band ((1+c) x <= 0.8) unwritten; the batched mass integrals evaluate the same device function for those
tiles instead of loading them, and every other native reader has them filled first.  The tests poison the NFW buffer
with NaN before the pass, so a deferred byte that anybody reads shows, and compare bit for bit (the same instruction
sequence runs on both sides) with a model that writes its tensors whole (prefix_deferral off).

The mass integrals substitute in every launch shape.  Left alone, the small grids here all run in the thin-slab shape
(16 wavefronts, 64-k tiles), so the shape is also forced (HMG_PB_THIN: "0" 8 wavefronts, "3" 16 wavefronts with 128-k
tiles); the summation order is the same in all of them, so one reference per grid serves every shape."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PAIRS = [("nfw", "nfw"), ("electron", "electron"), ("g", "g"), ("nfw", "electron"), ("g", "nfw"), ("g", "electron")]
MS = np.geomspace(2e10, 1e17, 70)        # crosses a 64-mass tile, leaves a remainder in the 16 virtual slices
ZS3 = np.linspace(0.1, 2.5, 3)
KS_A = np.geomspace(1e-4, 50, 300)
GRIDS = {
    "a": (ZS3, KS_A),                                    # rows with 0, 1, 2 whole deferred tiles, ragged last tile
    "b256": (ZS3, np.geomspace(1e-6, 1e-3, 256)),        # whole rows in the band, nser == nk a multiple of 128
    "b200": (ZS3, np.geomspace(1e-6, 1e-3, 200)),        # ... and not
    "c": (ZS3, np.geomspace(20, 100, 130)),              # nothing in the band
    "d": (ZS3, np.geomspace(1e-4, 50, 257)),             # odd nk: the one-wavenumber-per-lane instantiation
    "e": (ZS3[:1], KS_A),                                      # nz = 1
}


def build(monkeypatch, defer, zs, ks, shape="0"):
    import hmvec_amd as hm
    monkeypatch.delenv("HMG_NO_HINTS", raising=False)
    monkeypatch.setenv("HMG_NO_GROUPS", "0")
    monkeypatch.setenv("HMG_NO_PREFIX_DEFERRAL", "0" if defer else "1")
    if shape is None:
        monkeypatch.delenv("HMG_PB_THIN", raising=False)
    else:
        monkeypatch.setenv("HMG_PB_THIN", shape)
    h = hm.HaloModel(zs, ks, ms=MS, accuracy="low", engine="analytic")
    assert h.prefix_deferral == defer
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


def same(got, want):
    assert len(got) == len(want) == 12
    for p, a, b in zip(PAIRS + PAIRS, got, want):
        assert np.all(np.isfinite(a)), p
        assert np.array_equal(a, b), p


_REF = {}


def reference(monkeypatch, grid):
    """The non-deferring model of a grid, its spectra and its NFW tensor: computed once, shared, never changed."""
    if grid not in _REF:
        zs, ks = GRIDS[grid]
        ref = build(monkeypatch, False, zs, ks, None)
        _REF[grid] = (ref, spectra(ref), ref.uk_profiles["nfw"].copy())
    return _REF[grid]


@pytest.mark.parametrize("grid,shape", [(g, s) for g in GRIDS for s in (None, "0")] + [("a", "3")])
def test_batched_spectra_and_filled_tensor_equal_the_whole_tensor(monkeypatch, grid, shape):
    """Checks 1, 2 and 3."""
    zs, ks = GRIDS[grid]
    ref, want, want_t = reference(monkeypatch, grid)
    assert pending(ref) == 0
    h = build(monkeypatch, True, zs, ks, shape)
    poison(h)
    assert pending(h) == 0                       # the host's values replaced the tensor: nothing to substitute
    step(h)
    same(spectra(h), want)
    assert pending(h) == 1                       # the pass deferred, and the mass integrals filled nothing
    full = nfw_dev(h).numpy()                    # a host copy fills first
    assert pending(h) == 0
    assert not np.isnan(full).any()
    assert np.array_equal(full, want_t)
    step(h)
    same(spectra(h), want)
    assert pending(h) == 1
    assert np.array_equal(h.uk_profiles["nfw"], want_t)


def test_one_pair_path_reads_a_filled_tensor(monkeypatch):
    """Check 4: the one-pair kernel reads whole rows (a bias override takes it; so does get_power_1halo)."""
    zs, ks = GRIDS["a"]
    ref, _, _ = reference(monkeypatch, "a")
    b1 = np.linspace(1.0, 2.0, zs.size).reshape(-1, 1)
    want1 = ref.get_power_1halo("nfw", "nfw")
    want2 = ref.get_power_2halo("nfw", "nfw", b1_in=b1, b2_in=b1)
    h = build(monkeypatch, True, zs, ks)
    poison(h)
    step(h)
    got2 = h.get_power_2halo("nfw", "nfw", b1_in=b1, b2_in=b1)
    poison(h)
    step(h)
    got1 = h.get_power_1halo("nfw", "nfw")
    assert np.all(np.isfinite(got1)) and np.all(np.isfinite(got2))
    assert np.array_equal(got1, want1) and np.array_equal(got2, want2)


def test_trispectrum_and_bispectrum_read_a_filled_tensor(monkeypatch):
    """Check 5."""
    zs, ks = GRIDS["a"]
    ref, _, _ = reference(monkeypatch, "a")
    kindex = np.array([0, 40, 130, 299])
    want_t = ref.get_trispectrum_1halo("nfw", kindex=kindex)
    want_b = ref.get_bispectrum("nfw", kindex=kindex)
    h = build(monkeypatch, True, zs, ks)
    poison(h)
    step(h)
    got_t = h.get_trispectrum_1halo("nfw", kindex=kindex)
    poison(h)
    step(h)
    got_b = h.get_bispectrum("nfw", kindex=kindex)
    assert np.all(np.isfinite(got_t)) and np.all(np.isfinite(got_b))
    assert np.array_equal(got_t, want_t) and np.array_equal(got_b, want_b)


def test_captured_step_replays_the_deferral(monkeypatch):
    """Check 6: three replays of the captured step equal the eager pass; the step keeps its 3 kernel nodes."""
    zs, ks = GRIDS["a"]
    _, want, want_t = reference(monkeypatch, "a")
    h = build(monkeypatch, True, zs, ks)
    blk = h.spectra_block(PAIRS)
    ctx = h._ctx()

    def whole():
        step(h)
        blk.compute()

    whole()                                    # eager once: every buffer exists
    gid = ctx.capture(whole)
    assert ctx.graph_kernel_nodes(gid) == 3
    for _ in range(3):
        poison(h)
        ctx.replay(gid)
        assert pending(h) == 1
        got = blk.fetch()
        for i, p in enumerate(PAIRS):
            assert np.array_equal(got[p][0], want[i]) and np.array_equal(got[p][1], want[len(PAIRS) + i]), p
    assert np.array_equal(nfw_dev(h).numpy(), want_t)
    assert pending(h) == 0
    ctx.call("hmg_graph_destroy", gid)


def test_z_slab_equals_the_rows_of_the_full_grid(monkeypatch):
    """Check 7."""
    zs, ks = GRIDS["a"]
    _, want, _ = reference(monkeypatch, "a")
    slab = build(monkeypatch, True, zs[:2], ks)
    got = spectra(slab)
    for p, a, b in zip(PAIRS + PAIRS, got, want):
        assert np.array_equal(a, b[:2]), p


def test_host_values_written_into_the_tensor_are_used(monkeypatch):
    """Check 8: hmg_memcpy_h2d into a tensor with deferred tiles clears its entry - the integrals load the host's ones."""
    zs, ks = GRIDS["a"]
    ref = build(monkeypatch, False, zs, ks)
    ref._ctx().write(nfw_dev(ref), np.ones(nfw_dev(ref).shape))
    want = spectra(ref)
    h = build(monkeypatch, True, zs, ks)
    step(h)                                      # (a model's first pass takes separate launches; from the second on the
    spectra(h)                                   # pass is issued with its mass integrals, on the tensor-group route)
    assert pending(h) == 1
    h._ctx().write(nfw_dev(h), np.ones(nfw_dev(h).shape))
    assert pending(h) == 0
    same(spectra(h), want)
    assert np.array_equal(nfw_dev(h).numpy(), np.ones(nfw_dev(h).shape))
