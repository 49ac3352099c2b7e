"""Deferred left fill of the hinted profile tensors (include/hmgrid.h: hmg_prefix_deferral).

A pass of the facade leaves the whole HMG_PREFIX_TILE-wide tiles of every row's constant prefix unwritten: the batched
mass integrals never load them, every other reader has them filled first.  The tests poison the tensor buffers with NaN
before the pass, so a deferred byte that anybody reads shows, and compare bit for bit with a model that writes its
tensors whole (prefix_deferral off)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TILE = 128      # HMG_PREFIX_TILE
PAIRS = [("nfw", "nfw"), ("electron", "electron"), ("g", "g"), ("nfw", "electron"), ("g", "nfw"), ("g", "electron")]


def build(monkeypatch, defer, zs, ms, ks, nxs=1000, central=None, pressure=False, groups=True):
    import hmvec_amd as hm
    monkeypatch.delenv("HMG_NO_HINTS", raising=False)
    monkeypatch.setenv("HMG_NO_GROUPS", "0" if groups else "1")
    monkeypatch.setenv("HMG_NO_PREFIX_DEFERRAL", "0" if defer else "1")
    h = hm.HaloModel(zs, ks, ms=ms, accuracy="low", engine="analytic")
    assert h.prefix_deferral == defer
    h._test_args = dict(nxs=nxs, central=central, pressure=pressure)
    step(h)
    return h


def step(h):
    """One pass of the facade up to (not including) the spectra; buffers are reused from the second call on."""
    a = h._test_args
    zs = h.zs
    h.init_mass_function(h.ms)
    h.add_nfw_profile("nfw", ignore_existing=True)
    h.add_battaglia_profile("electron", family="AGN", xmax=20, nxs=a["nxs"], ignore_existing=True)
    if a["pressure"]:
        h.add_battaglia_pres_profile("y", family="pres", xmax=5, nxs=a["nxs"], ignore_existing=True)
    h.add_hod("g", mthresh=10 ** 10.5 + zs * 0.0, central_profile_name=a["central"], ignore_existing=True)


def poison(h):
    ctx = h._ctx()
    for dd, name in ((h.uk_profiles, "electron"), (h.pk_profiles, "y")):
        if name in dd:
            d = dd.dev(name, fill=False)
            ctx.write(d, np.full(d.shape, np.nan))


def hints(dd, name, rows):
    n, c = dd.hint(name)
    return n.numpy().view(np.int32)[:rows].copy(), c.numpy().reshape(-1)


def spectra(h):
    o1, o2 = h.power_device_batch(PAIRS)
    return [a.numpy() for a in o1] + [a.numpy() for a in o2]


def check_pass(monkeypatch, zs, ms, ks, **kw):
    """Checks 1 and 2 of the issue on one grid; returns the deferring model."""
    ref = build(monkeypatch, False, zs, ms, ks, **kw)
    want = spectra(ref)
    h = build(monkeypatch, True, zs, ms, ks, **kw)
    poison(h)
    step(h)
    got = spectra(h)
    assert len(got) == 12
    for p, a, b in zip(PAIRS + PAIRS, got, want):
        assert np.all(np.isfinite(a)), p
        assert np.array_equal(a, b), p
    rows = zs.size * ms.size
    for dd, rd, name in ((h.uk_profiles, ref.uk_profiles, "electron"), (h.pk_profiles, ref.pk_profiles, "y")):
        if name not in dd:
            continue
        n, _ = hints(dd, name, rows)
        # the pass really left the tiles alone: the poison is still there, in exactly the deferred elements
        raw = dd.dev(name, fill=False).numpy().reshape(rows, ks.size)
        print(f"{name}: {int(np.isnan(raw).sum())} deferred elements of {raw.size}, hint sum {int((n & ~(TILE - 1)).sum())}")
        assert dd._pending(name)
        assert int(np.isnan(raw).sum()) == int((n & ~(TILE - 1)).sum())
        full = dd[name]                                   # a host read fills first
        assert not dd._pending(name)
        assert not np.isnan(full).any()
        assert np.array_equal(full, rd[name]), name
    return h, ref


@pytest.mark.parametrize("nz,nm,nk,central", [(3, 96, 512, None),            # even nk: 128-wide k tiles
                                              (3, 96, 515, None),            # odd nk: 64-wide k tiles, ragged last tile
                                              (2, 64, 384, "electron"),      # HOD with a (hinted) central profile
                                              (4, 512, 4096, None)])         # thin slab: the 16-wavefront shape
def test_batched_spectra_never_read_a_deferred_byte(monkeypatch, nz, nm, nk, central):
    zs = np.linspace(0.1, 2.5, nz)
    ms = np.geomspace(2e10, 1e17, nm)
    ks = np.geomspace(1e-4, 100, nk)
    h, _ = check_pass(monkeypatch, zs, ms, ks, central=central, pressure=(nz == 3))
    n, _ = hints(h.uk_profiles, "electron", nz * nm)
    assert (n & ~(TILE - 1)).sum() > 0          # there was something to defer on this grid


def test_recorded_and_captured_passes_keep_the_pending_state(monkeypatch):
    """Check 3: the pass through Context.trace / run_trace and through capture / replay - poison between two re-issues,
    read after the second."""
    zs = np.linspace(0.1, 2.5, 3)
    ms = np.geomspace(2e10, 1e17, 96)
    ks = np.geomspace(1e-4, 100, 512)
    ref = build(monkeypatch, False, zs, ms, ks)
    want, want_t = spectra(ref), ref.uk_profiles["electron"]
    h = build(monkeypatch, True, zs, ms, ks)
    blk = h.spectra_block(PAIRS)
    ctx = h._ctx()

    def whole():
        step(h)
        blk.compute()

    whole()                                    # eager once: every buffer exists
    calls = ctx.trace(whole)
    gid = ctx.capture(whole)
    for issue in (lambda: ctx.run_trace(calls), lambda: ctx.replay(gid)):
        issue()
        assert h.uk_profiles._pending("electron")
        first = h.uk_profiles["electron"].copy()
        assert not h.uk_profiles._pending("electron")
        poison(h)
        issue()
        assert h.uk_profiles._pending("electron")
        got = blk.fetch()
        for i, p in enumerate(PAIRS):
            assert np.array_equal(got[p][0], want[i]) and np.array_equal(got[p][1], want[len(PAIRS) + i]), p
        second = h.uk_profiles["electron"]       # (the cached host copy must not survive the re-issue)
        assert not np.isnan(second).any()
        assert np.array_equal(first, want_t) and np.array_equal(second, want_t)
    ctx.call("hmg_graph_destroy", gid)


def test_one_pair_path_reads_a_filled_tensor(monkeypatch):
    """Check 4: poison, then get_power_1halo / get_power_2halo with a bias override (the one-pair kernel reads whole rows)."""
    zs = np.linspace(0.1, 2.5, 3)
    ms = np.geomspace(2e10, 1e17, 96)
    ks = np.geomspace(1e-4, 100, 512)
    b1 = np.linspace(1.0, 2.0, zs.size).reshape(-1, 1)
    ref = build(monkeypatch, False, zs, ms, ks)
    want1 = ref.get_power_1halo("electron", "g")
    want2 = ref.get_power_2halo("electron", "g", b1_in=b1, b2_in=b1)
    h = build(monkeypatch, True, zs, ms, ks)
    poison(h)
    step(h)
    got2 = h.get_power_2halo("electron", "g", b1_in=b1, b2_in=b1)
    poison(h)
    step(h)
    got1 = h.get_power_1halo("electron", "g")
    assert np.all(np.isfinite(got1)) and np.all(np.isfinite(got2))
    assert np.array_equal(got1, want1) and np.array_equal(got2, want2)


def test_row_extremes(monkeypatch):
    """Check 5: rows with no prefix, a prefix shorter than a tile, a prefix of exactly one tile, and a row that is all
    prefix.  The target grid is built from the rows' own first FFT modes k_lo = kt_1 / (r_s (1+z)) (host arithmetic on
    the row scales of a throw-away model): 128 wavenumbers between the 25 % and 50 % quantiles of k_lo, a gap, and 172
    more between the 75 % and 90 % quantiles.  Of the 3 x 96 = 288 rows a quarter then have nleft == 0 (71 rows on an
    MI355X), a quarter 0 < nleft < 128 (73), a quarter nleft == 128 exactly (72), and a tenth nleft == nk = 300 (29);
    the counts are printed and each must be non-zero."""
    zs = np.linspace(0.1, 2.5, 3)
    ms = np.geomspace(2e10, 1e17, 96)
    probe = build(monkeypatch, False, zs, ms, np.geomspace(1e-4, 100, 64))
    rss = probe._pool[(("uk", "electron"), "rowp", 5)].numpy()
    kt1 = probe._fft_grids(20, 1000)[1].numpy()[1]
    klo = np.sort((kt1 / (rss * (1.0 + zs[:, None]))).reshape(-1))
    q = lambda f: klo[int(f * (klo.size - 1))]      # noqa: E731
    ks = np.concatenate([np.geomspace(q(0.25), q(0.50), TILE), np.geomspace(q(0.75), q(0.90), 300 - TILE)])
    assert np.all(np.diff(ks) > 0)
    h, _ = check_pass(monkeypatch, zs, ms, ks)
    n, _ = hints(h.uk_profiles, "electron", zs.size * ms.size)
    kinds = {"nleft == 0": int((n == 0).sum()), "0 < nleft < TILE": int(((n > 0) & (n < TILE)).sum()),
             "nleft == TILE": int((n == TILE).sum()), "nleft == nk": int((n == ks.size).sum())}
    print(kinds)
    for k, v in kinds.items():
        assert v > 0, (k, kinds)


def test_a_c_caller_without_the_opt_in_gets_the_whole_tensor(monkeypatch):
    """Check 6: hmg_profile_fft called through ctypes, no hmg_prefix_deferral before it, into a poisoned buffer."""
    zs = np.linspace(0.1, 2.5, 3)
    ms = np.geomspace(2e10, 1e17, 96)
    ks = np.geomspace(1e-4, 100, 512)
    ref = build(monkeypatch, False, zs, ms, ks)
    want = ref.uk_profiles["electron"]
    h = build(monkeypatch, True, zs, ms, ks, groups=False)      # (one launch per stage: the facade calls hmg_profile_fft itself)
    ctx = h._ctx()
    calls = ctx.trace(lambda: step(h))
    fft = [args for name, args in calls if name == "hmg_profile_fft"]
    assert len(fft) == 1
    ctx.sync()
    poison(h)
    rc = ctx.lib.hmg_profile_fft(ctx.handle, *fft[0])
    assert rc == 0
    d = h.uk_profiles.dev("electron", fill=False)
    assert not h.uk_profiles._pending("electron")
    raw = d.numpy()
    assert not np.isnan(raw).any()
    assert np.array_equal(raw, want)
    # and the fill entry point on its own books: poison the deferred tiles of a whole tensor, fill, compare
    n, _ = hints(h.uk_profiles, "electron", zs.size * ms.size)
    holed = raw.reshape(n.size, ks.size).copy()
    for r, k in enumerate(n & ~(TILE - 1)):
        holed[r, :k] = np.nan
    ctx.write(d, holed.reshape(d.shape))
    hn, hc = h.uk_profiles.hint("electron")
    ctx.call("hmg_prefix_fill_rows", d.ptr, hn.ptr, hc.ptr, n.size, ks.size)
    assert np.array_equal(d.numpy(), want)
