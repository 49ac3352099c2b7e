"""GPU checks of the HOD parameter ensemble (HaloModel.hod_ensemble_device / get_power_hod_ensemble /
hod_ensemble_occupations; hmg_hod_ensemble, hmg_hod_ensemble_power); definition and gates in DESIGN.md section 21.

Three redshifts across the SHMR split at 0.8; 70 masses (a full 64-mass tile of the sums and a partial one); 259
wavenumbers (a full 256-column workgroup and a partial one); 11 sets (a full set tile of 8 and a partial one) and single
sets; the whole grid (set tile 8) and a scattered, unsorted kindex (set tile 2); the NFW tensor for both legs (one tensor,
loaded once) and a Battaglia gas tensor with a deferred prefix as the matter leg.  The sets vary every column; set 0 is
the defaults, set 10 has sig = 0.05 and a high threshold: Nc is exactly 0, in (0, 1e-8] and above 1e-8 along the grid.

Occupations, n_gal, b_g and the thresholds of the n_gal mode are compared bit for bit with add_hod of each set alone; the
spectra with get_power_1halo / get_power_2halo of that HOD (twice the restatement's tol: each side is within one of its
exact sums; the 1-halo planes with the tol of the other kernel's damping factor added) and with the numpy restatement
(tests/helpers/hod_ensemble_model.py) at its derived tol."""
import os
import sys

import numpy as np
import pytest

from hmvec_amd import hod_sets

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import hod_ensemble_model as hm  # noqa: E402
from lensing_model import model  # noqa: E402

pytestmark = pytest.mark.gpu

NM, NK, S = 70, 259, 11
ZS = np.array([0.2, 0.8, 1.4])
SCATTERED = np.array([NK - 1, 3, 130, 0, 17, 64, 8])
OCC = ("Nc", "Ns", "NsNsm1", "NcNs")
SETS = hod_sets(sig=[0.2, 0.15, 0.3, 0.25, 0.2, 0.18, 0.22, 0.35, 0.12, 0.2, 0.05],
                alphasat=[1.0, 0.8, 1.2, 1.1, 0.9, 1.0, 1.3, 0.7, 1.05, 0.95, 1.0],
                Bsat=[9.04, 7.0, 12.0, 9.5, 8.0, 10.0, 6.0, 15.0, 9.04, 11.0, 9.04],
                betasat=[0.74, 0.6, 0.9, 0.8, 0.7, 0.74, 0.65, 0.85, 0.78, 0.72, 0.74],
                Bcut=[1.65, 0.5, 3.0, 0.0, 1.0, 2.0, 1.65, 2.5, 0.8, 1.2, 1.65],
                betacut=[0.59, 0.4, 0.8, 0.59, 0.5, 0.7, 0.45, 0.65, 0.55, 0.6, 0.59])
L10 = np.array([10.5, 10.3, 10.8, 10.6, 10.4, 10.7, 10.2, 10.9, 10.5, 10.45, 11.4])[:, None] + np.array([0.0, 0.05, -0.05])[None, :]
MTHRESH = 10 ** L10
PREFIX = {"max": "e", "min": "m"}


def override(s):
    return {"hod_" + c: float(v) for c, v in zip(SETS.columns, SETS[s])}


@pytest.fixture(scope="module")
def h():
    m = model(ZS, ks=np.geomspace(1e-3, 30, NK), ms=np.geomspace(1e11, 10 ** 15.5, NM))
    m.add_battaglia_profile("electron", family="AGN", xmax=20, nxs=512)
    for corr, pre in PREFIX.items():
        for s in range(S):
            m.add_hod(f"{pre}{s}", mthresh=MTHRESH[s], corr=corr, param_override=override(s))
    return m


def single_occ(h, corr):
    pre = PREFIX[corr]
    out = {k: np.stack([np.asarray(h.hods[f"{pre}{s}"][k]) for s in range(S)]) for k in OCC + ("ngal", "bg")}
    return out


_ENS, _REF = {}, {}


def ens(h, corr="max", matter=None, kidx=None):
    """The ensemble of the 11 sets (planes, parts, sums), computed once per case and never changed."""
    key = (corr, matter, kidx is not None)
    if key not in _ENS:
        _ENS[key] = h.get_power_hod_ensemble(SETS, mthresh=MTHRESH, corr=corr, matter_name=matter, kindex=kidx, parts=True)
    return _ENS[key]


def ref(h, corr="max", matter=None, kidx=None):
    key = (corr, matter, kidx is not None)
    if key not in _REF:
        _REF[key] = hm.from_model(h, single_occ(h, corr), matter=matter, kindex=kidx)
    return _REF[key]


def within(got, want, tol, what):
    err = np.abs(got - want)
    worst = float(np.max(err / np.maximum(tol, 1e-300)))
    print(f"{what}: worst |got - ref| / tol = {worst:.3g}")
    return bool(np.all(err <= tol)), worst


CASES = [("max", None, None), ("max", None, SCATTERED), ("max", "electron", None), ("max", "electron", SCATTERED),
         ("min", None, None), ("min", "electron", SCATTERED)]
IDS = ["max-nfw-grid", "max-nfw-kindex", "max-electron-grid", "max-electron-kindex", "min-nfw-grid", "min-electron-kindex"]


# ---------------------------------------------------------------- 5. occupations are the single-set bits
@pytest.mark.parametrize("corr", ["max", "min"])
def test_occupations_have_the_bits_of_each_set_alone(h, corr):
    got = h.hod_ensemble_occupations(SETS, mthresh=MTHRESH, corr=corr)
    want = single_occ(h, corr)
    for k in OCC:
        assert got[k].shape == (S, 3, NM)
    for k in OCC + ("ngal", "bg"):
        assert np.array_equal(got[k], want[k]), (k, float(np.max(np.abs(got[k] - want[k]))))
    nc = got["Nc"][10]
    assert (nc == 0).any() and ((nc > 0) & (nc <= 1e-8)).any() and (nc > 1e-8).any()      # the isclose branch is taken
    if corr == "max":
        assert np.all(got["NsNsm1"][10][nc <= 1e-8] == 0) and np.any(got["Ns"][10][(nc > 0) & (nc <= 1e-8)] > 0)
    e = ens(h, corr)
    assert np.array_equal(e["ngal"], want["ngal"]) and np.array_equal(e["bg"], want["bg"])
    assert np.array_equal(e["log10mthresh"], np.log10(MTHRESH))


# ---------------------------------------------------------------- 6. spectra against the existing path
@pytest.mark.parametrize("corr,matter,kidx", CASES, ids=IDS)
def test_spectra_against_get_power(h, corr, matter, kidx):
    """Measured on an MI355X, worst |got - get_power| / (2 tol) over the six cases and the eleven sets: gg_1h 0.019, gg_2h
    0.0060, gm_1h 0.020, gm_2h 0.0056."""
    e, r = ens(h, corr, matter, kidx), ref(h, corr, matter, kidx)
    rd = hm.with_damping_tol(r, h.ks, h.p["kstar_damping"], kidx)
    cols = np.arange(NK) if kidx is None else kidx
    n = cols.size
    # non-vacuity, from the restatement alone
    for key in ("gg_1h", "gm_1h"):
        val, tol = rd[key]
        assert val.shape == (S, 3, n) and np.all(val > 0) and np.all(tol <= 1e-12 * np.abs(val)), key
    for key in ("gg_2h", "gm_2h"):
        val, tol = r[key]
        assert np.all(val > 0) and np.all(tol <= 1e-10 * np.abs(val)), key
    pre, m_ = PREFIX[corr], "nfw" if matter is None else matter
    for s in range(S):
        g = f"{pre}{s}"
        real = {"gg_1h": h.get_power_1halo(g, g), "gg_2h": h.get_power_2halo(g, g),
                "gm_1h": h.get_power_1halo(g, m_), "gm_2h": h.get_power_2halo(g, m_)}
        for key in hm.PLANES:
            src = rd if key.endswith("1h") else r
            ok, worst = within(e[key][s], real[key][:, cols], 2 * src[key][1][s], f"set {s} {key} against get_power (of twice the tol)")
            assert ok, (s, key, worst)
    assert np.array_equal(e["gg"], e["gg_1h"] + e["gg_2h"]) and np.array_equal(e["gm"], e["gm_1h"] + e["gm_2h"])


# ---------------------------------------------------------------- 7. against the restatement
@pytest.mark.parametrize("corr,matter,kidx", CASES, ids=IDS)
def test_spectra_and_parts_against_the_restatement(h, corr, matter, kidx):
    """Measured on an MI355X, worst |got - restatement| / tol over the six cases: gg_1h 0.035, gg_2h 0.012, gm_1h 0.036,
    gm_2h 0.011, G 0.035, X 0.036, I 0.033, ngal 0.018, bg 0.011."""
    e, r = ens(h, corr, matter, kidx), ref(h, corr, matter, kidx)
    for key in hm.PLANES + hm.PARTS:
        assert np.all(np.isfinite(e[key]))
        ok, worst = within(e[key], *r[key], f"{key}")
        assert ok, (key, worst)
    for key in ("ngal", "bg"):
        ok, worst = within(e[key], *r[key], key)
        assert ok, (key, worst)


# ---------------------------------------------------------------- 8. independence and determinism
def test_a_set_does_not_depend_on_the_rest_of_the_call(h):
    whole = h.get_power_hod_ensemble(SETS, mthresh=MTHRESH, matter_name="electron", parts=True)
    keys = hm.PLANES + hm.PARTS + ("ngal", "bg")
    again = h.get_power_hod_ensemble(SETS, mthresh=MTHRESH, matter_name="electron", parts=True)
    for k in keys:
        assert np.array_equal(whole[k], again[k]), k                                  # a repeat
    for s in (0, 7, 8, 10):                                                            # alone: S = 1
        one = h.get_power_hod_ensemble(SETS[s:s + 1], mthresh=MTHRESH[s], matter_name="electron", parts=True)
        for k in keys:
            assert one[k].shape[0] == 1 and np.array_equal(one[k][0], whole[k][s]), (s, k)
    perm = np.array([4, 10, 0, 9, 2, 7, 1, 8, 3, 6, 5])                               # another tile, another place in it
    shuffled = h.get_power_hod_ensemble(SETS[perm], mthresh=MTHRESH[perm], matter_name="electron", parts=True)
    for k in keys:
        assert np.array_equal(shuffled[k], whole[k][perm]), k
    picked = h.get_power_hod_ensemble(SETS, mthresh=MTHRESH, matter_name="electron", kindex=SCATTERED, parts=True)
    for k in hm.PLANES + hm.PARTS:                                                     # set tile 2 against set tile 8
        assert np.array_equal(picked[k], whole[k][..., SCATTERED]), k
    undamped = h.get_power_hod_ensemble(SETS, mthresh=MTHRESH, damping=False, parts=True)
    assert np.array_equal(undamped["gg_1h"], undamped["G"]) and np.array_equal(undamped["gm_1h"], undamped["X"])


# ---------------------------------------------------------------- 9. the n_gal mode
def test_ngal_mode_finds_the_thresholds_of_each_set_alone(h):
    """Measured on an MI355X: 17 to 20 bisection launches for the sets alone, 20 for the ensemble; worst |got - get_power| /
    (2 tol) gg_1h 0.018, gg_2h 0.0070, gm_1h 0.020, gm_2h 0.0055."""
    fixed = single_occ(h, "max")["ngal"]
    target = fixed * np.linspace(0.5, 2.0, S)[:, None]
    res = h.hod_ensemble_device(SETS, ngal=target)
    got = res.log10mthresh.numpy()
    iters = []
    for s in range(S):
        calls = []
        orig = h._hod_device
        h._hod_device = lambda *a, **k: (calls.append(1), orig(*a, **k))[1]
        try:
            h.add_hod(f"n{s}", ngal=target[s], param_override=override(s))
        finally:
            del h._hod_device
        iters.append(len(calls) - 1)                                                   # (the last launch is the HOD itself)
        assert np.array_equal(got[s], h.hods[f"n{s}"]["log10mthresh"][:, 0]), s
        assert np.array_equal(res.ngal.numpy()[s], h.hods[f"n{s}"]["ngal"]), s
    print("bisection launches of the sets alone:", iters, "of the ensemble:", res.iterations)
    assert len(set(iters)) > 1 and res.iterations == max(iters)                        # the stop rule is per set
    power = res.power.numpy()
    occ = {k: np.stack([np.asarray(h.hods[f"n{s}"][k]) for s in range(S)]) for k in OCC}
    r = hm.with_damping_tol(hm.from_model(h, occ), h.ks, h.p["kstar_damping"])
    for s in range(S):
        g = f"n{s}"
        real = (h.get_power_1halo(g, g), h.get_power_2halo(g, g), h.get_power_1halo(g, "nfw"), h.get_power_2halo(g, "nfw"))
        for i, key in enumerate(hm.PLANES):
            ok, worst = within(power[i][s], real[i], 2 * r[key][1][s], f"n_gal mode, set {s} {key} (of twice the tol)")
            assert ok, (s, key, worst)
    shared = h.get_power_hod_ensemble(SETS[:3], ngal=target[1])                        # (nz,): shared by the sets
    assert shared["log10mthresh"].shape == (3, 3) and np.array_equal(shared["log10mthresh"][1], got[1])


# ---------------------------------------------------------------- 10. refusals and no side effects
def test_refusals_and_no_side_effects(h):
    h.add_battaglia_pres_profile("y", family="pres", xmax=5, nxs=512)
    names, version = set(h.hods), h._version
    cached = h.get_power("e0", "nfw")
    ctx = h._ctx()
    launched = []
    orig_call, orig_now = ctx.call, ctx.call_now
    ctx.call = lambda name, *a, **kw: (launched.append(name), orig_call(name, *a, **kw))[1]
    ctx.call_now = lambda name, *a: (launched.append(name), orig_now(name, *a))[1]
    try:
        for kw in (dict(), dict(mthresh=MTHRESH, ngal=MTHRESH), dict(mthresh=MTHRESH[:5]), dict(mthresh=MTHRESH[:, :2]),
                   dict(ngal=np.ones(4)), dict(mthresh=-MTHRESH), dict(mthresh=MTHRESH, matter_name="y"),
                   dict(mthresh=MTHRESH, matter_name="nope"), dict(mthresh=MTHRESH, satellite_profile_name="y"),
                   dict(mthresh=MTHRESH, satellite_profile_name="e0"), dict(mthresh=MTHRESH, kindex=[0, NK]),
                   dict(mthresh=MTHRESH, kindex=[-1]), dict(mthresh=MTHRESH, kindex=[]), dict(mthresh=MTHRESH, corr="both")):
            with pytest.raises(ValueError):
                h.hod_ensemble_device(SETS, **kw)
        with pytest.raises(ValueError):
            h.hod_ensemble_device(np.ones((2, 5)), mthresh=MTHRESH[:2])
        with pytest.raises(ValueError):
            h.hod_ensemble_occupations(SETS, mthresh=MTHRESH, ngal=MTHRESH)
        assert not [n for n in launched if "ensemble" in n], launched                  # every refusal was on the host
        h.get_power_hod_ensemble(SETS, mthresh=MTHRESH, kindex=SCATTERED)
        assert "hmg_hod_ensemble" in launched and "hmg_hod_ensemble_power" in launched
        assert set(h.hods) == names and h._version == version
        del launched[:]
        assert np.array_equal(h.get_power("e0", "nfw"), cached)                        # still cached: no mass integrals
        assert not [n for n in launched if "power" in n or "hod" in n], launched
    finally:
        del ctx.call, ctx.call_now
    # the native check of a node list (a C caller has no host check in front of it)
    import ctypes as C
    from hmvec_amd import _native as nat
    nz = 3
    d_par, d_thr = ctx.upload(np.asarray(SETS)), ctx.upload(np.log10(MTHRESH))
    d_ngal, d_bg = ctx.empty((S, nz)), ctx.empty((S, nz))
    from hmvec_amd import hod_ensemble as he
    coef = ctx.empty((he.coef_block_size(S, nz, NM),))
    ctx.call("hmg_hod_ensemble", S, nz, NM, 0, d_par.ptr, d_thr.ptr, h._d_zs().ptr, h._d_ms().ptr, h._d_nzm.ptr, h._d_bh.ptr,
             h._d_wm().ptr, d_ngal.ptr, d_bg.ptr, None, coef.ptr)
    d_u = h.uk_profiles.dev("nfw")
    out, d_damp = ctx.empty((4, S, nz, 2)), ctx.upload(np.ones(2))
    block = h._model_block("hmg_hod_ensemble_power").values()      # (in the order of the entry point's parameters)
    for bad in ([0, NK], [-1, 5]):
        d_k = ctx.upload_int32(np.array(bad, dtype=np.int32))
        rc = ctx.lib.hmg_hod_ensemble_power(ctx.handle, S, nz, NM, NK, 2, d_u.ptr, d_u.ptr, coef.ptr, d_ngal.ptr, d_bg.ptr,
                                            *block, d_k.ptr, d_damp.ptr, out.ptr, None)
        assert rc != 0 and b"outside 0 .. nk-1" in ctx.lib.hmg_last_error()
    rc = ctx.lib.hmg_hod_ensemble_power(ctx.handle, S, nz, NM, NK, 2, d_u.ptr, d_u.ptr, coef.ptr, d_ngal.ptr, d_bg.ptr,
                                        *block, None, d_damp.ptr, out.ptr, None)
    assert rc != 0 and b"n must be nk" in ctx.lib.hmg_last_error()
    rc = ctx.lib.hmg_hod_ensemble(ctx.handle, S, nz, NM, 2, d_par.ptr, d_thr.ptr, h._d_zs().ptr, h._d_ms().ptr, h._d_nzm.ptr,
                                  h._d_bh.ptr, h._d_wm().ptr, d_ngal.ptr, d_bg.ptr, None, None)
    assert rc != 0 and b"corr must be 0 (max) or 1 (min)" in ctx.lib.hmg_last_error()
    assert C.sizeof(C.c_double) == 8 and nat.ABI_VERSION == 10
