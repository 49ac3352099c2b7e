"""CPU-only checks of the host layer and of the C-ABI library's symbol table.

No compute calls are made here (there is no GPU in the build container).
"""
import ctypes
import os
import re

import numpy as np
import pytest
from scipy.integrate import simpson

from conftest import REPO, load_golden, merged_params, rel_err
from hmvec_amd import _native as nat
from hmvec_amd.background import AnalyticBackground
from hmvec_amd.cosmology import Cosmology
from hmvec_amd.quadrature import gradient_is_uniform, simpson_weights, trapz_weights


def test_library_exports_every_declared_symbol():
    """Every hmg_* function declared in include/hmgrid.h must be exported by libhmgrid.so
    and bound in the ctypes table (and vice versa)."""
    header = open(os.path.join(REPO, "include", "hmgrid.h")).read()
    declared = set(re.findall(r"\b(hmg_[a-z0-9_]+)\s*\(", header))
    declared -= {"hmg_ctx", "hmg_tracer", "hmg_massfn_params", "hmg_hod_params"}
    assert os.path.exists(nat.LIB_PATH), "libhmgrid.so not built (run __graft_entry__.build())"
    lib = ctypes.CDLL(nat.LIB_PATH)
    for name in sorted(declared):
        assert hasattr(lib, name), f"{name} declared in hmgrid.h but not exported"
    bound = set(nat.SIGNATURES) | {"hmg_last_error"}
    assert declared == bound, (declared - bound, bound - declared)
    assert nat.load().hmg_abi_version() == nat.ABI_VERSION


def test_missing_library_fails_loudly(monkeypatch):
    monkeypatch.setattr(nat, "_lib", None)
    monkeypatch.setattr(nat, "LIB_PATH", "/nonexistent/libhmgrid.so")
    with pytest.raises(ImportError, match="no CPU"):
        nat.load()


@pytest.mark.parametrize("n", [2, 3, 8, 9, 2001, 10000])
def test_simpson_weights_match_scipy(n):
    x = np.geomspace(1e-4, 2000.0, n)
    rng = np.random.default_rng(n)
    y = rng.random(n) + np.sin(x) ** 2
    assert abs(np.dot(simpson_weights(x), y) / simpson(y, x=x) - 1) < 5e-15


def test_trapz_weights_and_gradient_flag():
    x = np.geomspace(2e10, 1e17, 57)
    y = np.cos(np.log(x))
    trapz = getattr(np, "trapezoid", None) or np.trapz
    assert np.isclose(np.dot(trapz_weights(x), y), trapz(y, x), rtol=1e-14)
    assert gradient_is_uniform(np.arange(5.0))[0] is True
    assert gradient_is_uniform(np.log(x))[0] == bool((np.diff(np.log(x)) == np.diff(np.log(x))[0]).all())


@pytest.mark.parametrize("case", ["case_a", "case_b", "case_c"])
def test_host_cosmology_reproduces_reference_inputs(case):
    """The product's own host cosmology (Eisenstein-Hu P(k), densities, H(z)) must give the
    arrays the reference computed, because they are the inputs of every kernel."""
    g = load_golden(case)
    p = merged_params(g["meta"]["params"])
    cos = Cosmology(p, accuracy="low", engine="analytic")
    zs, ks = g["zs"], g["ks"]
    assert rel_err(cos.P_lin_approx(ks, zs), g["in_Pzk"]) < 1e-13
    ksig = np.geomspace(p["sigma2_kmin"], p["sigma2_kmax"], p["sigma2_numks"])
    assert rel_err(cos.P_lin_approx(ksig, zs), g["in_sPzk"]) < 1e-13
    assert rel_err(cos.rho_critical_z(zs), g["in_rho_crit_zs"]) < 1e-14
    assert rel_err(cos.rho_matter_z(0), g["in_rho_matter_0"]) < 1e-14
    assert rel_err(cos.h_of_z(zs), g["in_h_of_z_zs"]) < 1e-14
    assert rel_err(cos.comoving_radial_distance(zs), g["in_chi_zs"]) < 1e-13
    assert abs(cos.h - float(g["in_h"])) < 1e-15 and abs(cos.omm0 - float(g["in_omm0"])) < 1e-15


def test_provider_caches_return_what_a_fresh_evaluation_returns():
    """Round 5: Cosmology.Tk keeps its last results per (parameters, grid OBJECT), P_lin_approx the whole product on the
    shared read-only sigma^2 grid (by identity; writable grids by their bytes).  Alternating two cosmologies on the same
    grids, a grid modified in place between calls, equal values in a new array: every answer equals the uncached
    evaluation bit for bit."""
    from hmvec_amd import cosmology as cm
    pa = merged_params({})
    pb = merged_params({"omch2": 0.11, "ns": 0.97, "As": 2.3e-9})
    zs = np.array([0.0, 0.7, 2.1])
    kq = cm.sigma2_kgrid(pa["sigma2_kmin"], pa["sigma2_kmax"], pa["sigma2_numks"])
    assert kq is cm.sigma2_kgrid(pa["sigma2_kmin"], pa["sigma2_kmax"], pa["sigma2_numks"]) and not kq.flags.writeable
    ks = np.geomspace(1e-4, 50, 301)

    def fresh(p, k):
        cm._TK_CACHE.clear(); cm._PLIN_CACHE.clear()
        c = Cosmology(p, accuracy="low", engine="analytic")
        return c.Tk(k).copy(), c.P_lin_approx(k, zs).copy()

    want = {(n, g): fresh(p, k) for n, p in (("a", pa), ("b", pb)) for g, k in (("q", kq), ("k", ks))}
    cm._TK_CACHE.clear(); cm._PLIN_CACHE.clear()
    ca, cb = (Cosmology(p, accuracy="low", engine="analytic") for p in (pa, pb))
    for _ in range(3):                                   # hits after the first round
        for n, c in (("a", ca), ("b", cb)):
            for g, k in (("q", kq), ("k", ks)):
                assert np.array_equal(c.Tk(k), want[(n, g)][0]) and np.array_equal(c.P_lin_approx(k, zs), want[(n, g)][1])
    first = ca._P_lin_approx_shared(kq, zs)
    assert ca._P_lin_approx_shared(kq, zs) is first and not first.flags.writeable   # the shared product itself, read-only
    pub = ca.P_lin_approx(kq, zs)                                                # the public call: the caller's own array,
    assert pub is not first and pub.flags.writeable and np.array_equal(pub, first)   # writable like the reference's
    pub *= 2.0
    assert np.array_equal(ca.P_lin_approx(kq, zs), first)                        # ... and the cache is out of its reach
    tk_pub = ca.Tk(kq)
    assert tk_pub.flags.writeable and tk_pub is not ca.Tk(kq)
    tk_pub[:] = 0.0
    assert np.array_equal(ca.Tk(kq), want[("a", "q")][0])
    assert ca.P_lin_approx(ks, zs) is not ca.P_lin_approx(ks, zs)               # a user's grid: a fresh array every time
    assert not np.array_equal(ca.P_lin_approx(kq, zs + 0.1), first)             # other redshifts: another entry
    k2 = ks.copy()
    t1 = ca.Tk(k2).copy()
    assert np.array_equal(ca.Tk(ks.copy()), t1)          # equal values in a new writable array: found by content
    k2[10] *= 1.5                                        # the same OBJECT, ONE element changed in place: another grid
    t2 = ca.Tk(k2)
    assert not np.array_equal(t1, t2) and np.array_equal(t2, ca._Tk_eval(k2, "eisenhu_osc"))


def test_a_read_only_view_of_a_writable_grid_is_keyed_by_its_contents():
    """`not ks.flags.writeable` does not mean the contents cannot change - a read-only VIEW follows
    its writable base, and a flag can be toggled.  Foreign arrays are keyed by their bytes whatever their flag; only the
    grid objects this module made itself (sigma2_kgrid) are trusted by identity."""
    from hmvec_amd import cosmology as cm
    cm._TK_CACHE.clear(); cm._PLIN_CACHE.clear()
    c = Cosmology(merged_params({}), accuracy="low", engine="analytic")
    zs = np.array([0.0, 1.0])
    base = np.geomspace(1e-4, 50, 257)
    view = base.view()
    view.setflags(write=False)
    t1, p1 = c.Tk(view).copy(), c.P_lin_approx(view, zs).copy()
    base[100:] *= 1.25                                   # the view's contents change under the cache
    t2, p2 = c.Tk(view), c.P_lin_approx(view, zs)
    assert np.array_equal(t2, c._Tk_eval(view, "eisenhu_osc")) and not np.array_equal(t1, t2)
    assert not np.array_equal(p1, p2) and np.array_equal(p2[:, :100], p1[:, :100])
    own = np.geomspace(1e-4, 50, 129)                    # an owner whose flag is toggled around an in-place change
    own.setflags(write=False)
    t3 = c.Tk(own).copy()
    own.setflags(write=True); own *= 1.1; own.setflags(write=False)
    assert np.array_equal(c.Tk(own), c._Tk_eval(own, "eisenhu_osc")) and not np.array_equal(c.Tk(own), t3)
    kq = cm.sigma2_kgrid(1e-4, 2e3, 500)                 # the module's own grid: by identity, shared, read-only
    assert cm._grid_identity(kq) is kq and isinstance(cm._grid_identity(view), tuple)
    assert not cm._is_shared_product(p2) and cm._is_shared_product(c._P_lin_approx_shared(kq, zs))


def test_background_distances_consistent():
    bg = AnalyticBackground(67.3, 0.02225, 0.1198)
    z = np.array([0.0, 0.5, 2.0])
    chi = bg.comoving_radial_distance(z)
    assert chi[0] == 0.0 and np.all(np.diff(chi) > 0)
    # finite-difference check of d chi / dz = c/H
    dz = 1e-4
    num = (bg.comoving_radial_distance(z[1:] + dz) - bg.comoving_radial_distance(z[1:] - dz)) / (2 * dz)
    assert np.allclose(num, 1.0 / bg.h_of_z(z[1:]), rtol=1e-7)
    assert np.allclose(bg.angular_diameter_distance2(0.5, 2.0) * 3.0, chi[2] - chi[1], rtol=1e-12)


def test_engine_and_accuracy_errors():
    with pytest.raises(ValueError):
        Cosmology(engine="bogus")
    with pytest.raises(ValueError):
        Cosmology({"sigma8": 0.8}, accuracy="low", engine="analytic")


class _FakePkBackground(AnalyticBackground):
    """Provider with a Boltzmann-code-like P(k): the EH spectrum scaled by a z-dependent factor,
    exposed through the CAMB interpolator interface (.P(zs, ks, grid=True))."""

    def __init__(self, cos, scale):
        p = cos.p
        super().__init__(p["H0"], p["ombh2"], p["omch2"])
        self._cos, self._scale = cos, scale

    def pk_interpolator(self, zs, kmax, var="total", nonlinear=False):
        cos, scale = self._cos, self._scale

        class PK:
            @staticmethod
            def P(z, k, grid=True):
                z, k = np.atleast_1d(z), np.atleast_1d(k)
                return cos.P_lin_approx(k, z) * scale(z)[:, None]
        return PK


def test_medium_accuracy_through_provider_seam():
    """Row N3: accuracy='medium'/'high' work with any provider that offers pk_interpolator();
    the EH-shape renormalisation of hmvec/cosmology.py:353-374 is reproduced."""
    base = Cosmology(accuracy="low", engine="analytic")
    scale = lambda z: 1.0 + 0.1 * np.asarray(z)        # noqa: E731
    zs, ks = np.array([0.0, 0.7, 2.0]), np.geomspace(1e-3, 10, 50)
    cos = Cosmology(accuracy="medium", background=_FakePkBackground(base, scale))
    want = base.P_lin_approx(ks, zs) * scale(zs)[:, None]
    # the reference normalises with T(knorm), not T(knorm)^2 (hmvec/cosmology.py:372): kept as is
    tk_norm = float(base.Tk(np.array([1e-4]))[0])
    assert rel_err(cos.P_lin(ks, zs), want * tk_norm) < 1e-12
    assert rel_err(cos.P_lin_slow(ks, zs), want) < 1e-14
    assert rel_err(cos._get_matter_power(zs, ks), want) < 1e-14
    with pytest.raises(NotImplementedError):
        Cosmology(accuracy="low", engine="analytic").get_pk_interpolator(zs, 10.0)


def _recording_camb(monkeypatch, calls):
    """A stand-in `camb` module (the shape tools/make_golden.py registers for the reference) that RECORDS what the
    seam passes to it: set_params keywords, the parameter object's flags, get_matter_power_interpolator arguments."""
    import sys
    import types
    from hmvec_amd.background import TabulatedPowerInterpolator
    camb = types.ModuleType("camb")
    model = types.ModuleType("camb.model")
    model.Transfer_Weyl = "Transfer_Weyl_sentinel"

    class Pars:
        pass

    def set_params(**kw):
        calls.append(("set_params", dict(kw)))
        p = Pars()
        p.kw = dict(kw)
        p.YHe = 0.2454 if kw.get("YHe") is None else kw["YHe"]
        return p

    def get_background(pars):
        calls.append(("get_background", {"WantTransfer": getattr(pars, "WantTransfer", None),
                                         "WantTensors": getattr(pars, "WantTensors", None)}))
        k = pars.kw
        return AnalyticBackground(H0=k["H0"] if k["H0"] is not None else 67.0, ombh2=k["ombh2"], omch2=k["omch2"],
                                  omk=k["omk"], w0=k["w"], wa=k["wa"], YHe=pars.YHe)

    def get_matter_power_interpolator(pars, **kw):
        calls.append(("get_matter_power_interpolator", dict(kw), pars))
        from helpers.pk_table import table
        return TabulatedPowerInterpolator(*table(pars.kw["ns"]))

    camb.set_params, camb.get_background = set_params, get_background
    camb.get_matter_power_interpolator, camb.model = get_matter_power_interpolator, model
    monkeypatch.setitem(sys.modules, "camb", camb)
    monkeypatch.setitem(sys.modules, "camb.model", model)
    return camb


def test_camb_seam_forwards_the_reference_keywords(monkeypatch):
    """VERDICT r05 missing #2 / weak #8: CambBackground is exercised through a recording stand-in `camb`.  The exact
    keyword set of camb.set_params (hmvec/cosmology.py:161-176), the two Want* flags (:177-179) and of
    camb.get_matter_power_interpolator (:783-786) is asserted; HaloModel(accuracy='medium', engine='camb') is built up
    to its first device call (ms=None, skip_nfw=True: the constructor then only sets up the cosmology and P(z,k))."""
    from hmvec_amd import HaloModel
    from hmvec_amd.background import CambBackground
    calls = []
    _recording_camb(monkeypatch, calls)
    p = merged_params({"YHe": 0.25, "r": 0.01})
    zs, ks = np.array([0.0, 0.5, 1.5]), np.geomspace(1e-3, 5.0, 40)
    h = HaloModel(zs, ks, ms=None, params=dict(p), skip_nfw=True, accuracy="medium", engine="camb", halofit=None)
    assert isinstance(h._background, CambBackground)
    name, kw = calls[0]
    assert name == "set_params"
    want = dict(ns=p["ns"], As=p["As"], r=0.01, H0=p["H0"], cosmomc_theta=None, ombh2=p["ombh2"], omch2=p["omch2"],
                mnu=p["mnu"], omk=p["omk"], tau=p["tau"], nnu=p["nnu"], num_massive_neutrinos=p["num_massive_neutrinos"],
                w=p["w0"], wa=p["wa"], dark_energy_model="ppf", halofit_version=p["default_halofit"], AccuracyBoost=2,
                pivot_scalar=p["pivot_scalar"], YHe=0.25)
    assert kw == want                                   # same keys, same values: nothing missing, nothing extra
    assert calls[1] == ("get_background", {"WantTransfer": True, "WantTensors": True})
    assert h.YHe == 0.25 and abs(h.h - p["H0"] / 100.0) < 1e-15
    # the constructor's P(z,k) for accuracy != 'low' (hmvec/hmvec.py:99-100 -> cosmology.py:227-229,783-786)
    name, kw, pars = calls[2]
    assert name == "get_matter_power_interpolator" and pars is h._background.pars
    assert kw == dict(nonlinear=False, hubble_units=False, k_hunit=False, kmax=ks.max(), var1="delta_tot",
                      var2="delta_tot", zmax=zs[-1])
    from helpers.pk_table import table
    from hmvec_amd.background import TabulatedPowerInterpolator
    assert np.array_equal(h.Pzk, TabulatedPowerInterpolator(*table(p["ns"])).P(zs, ks, grid=True))
    # the other two variables of hmvec/cosmology.py:775-782 and the non-linear switch
    n0 = len(calls)
    h.get_pk_interpolator(zs, 3.0, var="weyl", nonlinear=True)
    h.get_pk_interpolator(zs, 3.0, var="CB")
    assert calls[n0][1]["var1"] == calls[n0][1]["var2"] == "Transfer_Weyl_sentinel" and calls[n0][1]["nonlinear"] is True
    assert calls[n0 + 1][1]["var1"] == "delta_nonu" and calls[n0 + 1][1]["kmax"] == 3.0
    with pytest.raises(KeyError):
        h.get_pk_interpolator(zs, 3.0, var="bogus")
    # halofit: version forwarded, and the non-linear P(z,k) is asked for as well (hmvec/hmvec.py:101-102)
    calls.clear()
    h2 = HaloModel(zs, ks, ms=None, params=dict(p), skip_nfw=True, accuracy="medium", engine="camb", halofit="takahashi")
    assert calls[0][1]["halofit_version"] == "takahashi"
    assert [c[1]["nonlinear"] for c in calls if c[0] == "get_matter_power_interpolator"] == [False, True]
    assert np.array_equal(h2.nPzk, h2.Pzk)              # (the stand-in serves one table for both)


def test_theta100_is_forwarded_to_camb_as_cosmomc_theta(monkeypatch, capsys):
    """hmvec/cosmology.py:140-143,163: theta100 -> cosmomc_theta = theta100/100 with H0=None.  The reference then needs
    `omm` to define h (its h is otherwise unassigned: UnboundLocalError at hmvec/cosmology.py:214, after CAMB was set up);
    both behaviours are kept.  Without CAMB the closed-form background cannot solve theta -> H0 and says so."""
    calls = []
    _recording_camb(monkeypatch, calls)
    p = merged_params({"theta100": 1.04109, "omm": 0.31})
    cos = Cosmology(dict(p), accuracy="medium", engine="camb")
    out = capsys.readouterr().out
    assert "WARNING: Using theta100 parameterization. H0 ignored." in out and "WARNING: omm specified" in out
    kw = calls[0][1]
    assert kw["H0"] is None and kw["cosmomc_theta"] == 1.04109 / 100.0
    assert abs(kw["omch2"] - (0.31 * (p["H0"] / 100.0) ** 2 - p["ombh2"])) < 1e-15      # omm rewrote omch2 first
    assert abs(cos.h - p["H0"] / 100.0) < 1e-15
    calls.clear()
    with pytest.raises(UnboundLocalError):
        Cosmology(merged_params({"theta100": 1.04109}), accuracy="medium", engine="camb")
    assert calls and calls[0][1]["cosmomc_theta"] == 1.04109 / 100.0                     # ... after CAMB was set up
    with pytest.raises(NotImplementedError):
        Cosmology(merged_params({"theta100": 1.04109, "omm": 0.31}), accuracy="low", engine="analytic")


def test_bench_launcher_dry_run_and_failure_propagation():
    """`python bench.py --gpus N` without a rank environment spawns the N ranks itself (the way the
    driver starts N=1).  --dry-run shows the dispatch; on this GPU-less box the ranks fail at context
    creation and the launcher must report that with a non-zero exit instead of hanging."""
    import json
    import subprocess
    import sys
    from conftest import REPO
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    bench = os.path.join(REPO, "bench.py")
    r = subprocess.run([sys.executable, bench, "--gpus", "2", "--steps", "3", "--dry-run"], env=env,
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    d = json.loads(r.stdout.strip().splitlines()[-1])
    assert d["n_ranks"] == 2 and "--dry-run" not in d["cmd"] and d["cmd"][-2:] == ["--steps", "3"]
    assert [e["RANK"] for e in d["rank_env"]] == ["0", "1"] and all(e["WORLD_SIZE"] == "2" for e in d["rank_env"])
    assert len({e["MASTER_PORT"] for e in d["rank_env"]}) == 1 and d["rank_env"][0]["MASTER_ADDR"] == "127.0.0.1"
    try:
        import ctypes
        ctypes.CDLL("libamdhip64.so").hipGetDeviceCount
        has_gpu = os.path.exists("/dev/kfd")
    except OSError:
        has_gpu = False
    if not has_gpu:
        r = subprocess.run([sys.executable, bench, "--gpus", "2", "--steps", "2", "--warmup", "1", "--no-cpu-baseline"],
                           env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode != 0 and "rank exit codes" in r.stderr


@pytest.mark.parametrize("failing", ["1", "0"])
def test_bench_launcher_stops_everything_when_one_rank_dies(failing, capfd):
    """A rank that dies before the communicator exists must not leave its peers waiting (in ncclCommInitRank,
    at the rendezvous file) until the driver's time limit: the launcher polls ALL ranks, terminates the others
    on the first non-zero exit, reports that rank's stderr and returns non-zero - in seconds."""
    import argparse
    import importlib.util
    import sys
    import time
    from conftest import REPO
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(REPO, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    helper = os.path.join(REPO, "tests", "helpers", "launcher_rank.py")
    t0 = time.monotonic()
    rc = bench.spawn_ranks(argparse.Namespace(gpus=3, dry_run=False), [], cmd=[sys.executable, helper, failing, "120"])
    took = time.monotonic() - t0
    out, err = capfd.readouterr()
    assert rc != 0 and took < 10.0, (rc, took)
    assert f"rank {failing} exited with code 3" in err and "fails on purpose" in err


def test_bench_launcher_deadline(monkeypatch, capfd):
    """... and a launch in which nobody fails but nobody finishes either ends at its deadline."""
    import argparse
    import importlib.util
    import sys
    from conftest import REPO
    spec = importlib.util.spec_from_file_location("bench_under_test2", os.path.join(REPO, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    monkeypatch.setenv("HMG_LAUNCH_DEADLINE", "1.5")
    helper = os.path.join(REPO, "tests", "helpers", "launcher_rank.py")
    rc = bench.spawn_ranks(argparse.Namespace(gpus=2, dry_run=False), [], cmd=[sys.executable, helper, "none", "60"])
    out, err = capfd.readouterr()
    assert rc != 0 and "deadline" in err and "rank 0 started" in out


def test_bench_dump_outputs_writes_the_spectra_and_samples_above_the_cap(tmp_path):
    """bench.py --dump-outputs: one float64 file per (pair, term) with the spectrum as the caller gets it; above the
    size cap every file holds the same fixed, seeded sample of points, identical from call to call."""
    import importlib.util
    from conftest import REPO
    spec = importlib.util.spec_from_file_location("bench_under_test3", os.path.join(REPO, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    rng = np.random.default_rng(1)
    res = {p: (rng.standard_normal((5, 64)), rng.standard_normal((5, 64))) for p in bench.PAIRS}
    names = bench.dump_outputs(str(tmp_path / "full"), res, bench.PAIRS)
    assert len(names) == 2 * len(bench.PAIRS) and "P_g_electron_2h" in names
    for (a, b) in bench.PAIRS:
        for i, t in enumerate(("1h", "2h")):
            got = np.load(tmp_path / "full" / f"P_{a}_{b}_{t}.npy")
            assert got.dtype == np.float64 and np.array_equal(got, res[(a, b)][i])
    cap = 12 * (8 * 100 + 128)
    for d in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / d), res, bench.PAIRS, max_bytes=cap)
    files = sorted(os.listdir(tmp_path / "s1"))
    assert files == sorted(os.listdir(tmp_path / "s2")) and len(files) == 12
    assert sum(os.path.getsize(tmp_path / "s1" / f) for f in files) <= cap
    a1, a2 = np.load(tmp_path / "s1" / "P_nfw_nfw_1h.npy"), np.load(tmp_path / "s2" / "P_nfw_nfw_1h.npy")
    assert a1.shape == (100,) and np.array_equal(a1, a2) and np.isin(a1, res[("nfw", "nfw")][0]).all()


def _rehearsal_rank(rank, world, tag, directory, q):
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
    from rehearsal_comm import HostRehearsalComm
    c = HostRehearsalComm(None, rank, world, tag, directory=directory)
    got = c.exchange(np.arange(4.0) + 10.0 * rank)
    tim = c.allgather_host([1.5 + rank])
    c.barrier()
    q.put((rank, [g.tolist() for g in got], tim.tolist()))


def test_host_rehearsal_comm_exchanges_between_processes(tmp_path):
    """The file transport that rehearses the N-rank flow on a one-GPU box (tests/helpers/rehearsal_comm.py):
    three processes, every rank receives every rank's array in rank order, several rounds."""
    import multiprocessing as mp
    world = 3
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    # same parent for all ranks, as under the launcher (the file names carry the parent's PID)
    procs = [ctx.Process(target=_rehearsal_rank, args=(r, world, "t", str(tmp_path), q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, got, tim in res:
        assert got == [[0.0, 1.0, 2.0, 3.0], [10.0, 11.0, 12.0, 13.0], [20.0, 21.0, 22.0, 23.0]]
        assert tim == [[1.5], [2.5], [3.5]]
