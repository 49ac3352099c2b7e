"""CPU checks of the HOD parameter ensemble: the numpy restatement of its definition against the
reference's golden P_gg and P_gm, the table of parameter sets, the stencil and its central differences, and the
declarations and exports of the two native entry points.  No device call is made here."""
import inspect
import os
import re
import sys

import numpy as np
import pytest

from conftest import REPO, cosmo_inputs_from_golden, load_golden, merged_params, power_close
from oracle import hmref

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import hod_ensemble_model as hm  # noqa: E402


# ---------------------------------------------------------------- 1. the restatement against the reference's spectra
def test_the_restatement_reproduces_the_golden_gg_and_gm(alpha_table):
    """case_a has an HOD without a central profile: the set equal to the defaults reproduces the golden P_gg and P_gm, 1h
    and 2h, at the project's gate; a set with another alphasat and Bcut differs from it by more than that gate."""
    from hmvec_amd import hod_sets
    g = load_golden("case_a")
    meta = g["meta"]
    assert not meta["central"] and not meta["ngal_mode"]
    p = merged_params(meta["params"])
    ci = cosmo_inputs_from_golden(g, p)
    om = hmref.RefHaloModel(ci, g["zs"], g["ks"], g["ms"], p, mass_function=meta["mass_function"], mdef=meta["mdef"],
                            alpha_table=alpha_table)
    sets = hod_sets(alphasat=[p["hod_alphasat"], 1.3], Bcut=[p["hod_Bcut"], 0.4])
    assert sets.shape == (2, 6) and np.array_equal(sets[0], [p["hod_" + c] for c in sets.columns])
    l10 = g["hod_log10mthresh"][:, 0]
    occ = {k: [] for k in ("Nc", "Ns", "NsNsm1", "NcNs")}
    for row in sets:
        ps = dict(p)
        ps.update({"hod_" + c: float(v) for c, v in zip(sets.columns, row)})
        for k, v in zip(occ, hmref.hod_occupations(om.ms, om.zs, l10, ps, meta["corr"])):
            occ[k].append(v)
    occ = {k: np.stack(v) for k, v in occ.items()}
    ref = hm.ensemble(om.nzm, om.bh, om.ms, om.ks, om.Pzk, ci.rho_matter_0, om.uk_profiles["nfw"], om.uk_profiles["nfw"],
                      occ, p["kstar_damping"])
    golden = {"gg_1h": g["P1h_g_g"], "gg_2h": g["P2h_g_g"], "gm_1h": g["P1h_nfw_g"], "gm_2h": g["P2h_nfw_g"]}
    for key in hm.PLANES:
        val = ref[key][0]
        assert val.shape == (2,) + golden[key].shape
        ok, worst = power_close(val[0], golden[key])
        print(f"{key}: worst share of the gate {worst:.3g}")
        assert ok, (key, worst)
        ok, worst = power_close(val[1], val[0])
        assert not ok and worst > 1e3, (key, worst)                     # the second set is another model
        assert np.all(ref[key][1] >= 0) and np.all(np.isfinite(ref[key][1]))
    assert np.allclose(ref["ngal"][0][0], g["hod_ngal"], rtol=1e-11) and np.allclose(ref["bg"][0][0], g["hod_bg"], rtol=1e-11)
    # the same with the gas tensor as the matter leg, and at scattered nodes
    kidx = np.array([39, 3, 0, 17])
    ref_e = hm.ensemble(om.nzm, om.bh, om.ms, om.ks, om.Pzk, ci.rho_matter_0, om.uk_profiles["nfw"], g["uk_electron"], occ,
                        p["kstar_damping"], kindex=kidx)
    for key, gold in (("gm_1h", g["P1h_electron_g"]), ("gm_2h", g["P2h_electron_g"])):
        ok, worst = power_close(ref_e[key][0][0], gold[:, kidx], atol_frac=0.0)
        assert ok, (key, worst)


# ---------------------------------------------------------------- 2. hod_sets
def test_hod_sets_defaults_broadcasting_and_refusals():
    from hmvec_amd import default_params, hod_ensemble, hod_sets
    cols = hod_ensemble.COLUMNS
    assert cols == ("sig_log_mstellar", "alphasat", "Bsat", "betasat", "Bcut", "betacut")
    d = np.array([default_params["hod_" + c] for c in cols])
    one = hod_sets()
    assert one.shape == (1, 6) and one.dtype == np.float64 and np.array_equal(one[0], d) and one.columns == cols
    t = hod_sets(n=5, sig=0.3, alphasat=np.linspace(0.8, 1.2, 5))
    assert t.shape == (5, 6) and np.all(t[:, 0] == 0.3) and np.array_equal(t.column("alphasat"), np.linspace(0.8, 1.2, 5))
    assert np.array_equal(t[:, 2:], np.tile(d[2:], (5, 1)))
    assert np.array_equal(hod_sets(hod_Bsat=[1.0, 2.0]).column("Bsat"), [1.0, 2.0])           # S from the columns
    b = hod_sets(base={"hod_Bcut": 0.5, "betasat": 0.9, "H0": 70.0}, n=2)
    assert np.all(b.column("Bcut") == 0.5) and np.all(b.column("hod_betasat") == 0.9)
    assert np.array_equal(hod_sets(base=t[3])[0], t[3])
    assert np.array_equal(hod_sets(base=dict(default_params))[0], d)
    assert hod_sets(Bcut=0.0).column("Bcut")[0] == 0.0                                        # zero is allowed
    for bad in (dict(colour=1.0), dict(sig=0.0), dict(sig=-0.1), dict(Bsat=0.0), dict(Bcut=-1.0), dict(alphasat=np.nan),
                dict(betacut=np.inf), dict(n=3, alphasat=[1.0, 2.0]), dict(n=0), dict(alphasat=[[1.0]]),
                dict(sig=0.2, sig_log_mstellar=0.3), dict(base={"colour": 1.0}), dict(base=[1.0, 2.0]), dict(alphasat=[])):
        with pytest.raises(ValueError):
            hod_sets(**bad)
    with pytest.raises(ValueError):
        hod_ensemble.as_sets(np.ones((3, 5)))
    with pytest.raises(ValueError):
        hod_ensemble.as_sets(np.zeros((1, 6)))


# ---------------------------------------------------------------- 3. stencil and central differences
def test_stencil_rows_and_exact_differences_of_a_quadratic():
    from hmvec_amd import central_differences, hod_ensemble, stencil
    base = dict(sig=0.25, alphasat=1.0, Bsat=8.0, betasat=0.75, Bcut=1.5, betacut=0.5)       # all exact in binary
    steps = {"alphasat": 0.125, "log10mthresh": 0.0625, "sig": 0.03125, "hod_Bcut": 0.25}
    sets, plan = stencil(base, steps)
    b = np.array([base[c if c != "sig_log_mstellar" else "sig"] for c in hod_ensemble.COLUMNS])
    assert sets.shape == (9, 6) and plan.size == 9 and np.array_equal(sets[0], b)
    assert plan.params == ("alphasat", "log10mthresh", "sig_log_mstellar", "Bcut")
    assert plan.rows == {"alphasat": (1, 2), "log10mthresh": (3, 4), "sig_log_mstellar": (5, 6), "Bcut": (7, 8)}
    for p, (ip, im) in plan.rows.items():
        h = plan.steps[p]
        if p == "log10mthresh":
            assert np.array_equal(sets[ip], b) and np.array_equal(sets[im], b)
            assert plan.log10mthresh_offset[ip] == h and plan.log10mthresh_offset[im] == -h
            continue
        j = hod_ensemble.COLUMNS.index(p)
        assert sets[ip, j] == b[j] + h and sets[im, j] == b[j] - h
        assert np.array_equal(np.delete(sets[ip], j), np.delete(b, j)) and np.array_equal(np.delete(sets[im], j), np.delete(b, j))
        assert plan.log10mthresh_offset[ip] == 0.0 and plan.log10mthresh_offset[im] == 0.0
    # values that are a quadratic polynomial of (the six parameters, the threshold): central differences are exact
    rng = np.random.default_rng(5)
    x0 = np.append(b, 10.5)
    x = np.column_stack([np.asarray(sets), 10.5 + plan.log10mthresh_offset])
    A, L, c = rng.integers(-4, 5, (3, 7, 7)).astype(float), rng.integers(-4, 5, (3, 7)).astype(float), np.array([1.0, 2.0, 3.0])
    A = A + A.transpose(0, 2, 1)
    values = np.einsum("si,vij,sj->sv", x, A, x) + x @ L.T + c
    grad = 2.0 * np.einsum("vij,j->vi", A, x0) + L
    d = central_differences(values, plan)
    assert set(d) == set(plan.params)
    names = list(hod_ensemble.COLUMNS) + ["log10mthresh"]
    for p in plan.params:
        want = grad[:, names.index(p)]
        # every operand is a dyadic rational of a few bits: the polynomial and the difference quotient are exact
        assert d[p].shape == (3,) and np.array_equal(d[p], want), (p, d[p], want)
    with pytest.raises(ValueError):
        central_differences(values[:-1], plan)
    for bad in ({"alphasat": 0.0}, {"alphasat": -0.1}, {"colour": 0.1}, {"sig": 0.1, "sig_log_mstellar": 0.1},
                {"sig": 0.3}, {"Bcut": np.inf}):
        with pytest.raises(ValueError):
            stencil(base, bad)


# ---------------------------------------------------------------- 4. declarations and exports
@pytest.mark.parametrize("name,count", [("hmg_hod_ensemble", 16), ("hmg_hod_ensemble_power", 22)])
def test_entry_points_are_declared_and_bound(name, count):
    from hmvec_amd import _native as nat
    header = open(os.path.join(REPO, "include", "hmgrid.h")).read()
    m = re.search(r"\bint " + name + r"\(hmg_ctx\* ctx, int S, int nz, int nm, ([^;]*)\);", header)
    assert m, name
    declared = re.sub(r"/\*.*?\*/", "", m.group(0), flags=re.S)
    assert declared.count(",") + 1 == count == len(nat.SIGNATURES[name])
    assert int(re.search(r"#define HMG_ABI_VERSION (\d+)", header).group(1)) == 10 == nat.ABI_VERSION
    mk = open(os.path.join(REPO, "hmvec_amd", "csrc", "Makefile")).read()
    assert re.search(r"^KUNITS = .*\bhodens\b", mk, flags=re.M)
    deps = re.search(r"^DEPS_hodens\s*=(.*)$", mk, flags=re.M)
    assert deps and "kernels/hodens.hpp" in deps.group(1) and "kernels/hod_occ.hpp" in deps.group(1)
    csrc = os.path.join(REPO, "hmvec_amd", "csrc")
    assert os.path.exists(os.path.join(csrc, "hodens.hip")) and os.path.exists(os.path.join(csrc, "kernels", "hodens.hpp"))
    hod = open(os.path.join(csrc, "kernels", "hod.hpp")).read()
    occ = open(os.path.join(csrc, "kernels", "hod_occ.hpp")).read()
    assert '#include "hod_occ.hpp"' in hod and "__global__" in hod and "__global__" not in occ    # a kernel lives in one unit
    assert "hod_occ_point" in occ and "hod_sums_row" in occ


def test_exports_and_method_signatures():
    import hmvec_amd
    from hmvec_amd import hod_ensemble
    for name in ("hod_sets", "stencil", "central_differences"):
        assert getattr(hmvec_amd, name) is getattr(hod_ensemble, name)
        assert name in hmvec_amd.__all__ and name in hod_ensemble.__all__
    assert hmvec_amd.hod_ensemble is hod_ensemble and "hod_ensemble" in hmvec_amd.__all__
    assert list(inspect.signature(hod_ensemble.hod_sets).parameters) == ["n", "base", "columns"]
    assert list(inspect.signature(hod_ensemble.stencil).parameters) == ["base", "steps"]
    assert list(inspect.signature(hod_ensemble.central_differences).parameters) == ["values", "plan"]
    want = {"self": inspect.Parameter.empty, "sets": inspect.Parameter.empty, "mthresh": None, "ngal": None, "corr": "max",
            "satellite_profile_name": "nfw", "matter_name": None, "kindex": None, "damping": True, "parts": False}
    for name in ("hod_ensemble_device", "get_power_hod_ensemble"):
        par = inspect.signature(getattr(hmvec_amd.HaloModel, name)).parameters
        assert {k: v.default for k, v in par.items()} == want and list(par) == list(want), name
    par = inspect.signature(hmvec_amd.HaloModel.hod_ensemble_occupations).parameters
    assert list(par) == ["self", "sets", "mthresh", "ngal", "corr"] and par["corr"].default == "max"
    hpp = open(os.path.join(REPO, "hmvec_amd", "csrc", "kernels", "hodens.hpp")).read()
    assert int(re.search(r"constexpr int HE_TS = (\d+);", hpp).group(1)) == hod_ensemble.SET_TILE     # one padding rule
    assert hod_ensemble.coef_block_size(11, 3, 70) == 4 * 3 * 70 * 16 + 11 * 3
    assert hod_ensemble.coef_block_size(8, 2, 5) == 4 * 2 * 5 * 8 + 8 * 2


def test_request_checks_refuse_on_the_host():
    from hmvec_amd import hod_ensemble as he
    assert he.check_kindex(None, 10) is None
    assert he.check_kindex([9, 0, 3, 3], 10).dtype == np.int32
    for bad in ([10], [-1], [], [[1]], [0.5]):
        with pytest.raises(ValueError):
            he.check_kindex(bad, 10)
    assert he.per_set(np.ones(3), 4, 3, "ngal").shape == (4, 3) and he.per_set(np.ones((4, 3)), 4, 3, "ngal").flags.c_contiguous
    for bad in (np.ones(4), np.ones((3, 4)), np.zeros(3), -np.ones(3), np.full(3, np.nan), 1.0):
        with pytest.raises(ValueError):
            he.per_set(bad, 4, 3, "mthresh")
    assert he.check_corr("max") == 0 and he.check_corr("min") == 1
    with pytest.raises(ValueError):
        he.check_corr("both")
    # one step of the bisection: only the active sets move, and they move as utils.vectorized_bisection_search does
    lo, hi = np.zeros((2, 2)), np.ones((2, 2))
    mid = (lo + hi) / 2
    he.bisection_step(lo, hi, mid, np.array([[0.1, -0.1], [0.1, -0.1]]), np.array([True, False]))
    assert np.array_equal(lo, [[0.5, 0.0], [0.0, 0.0]]) and np.array_equal(hi, [[1.0, 0.5], [1.0, 1.0]])
