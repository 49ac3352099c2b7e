"""kSZ forecasts on the GPU (hmvec_amd.ksz, kernels/ksz.hpp): every case of tests/golden/ksz.npz end to end against
the unmodified reference on the same tabulated P(k) (tests/helpers/pk_table.py), the three kernels against their
numpy definitions (tests/test_ksz_cpu.py), batching, determinism, a grid that is not log-uniform, the P_q_perp
kernel's route for tables too large for LDS, and input validation."""
import os
import sys

import numpy as np
import pytest

from conftest import load_golden, merged_params
from test_ksz_cpu import cl_prefactors, limber_def, nvv_def, pqperp_def

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import pk_table  # noqa: E402

pytestmark = pytest.mark.gpu

RTOL = 1e-9


@pytest.fixture(scope="module")
def g():
    return load_golden("ksz")


def provider():
    import hmvec_amd as hm
    p = merged_params()
    return hm.TabulatedBackground(p, *pk_table.table(p["ns"]))


def grid(g):
    gr = dict(g["meta"]["grid"])
    return gr


def worst(got, ref, scale=None):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    scale = np.abs(ref) if scale is None else scale
    return float(np.max(np.abs(got - ref) / np.maximum(scale, 1e-300)))


@pytest.fixture(scope="module")
def models(g):
    from hmvec_amd.ksz import kSZ
    out = {}
    for tag, sigz in (("a", None), ("b", g["meta"]["sigz"])):
        out[tag] = kSZ(g["zs"], g["meta"]["vol"] * np.ones(3), g["ngals"], ms=g["ms"], sigz=sigz,
                       background=provider(), **grid(g))
    return out


@pytest.fixture(scope="module")
def auto_model(g):
    from hmvec_amd.ksz import get_kmin, kSZ
    m = g["meta"]
    vol = m["vol"]
    return kSZ(g["zs"], vol * np.ones(3), g["ngals"], kL_max=m["kmax_auto"], num_kL_bins=m["nk_auto"],
               kS_min=get_kmin(vol), kS_max=m["kmax_auto"], num_kS_bins=m["nk_auto"], num_mu_bins=m["nmu_auto"],
               ms=g["ms"], background=provider())


# ------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize("tag", ["a", "b"])
def test_ksz_model_and_nvv_match_reference(g, models, tag):
    k = models[tag]
    assert np.allclose(k.bgs, g[tag + "_bgs"], rtol=RTOL, atol=0), worst(k.bgs, g[tag + "_bgs"])
    assert np.allclose([f[0] for f in k.fs], g[tag + "_fs"], rtol=1e-13, atol=0)
    assert np.allclose(k.chistars, g[tag + "_chistars"], rtol=1e-14, atol=0)
    vrec = np.array([np.asarray(v) for v in k.vrec])
    assert vrec.shape == g[tag + "_vrec"].shape
    assert np.allclose(vrec, g[tag + "_vrec"], rtol=RTOL, atol=0), worst(vrec, g[tag + "_vrec"])
    Cls = g["Cls"].copy()
    for iz in range(g["zs"].size):
        N = k.Nvv(iz, Cls)
        assert N.shape == g[tag + "_Nvv"][iz].shape
        assert np.allclose(N, g[tag + "_Nvv"][iz], rtol=RTOL, atol=0), (iz, worst(N, g[tag + "_Nvv"][iz]))
    if tag == "a":
        for iz in range(g["zs"].size):
            e = k.Pge_err(iz, g["a_Pge_err_edges"], g["Cls"].copy())
            assert np.allclose(e, g["a_Pge_err"][iz], rtol=RTOL, atol=0), worst(e, g["a_Pge_err"][iz])
    else:
        nmu, nkL = k.mu.size, k.kLs.size
        assert k.lPgg(0, 1.0, 1.0).shape == (nmu, nkL, 1) and k.lPgv(0, 1.0).shape == (nmu, nkL, 1)
        assert np.shape(k.vrec[0]) == (nkL,)            # (kL,1) spectra against (kL,) weights: an array


@pytest.mark.parametrize("tag", ["a", "b"])
def test_snr_matches_reference(g, tag):
    from hmvec_amd.ksz import get_ksz_snr
    sigz = g["meta"]["sigz"] if tag == "b" else None
    snr, _ = get_ksz_snr(g["meta"]["vol"], g["zs"][1], g["ngals"][1], g["Cls"].copy(), ms=g["ms"], sigz=sigz,
                         background=provider(), **grid(g))
    assert np.allclose(np.ravel(snr), g[tag + "_snr"], rtol=RTOL, atol=0), worst(snr, g[tag + "_snr"])


def test_mafry_and_squeezed_cl_match_reference(g, auto_model, tmp_path, monkeypatch):
    from hmvec_amd.ksz import get_ksz_auto_signal_mafry, get_ksz_auto_squeezed
    monkeypatch.chdir(tmp_path)
    os.mkdir("debug_files")
    _, cl = get_ksz_auto_signal_mafry(g["ells"], g["meta"]["vol"], g["zs"], g["ngals"][0], None,
                                      pksz_in=auto_model, save_debug_files=True)
    P = np.loadtxt("debug_files/pqperp.dat").reshape(g["c_pqperp"].shape)
    _, Pabs = pqperp_def(g["c_ks"], g["c_mus"], g["c_Pee"], g["c_Pmm"], g["c_adotf"])
    assert worst(P, g["c_pqperp"], Pabs) <= RTOL
    assert np.allclose(cl, g["c_cl"], rtol=RTOL, atol=0), worst(cl, g["c_cl"])
    assert cl[-1] < 0
    _, cl2, spec = get_ksz_auto_squeezed(g["ells"], g["meta"]["vol"], g["zs"], g["ngals"], np.ones(3),
                                         pksz_in=auto_model, save_debug_files=True)
    Pqr = np.loadtxt("debug_files/pqr.dat").reshape(g["d_pqr"].shape)
    assert np.allclose(Pqr, g["d_pqr"], rtol=RTOL, atol=0), worst(Pqr, g["d_pqr"])
    assert np.allclose(cl2, g["d_cl"], rtol=RTOL, atol=0), worst(cl2, g["d_cl"])
    assert set(spec) == {"ks", "sPee", "lPvv"}


def test_template_signal_matches_reference(g):
    from hmvec_amd.ksz import get_ksz_template_signal_snapshot
    cl, fk, pk = get_ksz_template_signal_snapshot(g["ells"][:5], g["meta"]["vol"], g["zs"][1], g["ngals"][1],
                                                  g["meta"]["bg_template"], ms=g["ms"], background=provider(),
                                                  **grid(g))
    assert fk is pk
    assert np.allclose(cl, g["e_cl"], rtol=RTOL, atol=0), worst(cl, g["e_cl"])


# ------------------------------------------------------------------------------------------ kernels vs definitions
def test_pqperp_kernel_matches_definition(g):
    from hmvec_amd.ksz import pqperp_table
    P = pqperp_table(g["c_ks"], g["c_mus"], g["c_Pee"], g["c_Pmm"], g["c_adotf"])
    ref, Pabs = pqperp_def(g["c_ks"], g["c_mus"], g["c_Pee"], g["c_Pmm"], g["c_adotf"])
    assert worst(P, ref, Pabs) <= 1e-12
    assert worst(P, g["c_pqperp"], Pabs) <= 1e-12


def _synthetic_pq(ks, nz=2, seed=3):
    rng = np.random.default_rng(seed)
    x = ks / 0.05
    Pee = np.array([1e3 * x / (1 + x ** 2.2) * (1 + 0.1 * i) for i in range(nz)]) * (1 + 0.01 * rng.random((nz, 1)))
    Pmm = np.array([2e4 * x / (1 + x ** 2.9) * (1 - 0.1 * i) for i in range(nz)])
    return Pee, Pmm, np.linspace(40.0, 60.0, nz)


def test_pqperp_non_log_uniform_grid_and_lds_fallback():
    from hmvec_amd.ksz import pqperp_table
    ks = np.unique(np.concatenate([np.geomspace(1e-3, 50.0, 90), np.linspace(0.05, 2.0, 70)]))
    mus = np.linspace(-1.0, 1.0, 17)
    Pee, Pmm, adotf = _synthetic_pq(ks)
    P = pqperp_table(ks, mus, Pee, Pmm, adotf)
    ref, Pabs = pqperp_def(ks, mus, Pee, Pmm, adotf)
    assert worst(P, ref, Pabs) <= 1e-12
    # (nmu + 3 nk) doubles above 48 KiB: the kernel reads the tables from global memory
    ks = np.geomspace(1e-3, 50.0, 2100)
    mus = np.linspace(-1.0, 1.0, 6)
    Pee, Pmm, adotf = _synthetic_pq(ks, nz=1)
    P = pqperp_table(ks, mus, Pee, Pmm, adotf)
    ref, Pabs = pqperp_def(ks, mus, Pee, Pmm, adotf)
    assert worst(P, ref, Pabs) <= 1e-12


def test_nvv_kernel_general_rows_errs_and_robust(g, capsys):
    from hmvec_amd.ksz import Nvv_core_integral
    mus, kLs, kS = g["b_mu"], g["b_kLs"], g["b_kS"]
    chi, F = g["b_chistars"][0], g["b_kstars"][0]
    sig, H = g["meta"]["sigz"] * (1 + g["zs"][0]), g["b_in_Hphoto"][0]
    kr = mus[:, None] * kLs[None, :]
    W = np.exp(-sig ** 2 * kr ** 2 / 2 / H ** 2)[..., None]
    Pge = g["b_in_Pge"][0] * W
    Pgg = g["b_in_Pgg"][0] * W ** 2 + 1 / g["ngals"][0]
    N = Nvv_core_integral(chi, F, mus, kLs, kS, g["Cls"].copy(), Pge, Pgg)
    ref = nvv_def(chi, F, mus, kLs, kS, g["Cls"].copy(), Pge, Pgg, 0.0)
    assert np.allclose(N, ref, rtol=1e-12, atol=0)
    N1, ret = Nvv_core_integral(chi, F, mus, kLs, kS, g["Cls"].copy(), Pge, Pgg, errs=True)
    assert ret is not Pge and np.array_equal(ret, Pge)
    assert np.allclose(N1, nvv_def(chi, F, mus, kLs, kS, g["Cls"].copy(), 1.0, Pgg, 0.0), rtol=1e-12, atol=0)
    Pph = Pgg * 1.3
    N2 = Nvv_core_integral(chi, F, mus, kLs, kS, g["Cls"].copy(), Pge, Pgg, Pgg_photo_tot=Pph, robust_term=True)
    assert "WARNING: photo_zs were True" in capsys.readouterr().out
    assert np.allclose(N2, ref / 1.3, rtol=1e-12, atol=0)


def test_limber_kernel_matches_definition(g):
    from hmvec_amd.ksz import limber_cl
    c2, T2 = cl_prefactors(g)
    for P, sq in ((g["c_pqperp"], False), (g["d_pqr"], True)):
        got = limber_cl(g["ells"], g["c_chi_nodes"], g["c_z_nodes"], g["zs"], g["c_ks"], P, sq, c2, T2)
        ref = limber_def(g["ells"], g["c_chi_nodes"], g["c_z_nodes"], g["zs"], g["c_ks"], P, sq, c2, T2)
        assert np.allclose(got, ref, rtol=1e-12, atol=0)


# ------------------------------------------------------------------------------------------ batching, determinism
def test_batches_equal_single_calls_bit_for_bit(g, models):
    from hmvec_amd.ksz import limber_cl, pqperp_table
    P = pqperp_table(g["c_ks"], g["c_mus"], g["c_Pee"], g["c_Pmm"], g["c_adotf"])
    for iz in range(3):
        one = pqperp_table(g["c_ks"], g["c_mus"], g["c_Pee"][iz:iz + 1], g["c_Pmm"][iz:iz + 1], g["c_adotf"][iz:iz + 1])
        assert np.array_equal(one[:, 0], P[:, iz])
    for tag in ("a", "b"):
        k = models[tag]
        batch = k._nvv([0, 1, 2], g["Cls"].copy())
        for iz in range(3):
            assert np.array_equal(batch[iz], k.Nvv(iz, g["Cls"].copy()))
    c2, T2 = cl_prefactors(g)
    cl = limber_cl(g["ells"], g["c_chi_nodes"], g["c_z_nodes"], g["zs"], g["c_ks"], g["c_pqperp"], False, c2, T2)
    for i in range(g["ells"].size):
        one = limber_cl(g["ells"][i:i + 1], g["c_chi_nodes"][i:i + 1], g["c_z_nodes"][i:i + 1], g["zs"], g["c_ks"],
                        g["c_pqperp"], False, c2, T2)
        assert one[0] == cl[i]


def test_repeated_calls_are_bit_identical(g, models):
    from hmvec_amd.ksz import pqperp_table
    a = pqperp_table(g["c_ks"], g["c_mus"], g["c_Pee"], g["c_Pmm"], g["c_adotf"])
    b = pqperp_table(g["c_ks"], g["c_mus"], g["c_Pee"], g["c_Pmm"], g["c_adotf"])
    assert np.array_equal(a, b)
    k = models["b"]
    assert np.array_equal(k.Nvv(1, g["Cls"].copy()), k.Nvv(1, g["Cls"].copy()))


# ------------------------------------------------------------------------------------------ validation and quirks
def test_nvv_zeroes_the_callers_cls(g, models):
    Cls = g["Cls"].copy()
    assert Cls[0] != 0 and Cls[1] != 0
    models["a"].Nvv(0, Cls)
    assert Cls[0] == 0 and Cls[1] == 0 and Cls[2] == g["Cls"][2]


def test_input_validation(g, models):
    from hmvec_amd.ksz import Nvv_core_integral, get_ksz_auto_signal_mafry, kSZ, limber_cl, pqperp_table
    ks, mus = g["c_ks"], g["c_mus"]
    with pytest.raises(ValueError):
        pqperp_table(ks, mus, g["c_Pee"][:, :-1], g["c_Pmm"], g["c_adotf"])
    with pytest.raises(ValueError):
        pqperp_table(ks[::-1], mus, g["c_Pee"], g["c_Pmm"], g["c_adotf"])
    c2, T2 = cl_prefactors(g)
    with pytest.raises(ValueError):           # one redshift: no (z, k) interpolation
        limber_cl(g["ells"], g["c_chi_nodes"], g["c_z_nodes"], g["zs"][:1], ks, g["c_pqperp"][:, :1], False, c2, T2)
    with pytest.raises(ValueError):
        limber_cl(g["ells"], g["c_chi_nodes"][:, :5], g["c_z_nodes"], g["zs"], ks, g["c_pqperp"], False, c2, T2)
    k = models["a"]
    with pytest.raises(ValueError):
        Nvv_core_integral(1000.0, 1.0, k.mu, k.kLs, k.kS, g["Cls"].copy(), np.ones(7), np.ones(7))
    mu0 = np.linspace(-1.0, 1.0, 5)            # mu = 0: infinite N_vv, the reference's assert
    with pytest.raises(AssertionError):
        Nvv_core_integral(1000.0, 1.0, mu0, k.kLs, k.kS, g["Cls"].copy(), np.ones(k.kS.size),
                          np.ones(k.kS.size))
    with pytest.raises(AssertionError):        # the reference's kSZ.__init__: mthreshs_override with ngal
        kSZ(g["zs"][:1], [1.0], g["ngals"][:1], ms=g["ms"], mthreshs_override=np.array([1e12]),
            background=provider(), **grid(g))
    with pytest.raises(ValueError):
        get_ksz_auto_signal_mafry(g["ells"], 1.0, [0.5], 1e-4, None, pksz_in=kSZ(
            [0.5], [1.0], [1e-4], ms=g["ms"], kL_max=100.0, num_kL_bins=40, kS_min=0.01, kS_max=100.0,
            num_kS_bins=40, num_mu_bins=8, background=provider()))
