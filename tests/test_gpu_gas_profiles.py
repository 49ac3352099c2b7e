"""Projected gas and pressure profiles on the GPU against the independent quadrature model of
tests/helpers/gas_profile_model.py.

Gates.  The core gate of a kind is max(1e-10, 100 x the worst relative error of the CPU prototype of the kernels' rule
over the grid of test 1) and never looser than 1e-8.  The prototype (tools/gas_profile_prototype.py: the same nodes, maps
and formulas in numpy, libm instead of the short device functions) measures 8.3e-16 for "sigma", 7.0e-12 for "mean" and
7.0e-12 for "excess" against the model, so the gates are 1e-10, 7e-10 and 7e-10.  The smoothing gate is 1e-6 (the gate
of the miscentred NFW profile, the same integral structure); its prototype measures 9.7e-12 over the points of test 3.
Measured on an MI355X: see DESIGN.md section 18."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import gas_profile_model as gm  # noqa: E402

pytestmark = pytest.mark.gpu

PROTOTYPE_ERROR = {"sigma": 8.3e-16, "mean": 7.0e-12, "excess": 7.0e-12}
GATE = {k: min(1e-8, max(1e-10, 100.0 * e)) for k, e in PROTOTYPE_ERROR.items()}
SMOOTH_GATE = 1e-6
KINDS = ("sigma", "mean", "excess")

# (alpha, eta, gamma): two gas-like and two pressure-like rows
ROWS = [(0.88, 4.125, -0.2), (0.70, 6.04, -0.2), (1.0, 4.35, -0.3), (1.0, 6.0, -0.3)]
XCUTS = (2.0, 4.0, 20.0, 200.0)


def radii(xcut):
    return np.array([1e-3, 1e-2, 0.1, 0.5, 1.0, 1.9, 0.999 * xcut, xcut, 1.5 * xcut])


def relerr(got, ref):
    got, ref = np.asarray(got, float), np.asarray(ref, float)
    return np.where(ref != 0.0, np.abs(got - ref) / np.where(ref != 0.0, np.abs(ref), 1.0), np.abs(got))


@pytest.fixture(scope="module")
def core_reference():
    """{(kind, gamma): (alpha, eta, xcut, x, ref)} over rows x xcuts x radii, computed once."""
    out = {}
    for gamma in (-0.2, -0.3):
        al, et, xc, x = [], [], [], []
        for a, e, g in ROWS:
            if g != gamma:
                continue
            for c in XCUTS:
                al.append(a), et.append(e), xc.append(c), x.append(radii(c))
        al, et, xc, x = np.array(al), np.array(et), np.array(xc), np.array(x)
        F = np.array([[gm.F_proj(s, a, gamma, e, c) for s in row] for a, e, c, row in zip(al, et, xc, x)])
        G = np.array([[gm.G_mean(s, a, gamma, e, c) for s in row] for a, e, c, row in zip(al, et, xc, x)])
        for kind, ref in (("sigma", F), ("mean", G), ("excess", G - F)):
            out[kind, gamma] = (al, et, xc, x, ref)
    return out


# ---------------------------------------------------------------- 1. the core against the model
@pytest.mark.parametrize("gamma", [-0.2, -0.3])
@pytest.mark.parametrize("kind", KINDS)
def test_core_matches_the_quadrature_model(core_reference, kind, gamma):
    from hmvec_amd import projected_gnfw
    al, et, xc, x, ref = core_reference[kind, gamma]
    got = projected_gnfw(x, al, gamma, et, xc, kind=kind)
    err = relerr(got, ref)
    i, j = np.unravel_index(np.argmax(err), err.shape)
    print(f"{kind} gamma={gamma}: worst relative error {err.max():.3e} at alpha={al[i]} eta={et[i]} xcut={xc[i]} "
          f"s={x[i, j]:.4g} (gate {GATE[kind]:.1e})")
    assert np.all(np.isfinite(got))
    assert err.max() <= GATE[kind]


# ---------------------------------------------------------------- 2. exact conditions
def test_zero_beyond_the_cut_and_the_total_inside(core_reference):
    from hmvec_amd import projected_gnfw
    al, et, xc, x, _ = core_reference["sigma", -0.2]
    F = projected_gnfw(x, al, -0.2, et, xc, kind="sigma")
    G = projected_gnfw(x, al, -0.2, et, xc, kind="mean")
    beyond = x >= xc[:, None]
    assert beyond.sum() == 2 * len(al)
    assert np.all(F[beyond] == 0.0) and np.all(F[~beyond] > 0.0)
    N = np.array([gm.N_total(a, -0.2, e, c) for a, e, c in zip(al, et, xc)])
    err = relerr(G[beyond], (N[:, None] / (np.pi * x ** 2))[beyond])
    print(f"G beyond the cut against N / pi s^2: worst relative error {err.max():.3e}")
    assert err.max() <= GATE["mean"]


def test_excess_is_mean_minus_sigma_and_repeats_bit_for_bit(core_reference):
    from hmvec_amd import projected_gnfw
    for gamma in (-0.2, -0.3):
        al, et, xc, x, _ = core_reference["sigma", gamma]
        F, G, E = (projected_gnfw(x, al, gamma, et, xc, kind=k) for k in KINDS)
        assert np.array_equal(E, G - F)
        for k, first in zip(KINDS, (F, G, E)):
            assert np.array_equal(projected_gnfw(x, al, gamma, et, xc, kind=k), first)
        sm = projected_gnfw(x, al, gamma, et, xc, smooth=0.3)
        assert np.array_equal(projected_gnfw(x, al, gamma, et, xc, smooth=0.3), sm)


def test_shared_radii_equal_per_row_radii():
    from hmvec_amd import projected_gnfw
    al, et, xc = np.array([0.88, 0.7, 0.95]), np.array([4.125, 6.04, 5.0]), np.array([3.0, 4.0, 1.7])
    x = np.array([1e-3, 0.04, 0.7, 1.6999, 1.7, 2.5, 3.5, 5.0])
    for kind in KINDS:
        assert np.array_equal(projected_gnfw(x, al, -0.2, et, xc, kind=kind),
                              projected_gnfw(np.tile(x, (3, 1)), al, -0.2, et, xc, kind=kind))
    assert np.array_equal(projected_gnfw(x, al, -0.2, et, xc, smooth=[0.2, 0.0, 1.0]),
                          projected_gnfw(np.tile(x, (3, 1)), al, -0.2, et, xc, smooth=[0.2, 0.0, 1.0]))


def test_a_row_of_a_batch_equals_the_row_alone():
    """257 rows x 5 radii: more than one workgroup of the per-output kernel (256 threads) and of the per-wavefront kernel
    (4 outputs), an odd number of radii, rows that end in the middle of a wavefront."""
    from hmvec_amd import projected_gnfw
    rng = np.random.default_rng(7)
    n = 257
    al = np.where(np.arange(n) % 3 == 0, 1.0, rng.uniform(0.6, 1.3, n))
    et = rng.uniform(3.0, 7.0, n)
    xc = rng.uniform(1.5, 30.0, n)
    x = xc[:, None] * np.array([1e-3, 0.03, 0.4, 0.97, 1.2])[None, :] * rng.uniform(0.9, 1.0, (n, 1))
    sig = rng.uniform(0.05, 2.0, n)
    picks = (0, 1, 51, 52, 63, 64, 255, 256)
    for kind in KINDS:
        full = projected_gnfw(x, al, -0.25, et, xc, kind=kind)
        assert np.all(np.isfinite(full))
        for i in picks:
            assert np.array_equal(projected_gnfw(x[i:i + 1], al[i], -0.25, et[i], xc[i], kind=kind)[0], full[i]), (kind, i)
    full = projected_gnfw(x, al, -0.25, et, xc, smooth=sig)
    assert np.all(np.isfinite(full)) and np.all(full[:, :4] > 0.0)
    for i in picks:
        assert np.array_equal(projected_gnfw(x[i:i + 1], al[i], -0.25, et[i], xc[i], smooth=sig[i])[0], full[i]), i


def test_alpha_one_rows_agree_with_the_general_evaluation(core_reference, monkeypatch):
    from hmvec_amd import gasprofiles
    for kind in KINDS:
        al, et, xc, x, ref = core_reference[kind, -0.3]
        assert np.all(al == 1.0)
        short = gasprofiles.projected_gnfw(x, al, -0.3, et, xc, kind=kind)
        monkeypatch.setattr(gasprofiles, "_force_general", True)
        general = gasprofiles.projected_gnfw(x, al, -0.3, et, xc, kind=kind)
        monkeypatch.setattr(gasprofiles, "_force_general", False)
        err = relerr(short, general)
        print(f"{kind}: alpha == 1 evaluation against the general one, worst relative difference {err.max():.3e}")
        assert err.max() <= GATE[kind]
        assert relerr(general, ref).max() <= GATE[kind]


# ---------------------------------------------------------------- 3. smoothing
SMOOTH_ROWS = [(0.88, 4.125, -0.2, 4.0), (1.0, 4.35, -0.3, 2.0)]
SMOOTH_SIGMAS = (0.05, 0.5, 5.0)


def smooth_radii(xcut):
    return np.array([0.01, 0.3, 1.0, 0.95 * xcut, 1.3 * xcut])


@pytest.fixture(scope="module")
def smooth_reference():
    return {(row, sig): np.array([gm.F_smooth(s, sig, row[0], row[2], row[1], row[3]) for s in smooth_radii(row[3])])
            for row in SMOOTH_ROWS for sig in SMOOTH_SIGMAS}


def test_smoothed_projection_matches_the_nested_quadrature(smooth_reference):
    from hmvec_amd import projected_gnfw
    worst = 0.0
    for (row, sig), ref in smooth_reference.items():
        a, e, g, c = row
        got = projected_gnfw(smooth_radii(c), a, g, e, c, smooth=sig)[0]
        err = relerr(got, ref)
        print(f"alpha={a} xcut={c} sigma={sig}: relative errors {np.array2string(err, precision=2)}")
        worst = max(worst, err.max())
        assert np.all(got[ref == 0.0] == 0.0)              # s - 10 sigma beyond the cut
    print(f"smoothing: worst relative error {worst:.3e} (gate {SMOOTH_GATE:.0e})")
    assert worst <= SMOOTH_GATE


def test_rows_without_a_width_take_the_unsmoothed_route():
    from hmvec_amd import projected_gnfw
    al, et, xc = np.array([0.88, 0.7, 0.95, 0.8]), np.array([4.125, 6.04, 5.0, 4.5]), np.array([3.0, 4.0, 1.7, 2.2])
    x = np.array([0.01, 0.3, 1.0, 1.65, 2.9, 4.5])
    sig = np.array([0.0, 0.4, 0.0, 1.5])
    mixed = projected_gnfw(x, al, -0.2, et, xc, smooth=sig)
    plain = projected_gnfw(x, al, -0.2, et, xc)
    smooth = projected_gnfw(x, al, -0.2, et, xc, smooth=np.where(sig > 0, sig, 0.7))
    assert np.array_equal(mixed[sig == 0], plain[sig == 0])
    assert np.array_equal(mixed[sig > 0], smooth[sig > 0])
    assert not np.array_equal(mixed[sig > 0], plain[sig > 0])
    assert np.array_equal(projected_gnfw(x, al, -0.2, et, xc, smooth=0.0), plain)


def test_a_narrow_beam_returns_the_profile():
    from hmvec_amd import projected_gnfw
    for a, e, g, c in SMOOTH_ROWS:
        x = np.array([0.3, 1.0, 0.5 * c])
        narrow = projected_gnfw(x, a, g, e, c, smooth=1e-4)[0]
        plain = projected_gnfw(x, a, g, e, c)[0]
        err = relerr(narrow, plain)
        print(f"alpha={a}: sigma = 1e-4 against the unsmoothed profile, relative differences {err}")
        assert err.max() <= SMOOTH_GATE


# ---------------------------------------------------------------- 4. the HaloModel methods
ZS = np.array([0.3, 0.9])
MS_HALO = np.array([3.3e13, 2.1e14, 7.7e14])
THETAS = np.geomspace(0.3, 30.0, 5) * np.pi / 180.0 / 60.0


def small_model(zs):
    import hmvec_amd as hm
    return hm.HaloModel(np.atleast_1d(zs), np.geomspace(1e-3, 10.0, 32), ms=np.geomspace(1e11, 1e16, 16), accuracy="low",
                        engine="analytic")


@pytest.fixture(scope="module")
def model():
    return small_model(ZS)


def gas_pp(family="AGN", **over):
    from hmvec_amd import battaglia_defaults, default_params
    pp = dict(battaglia_defaults[family], battaglia_gas_gamma=default_params["battaglia_gas_gamma"])
    pp.update(over)
    return pp


def pres_pp(**over):
    from hmvec_amd import battaglia_defaults, default_params
    pp = dict(battaglia_defaults[default_params["battaglia_pres_family"]],
              battaglia_pres_gamma=default_params["battaglia_pres_gamma"],
              battaglia_pres_alpha=default_params["battaglia_pres_alpha"])
    pp.update(over)
    return pp


def model_reference(h, rows_of, pp, kind="sigma", scale=1.0, Ms=MS_HALO, thetas=THETAS, **kw):
    return scale * np.array([[[gm.profile(rows_of(h, iz, M, pp), t, kind=kind, **kw) for t in thetas] for M in Ms]
                             for iz in range(h.zs.size)])


def test_halo_model_profiles_match_the_model(model):
    h = model
    cases = [
        ("gas_sigma", h.gas_sigma_1h_profiles(THETAS, MS_HALO), model_reference(h, gm.gas_rows, gas_pp()), "sigma"),
        ("gas_delta_sigma", h.gas_delta_sigma_1h_profiles(THETAS, MS_HALO),
         model_reference(h, gm.gas_rows, gas_pp(), kind="excess"), "excess"),
        ("tau", h.tau_1h_profiles(THETAS, MS_HALO), model_reference(h, gm.gas_rows, gas_pp(), scale=gm.tau_factor()),
         "sigma"),
        ("y", h.y_1h_profiles(THETAS, MS_HALO), model_reference(h, gm.pres_rows, pres_pp()), "sigma"),
    ]
    for name, got, ref, kind in cases:
        assert got.shape == (2, 3, 5)
        err = relerr(got, ref)
        print(f"{name}: worst relative error {err.max():.3e} (gate {10 * GATE[kind]:.1e}); values {got.min():.3e} .. "
              f"{got.max():.3e}")
        assert np.array_equal(got == 0.0, ref == 0.0) and np.all(got[:, :, 0] > 0.0)     # zero beyond the cut, exactly
        assert err.max() <= 10.0 * GATE[kind]


def test_halo_model_options(model):
    h = model
    # given concentrations, another family, a cut inside the virial radius
    concs = np.array([6.0, 5.0, 4.0])
    got = h.gas_sigma_1h_profiles(THETAS, MS_HALO, concs=concs, family="SH", truncate=0.8)
    ref = np.array([[[gm.profile(gm.gas_rows(h, iz, M, gas_pp("SH"), conc=c, truncate=0.8), t) for t in THETAS]
                     for M, c in zip(MS_HALO, concs)] for iz in range(2)])
    assert relerr(got, ref).max() <= 10.0 * GATE["sigma"]
    # overrides: the named fit numbers change the result as the model predicts, other keys are ignored
    over = dict(rho0_A0=5000.0, alpha_alpham=-0.01, battaglia_gas_gamma=-0.3, not_a_parameter=1.0)
    got_o = h.gas_sigma_1h_profiles(THETAS, MS_HALO, param_override=over)
    known = {k: v for k, v in over.items() if k != "not_a_parameter"}
    err = relerr(got_o, model_reference(h, gm.gas_rows, gas_pp(**known)))
    print(f"gas_sigma with overrides: worst relative error {err.max():.3e}")
    assert err.max() <= 10.0 * GATE["sigma"]
    assert relerr(got_o, h.gas_sigma_1h_profiles(THETAS, MS_HALO))[:, :, 0].min() > 1e-3       # (inside the cut)
    over = dict(P0_A0=20.0, battaglia_pres_alpha=1.2, battaglia_pres_gamma=-0.4)
    err = relerr(h.y_1h_profiles(THETAS, MS_HALO, param_override=over), model_reference(h, gm.pres_rows, pres_pp(**over)))
    print(f"y with overrides (alpha = 1.2): worst relative error {err.max():.3e}")
    assert err.max() <= 10.0 * GATE["sigma"]


def test_mass_normalisation_holds_the_halo_mass(model):
    """norm="mass": the mean surface density inside a disc beyond the cut, times the disc's area, is the halo mass."""
    h = model
    worst = 0.0
    for iz in range(2):
        for i, M in enumerate(MS_HALO):
            _, da, _, rvir, _, _ = gm.halo_scalars(h, iz, M)
            theta = 1.001 * rvir / da
            sigma = h.gas_sigma_1h_profiles([theta], MS_HALO, norm="mass")[iz, i, 0]
            dsigma = h.gas_delta_sigma_1h_profiles([theta], MS_HALO, norm="mass")[iz, i, 0]
            assert sigma == 0.0
            worst = max(worst, abs(dsigma * np.pi * (da * theta) ** 2 / M - 1.0))
    print(f"norm='mass': worst relative error of the mass inside the cut {worst:.3e}")
    assert worst <= 10.0 * GATE["mean"]
    got = h.gas_sigma_1h_profiles(THETAS, MS_HALO, norm="mass")
    ref = model_reference(h, gm.gas_rows, gas_pp(), norm="mass")
    assert relerr(got, ref).max() <= 10.0 * GATE["mean"]


def test_beam_on_tau_and_y(model):
    h = model
    fwhm = 1.4 * np.pi / 180.0 / 60.0
    Ms, th = MS_HALO[1:2], THETAS[[0, 3]]
    for name, got, ref in (
            ("tau", h.tau_1h_profiles(th, Ms, fwhm=fwhm),
             model_reference(h, gm.gas_rows, gas_pp(), scale=gm.tau_factor(), Ms=Ms, thetas=th, fwhm=fwhm)),
            ("y", h.y_1h_profiles(th, Ms, fwhm=fwhm), model_reference(h, gm.pres_rows, pres_pp(), Ms=Ms, thetas=th, fwhm=fwhm))):
        err = relerr(got, ref)
        print(f"{name} through a 1.4' beam: worst relative error {err.max():.3e}")
        assert got.shape == (2, 1, 2)
        assert err.max() <= SMOOTH_GATE
    assert np.array_equal(h.tau_1h_profiles(th, Ms, fwhm=0.0), h.tau_1h_profiles(th, Ms))
    with pytest.raises(ValueError):
        h.tau_1h_profiles(th, Ms, fwhm=-1.0)


def test_a_redshift_slice_is_the_one_redshift_model(model):
    h1 = small_model(ZS[1])
    fwhm = 1.4 * np.pi / 180.0 / 60.0
    for name, kw in (("gas_sigma_1h_profiles", {}), ("gas_sigma_1h_profiles", dict(norm="mass")),
                     ("gas_delta_sigma_1h_profiles", {}), ("tau_1h_profiles", dict(fwhm=fwhm)), ("y_1h_profiles", {}),
                     ("y_1h_profiles", dict(fwhm=fwhm))):
        batch = getattr(model, name)(THETAS, MS_HALO, **kw)
        single = getattr(h1, name)(THETAS, MS_HALO, **kw)
        assert batch.shape == (2, 3, 5) and single.shape == (3, 5)
        assert np.array_equal(batch[1], single), (name, kw)
