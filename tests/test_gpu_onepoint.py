"""The one-point contractions on the GPU against the long-double numpy model of
tests/helpers/onepoint_model.py, and the HaloModel methods end to end.

The kernel gate, per (z, j) and separately for the real and the imaginary part, is

    |A_gpu - A_ref| <= eps sum_n |W_n| (|phi_n| + K min(|phi_n|, 2)),   K = 4 + chain_length(nm_used, nt):

half an ulp each of lambda_j and of the product lambda_j s moves a term by eps |phi|; the sine and cosine are within an ulp
plus 2e-16, the weight and its product with the term add theirs, and every addition on the longest chain adds an ulp of
the partial sum.  chain_length is asserted <= 64 for every shape here, so the bound cannot be inflated.
Measured on an MI355X: see DESIGN.md section 20."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import gas_profile_model as gm  # noqa: E402
import onepoint_model as om  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
RING_GATE = om.RING_GATE
# the last shape has more than 4096 samples per redshift: the exponent's samples go to two slices
SHAPES = [(1, 1, 1), (2, 5, 7), (3, 16, 64), (2, 67, 33), (1, 130, 33)]
NLAMBDAS = (1, 2, 65, 130)
PHI_MAX = (1e-12, 1.0, 2e4, 3e9)          # the last is above 2^30: the library's sine and cosine


def windows(nm):
    out = [(0, nm)]
    if nm >= 3:
        out.append((1, nm - 1))
    if nm >= 2:
        out.append((nm // 2, nm // 2 + 1))
    return out


def draw(shape, seed=11):
    """Random positive area, nzm, wm, zw and a signal in (0, 1] whose largest value is exactly 1."""
    nz, nm, nt = shape
    rng = np.random.default_rng(seed + 1000 * nz + 10 * nm + nt)
    signal = rng.uniform(0.05, 1.0, shape)
    signal.flat[rng.integers(signal.size)] = 1.0
    return dict(signal=signal, area=rng.uniform(0.1, 2.0, shape), nzm=rng.uniform(0.1, 3.0, (nz, nm)),
                wm=rng.uniform(0.1, 1.5, nm), zw=rng.uniform(0.2, 2.0, nz))


# ---------------------------------------------------------------- 1. the exponent against the model
@pytest.mark.parametrize("phimax", PHI_MAX)
@pytest.mark.parametrize("shape", SHAPES)
def test_exponent_matches_the_model(shape, phimax):
    from hmvec_amd import onepoint
    d = draw(shape)
    nz, nm, nt = shape
    worst = worst_re = 0.0
    for nl in NLAMBDAS:
        dl = phimax / max(nl - 1, 1)                  # lambda_max s_max = phimax
        for win in windows(nm):
            K = 4 + onepoint.chain_length(win[1] - win[0], nt)
            assert K - 4 <= 64
            got = onepoint.char_exponent(nlambda=nl, dlambda=dl, mwindow=win, per_z=True, **d)
            ref, bound = om.exponent(nlambda=nl, dlambda=dl, window=win, K=K, **d)
            assert got.shape == (nz, nl) and got.dtype == np.complex128
            assert np.all(got[:, 0] == 0.0)
            for part in (np.real, np.imag):
                err = np.abs(part(got) - part(ref))
                assert np.all(err[:, 1:] <= bound[:, 1:]), (nl, win, part.__name__, (err[:, 1:] / bound[:, 1:]).max())
                if nl > 1:
                    worst = max(worst, float((err[:, 1:] / bound[:, 1:]).max()))
            if phimax == 1e-12 and nl > 1:
                # every term of the real part has the same sign, so the gate is a relative one: 2 eps from the phase
                # (the term is quadratic in it), K eps from the rest.  cos(phi) - 1 has no digits here.
                rel = np.abs(np.real(got)[:, 1:] / np.real(ref)[:, 1:] - 1.0)
                assert np.all(np.real(ref)[:, 1:] < 0.0) and np.all(rel <= EPS * (2 + K)), (nl, win, rel.max() / EPS)
                worst_re = max(worst_re, float(rel.max() / (EPS * (2 + K))))
    print(f"shape {shape} phi_max {phimax:g}: worst |dA| / bound = {worst:.3f}"
          + (f", worst relative error of Re A / its bound = {worst_re:.3f}" if phimax == 1e-12 else ""))


# ---------------------------------------------------------------- 2. the moments against the model
@pytest.mark.parametrize("shape", SHAPES)
def test_moments_match_the_model(shape):
    from hmvec_amd import onepoint
    d = draw(shape, seed=5)
    worst = 0.0
    for win in windows(shape[1]):
        gate = EPS * (6 + onepoint.chain_length(win[1] - win[0], shape[2]))
        got = onepoint.cumulants(mwindow=win, per_z=True, **d)
        ref = om.moments(window=win, **d)
        assert got.shape == (shape[0], 4)
        rel = np.abs(got / ref - 1.0)
        assert np.all(rel <= gate), (win, rel.max() / gate)
        worst = max(worst, float(rel.max() / gate))
    print(f"shape {shape}: worst relative error of a moment / gate = {worst:.3f}")


@pytest.mark.parametrize("shape", [(2, 5, 7), (2, 67, 33)])
def test_first_moment_is_the_slope_of_the_imaginary_part(shape):
    """Im A(dlambda) / dlambda = kappa_1 (1 - O(phi^2 / 6)): with phi_max = 1e-6 the next term is 1.7e-13."""
    from hmvec_amd import onepoint
    d = draw(shape, seed=9)
    dl = 1e-6
    A = onepoint.char_exponent(nlambda=2, dlambda=dl, per_z=True, **d)
    K1 = onepoint.cumulants(per_z=True, **d)[:, 0]
    rel = np.abs(A[:, 1].imag / dl / K1 - 1.0)
    print(f"shape {shape}: Im A(dlambda) / dlambda against kappa_1: {rel.max():.2e}")
    assert np.all(rel <= 1e-11)


# ---------------------------------------------------------------- 3. determinism
@pytest.mark.parametrize("shape", [(3, 16, 64), (3, 130, 33)])
def test_repeats_and_a_row_of_a_batch_equals_the_row_alone(shape):
    from hmvec_amd import onepoint
    d = draw(shape, seed=21)
    nl, dl = 130, 2e4 / 129
    A = onepoint.char_exponent(nlambda=nl, dlambda=dl, per_z=True, **d)
    K = onepoint.cumulants(per_z=True, **d)
    assert np.array_equal(onepoint.char_exponent(nlambda=nl, dlambda=dl, per_z=True, **d), A)
    assert np.array_equal(onepoint.cumulants(per_z=True, **d), K)
    for z in range(shape[0]):
        one = {k: (v if k == "wm" else v[z:z + 1]) for k, v in d.items()}
        assert np.array_equal(onepoint.char_exponent(nlambda=nl, dlambda=dl, per_z=True, **one)[0], A[z])
        assert np.array_equal(onepoint.cumulants(per_z=True, **one)[0], K[z])
    Asum = onepoint.char_exponent(nlambda=nl, dlambda=dl, **d)
    Ksum = onepoint.cumulants(**d)
    assert Asum.shape == (nl,) and Ksum.shape == (4,)
    assert np.array_equal(onepoint.char_exponent(nlambda=nl, dlambda=dl, **d), Asum)
    for part in (np.real, np.imag):
        assert np.all(np.abs(part(Asum) - part(A).sum(axis=0)) <= 4 * EPS * np.abs(part(A)).sum(axis=0))
    assert np.all(np.abs(Ksum - K.sum(axis=0)) <= 4 * EPS * np.abs(K).sum(axis=0))


# ---------------------------------------------------------------- 4. end to end
ZS = np.array([0.2, 0.6, 1.0])
C_KMS = 299792.458


def small_model(zs):
    import hmvec_amd as hm
    return hm.HaloModel(np.atleast_1d(zs), np.geomspace(1e-3, 10.0, 32), ms=np.geomspace(1e11, 1e16, 16), accuracy="low",
                        engine="analytic")


def pres_pp():
    from hmvec_amd import battaglia_defaults, default_params
    return dict(battaglia_defaults[default_params["battaglia_pres_family"]],
                battaglia_pres_gamma=default_params["battaglia_pres_gamma"],
                battaglia_pres_alpha=default_params["battaglia_pres_alpha"])


@pytest.fixture(scope="module")
def model():
    return small_model(ZS)


@pytest.fixture(scope="module")
def host(model):
    """What the checks build on the host, once: the weights, the model's per-halo scalars (gas_profile_model.pres_rows),
    and the rings' radii, solid angles and y through the public y_1h_profiles, halo by halo."""
    from hmvec_amd import onepoint
    from hmvec_amd.quadrature import trapz_weights
    h = model
    chi = np.asarray(h.comoving_radial_distance(ZS)).reshape(-1)
    zw = trapz_weights(ZS) * C_KMS * chi ** 2 / np.asarray(h.hubble_parameter(ZS)).reshape(-1)
    rows = [[gm.pres_rows(h, iz, M, pres_pp()) for M in h.ms] for iz in range(ZS.size)]
    theta_out = np.array([[halo_edge(h, iz, M) for M in h.ms] for iz in range(ZS.size)])
    u, w = onepoint.ring_rule()
    y = np.empty((ZS.size, h.ms.size, u.size))
    for im, M in enumerate(h.ms):
        for iz in range(ZS.size):
            y[iz, im] = h.y_1h_profiles(theta_out[iz, im] * u, [M])[iz, 0]
    area = (2.0 * np.pi * theta_out ** 2)[:, :, None] * (u * w)[None, None, :]
    return dict(zw=zw, wm=trapz_weights(h.ms), nzm=np.asarray(h.nzm), rows=rows, theta_out=theta_out, y=y, area=area)


def halo_edge(h, iz, M):
    z, da, rhoc, rvir, m2, r2 = gm.halo_scalars(h, iz, M)
    return rvir / da


def test_mean_y_is_the_volume_integral_of_the_pressure(model, host):
    """<y> = sum_z zw sum_m wm n pref r^2 N_total / D_A^2: the disc integral of a halo's y is the volume integral of its
    pressure profile, which the ring rule reaches to RING_GATE (tests/test_onepoint_cpu.py)."""
    k = model.get_y_cumulants()
    assert k.shape == (4,) and np.all(k > 0)
    per_halo = np.array([[r["fit"] * r["r"] ** 2 * gm.N_total(r["alpha"], r["gamma"], r["eta"], r["xcut"]) / r["da"] ** 2
                          for r in rz] for rz in host["rows"]])
    ref = np.sum(host["zw"][:, None] * host["wm"][None, :] * host["nzm"] * per_halo)
    print(f"<y> = {k[0]:.6e}, against the volume integrals {abs(k[0] / ref - 1):.2e} (gate {RING_GATE:.2e}); "
          f"kappa_2..4 = {k[1]:.4e} {k[2]:.4e} {k[3]:.4e}")
    assert abs(k[0] / ref - 1.0) <= RING_GATE
    kz = model.get_y_cumulants(per_z=True)
    assert kz.shape == (3, 4) and np.all(np.abs(kz.sum(axis=0) / k - 1.0) <= 8 * EPS)


def test_y_exponent_equals_the_contraction_of_the_public_profiles(model, host):
    from hmvec_amd import onepoint
    k = model.get_y_cumulants()
    nbins = 256
    dy = np.sqrt(k[1]) / 10.0
    nl, dl = onepoint.lambda_grid(nbins, dy)
    got = model.get_y_char_exponent(nbins, dy, per_z=True)
    parts = {n: host[n] for n in ("area", "nzm", "wm", "zw")}
    ref = onepoint.char_exponent(host["y"], nlambda=nl, dlambda=dl, per_z=True, **parts)
    # both sides come from the kernel (twice its gate), from profiles that agree to the projection's 1e-10
    K = 4 + onepoint.chain_length(model.ms.size, host["y"].shape[-1])
    _, bound = om.exponent(host["y"], nlambda=nl, dlambda=dl, K=K, dtype=np.float64, **parts)
    W = np.abs(om.weights(dtype=np.float64, **parts)).reshape(ZS.size, -1)
    phi = dl * np.arange(nl)[None, :, None] * np.abs(host["y"]).reshape(ZS.size, 1, -1)
    tol = 2.0 * bound + 1e-10 * np.sum(W[:, None, :] * phi, axis=-1)
    assert got.shape == ref.shape == (ZS.size, nl) and np.all(got[:, 0] == 0.0)
    for part in (np.real, np.imag):
        err = np.abs(part(got) - part(ref))
        print(f"{part.__name__}: worst |dA| / tolerance = {(err[:, 1:] / tol[:, 1:]).max():.3e}")
        assert np.all(err[:, 1:] <= tol[:, 1:])
    total = model.get_y_char_exponent(nbins, dy)
    assert np.all(np.abs(total - got.sum(axis=0)) <= 4 * EPS * (np.abs(got.real) + np.abs(got.imag)).sum(axis=0))


def test_y_pdf_sums_to_one_and_has_the_cumulants_moments(model, host):
    """512 bins, noise = 3 dy, sd^2 = kappa_2 + noise^2, from ymin = kappa_1 - 8 sd to at least kappa_1 + 40 sd.

    The PDF of y is far from Gaussian: kappa_4 / kappa_2^2 is 1.5e3 on this grid, and the centre of the heaviest halo
    lies hundreds of sd above the mean.  A range that ends at exactly kappa_1 + 40 sd (dy = 1.93e-7) leaves 4.5e-5 of the
    probability outside, measured on an MI355X with the model below, far above the 1e-8 the moment checks need: the mean
    then misses kappa_1 by 8e-3 and the variance by 15 per cent, all of it aliasing.  The range therefore ends at the
    larger of kappa_1 + 40 sd and (the largest y any ring of the grid has) + kappa_1 + 8 sd: beyond that only two
    overlapping heavy halos reach.  dy follows from the 512 bins."""
    from scipy.optimize import brentq
    k = model.get_y_cumulants()
    nbins = 512
    ytop = float(host["y"].max())

    def slack(dy):          # bins available minus bins needed
        sd = np.sqrt(k[1] + 9.0 * dy ** 2)
        return nbins * dy - 8.0 * sd - max(40.0 * sd, ytop + 8.0 * sd)
    dy = brentq(slack, 1e-3 * np.sqrt(k[1]), 1e3 * max(np.sqrt(k[1]), ytop), xtol=1e-300, rtol=1e-14)
    noise = 3.0 * dy
    sd = np.sqrt(k[1] + noise ** 2)
    ymin = k[0] - 8.0 * sd
    assert ymin + nbins * dy >= k[0] + 40.0 * sd * (1 - 1e-12)
    print(f"largest y of a ring = {ytop:.4e} = kappa_1 + {(ytop - k[0]) / sd:.1f} sd; the range ends at kappa_1 + "
          f"{(ymin + nbins * dy - k[0]) / sd:.1f} sd")
    ys, p = model.get_y_pdf(nbins, dy, ymin=ymin, noise_sigma=noise)
    # the mass outside the range, from the model on a range four times as long (24 sd below, 168 sd above the mean)
    parts = {n: host[n] for n in ("area", "nzm", "wm", "zw")}
    Aw, _ = om.exponent(host["y"], nlambda=2 * nbins + 1, dlambda=2.0 * np.pi / (4 * nbins * dy), dtype=np.float64, **parts)
    yw, pw = om.pdf(Aw.sum(axis=0), dy, k[0] - 24.0 * sd, noise)
    inside = (yw >= ymin - 0.5 * dy) & (yw < ymin + (nbins - 0.5) * dy)
    tail = float(pw[~inside].sum())
    mean, var = np.sum(p * ys), np.sum(p * (ys - np.sum(p * ys)) ** 2)
    print(f"dy = {dy:.4e}, tail mass outside the range = {tail:.3e}, sum p - 1 = {p.sum() - 1:.2e}, min p = {p.min():.2e}, "
          f"mean / kappa_1 - 1 = {mean / k[0] - 1:.2e}, var / (kappa_2 + noise^2) - 1 = {var / sd ** 2 - 1:.2e}")
    assert tail < 1e-8
    assert abs(p.sum() - 1.0) <= 1e-12
    assert np.all(p >= -1e-15)
    assert abs(mean / k[0] - 1.0) <= 1e-6
    assert abs(var / sd ** 2 - 1.0) <= 1e-6


def test_mass_cut_lowers_the_cumulants_and_equals_the_generic_route(model, host):
    from hmvec_amd import onepoint
    k = model.get_y_cumulants()
    mmax = model.ms[11]
    kc = model.get_y_cumulants(mmax=mmax)
    assert np.all(kc < k)
    parts = {n: host[n] for n in ("area", "nzm", "wm", "zw")}
    ref = onepoint.cumulants(host["y"], mwindow=(0, 12), **parts)
    assert np.all(np.abs(kc / ref - 1.0) <= 1e-10 * np.arange(1, 5) + 2 * EPS * (6 + onepoint.chain_length(12, 256)))
    nbins, dy = 128, np.sqrt(kc[1]) / 6.0
    got = model.get_y_char_exponent(nbins, dy, mmax=mmax)
    gen = model.profile_char_exponent(host["y"], host["theta_out"], nbins, dy, mmax=mmax)
    nl, dl = onepoint.lambda_grid(nbins, dy)
    K = 4 + onepoint.chain_length(12, 256)
    _, bound = om.exponent(host["y"], nlambda=nl, dlambda=dl, window=(0, 12), K=K, dtype=np.float64, **parts)
    W = np.abs(om.weights(window=(0, 12), dtype=np.float64, **parts)).reshape(ZS.size, -1)
    phi = dl * np.arange(nl)[None, :, None] * np.abs(host["y"][:, :12]).reshape(ZS.size, 1, -1)
    tol = (2.0 * bound + 1e-10 * np.sum(W[:, None, :] * phi, axis=-1)).sum(axis=0) \
        + 4 * EPS * np.abs(om.exponent(host["y"], nlambda=nl, dlambda=dl, window=(0, 12), dtype=np.float64, **parts)[0]).sum(axis=0)
    for part in (np.real, np.imag):
        assert np.all(np.abs(part(got) - part(gen))[1:] <= tol[1:])
    # a device buffer is taken as it is
    d_y = model._ctx().upload(host["y"])
    assert np.array_equal(model.profile_char_exponent(d_y, host["theta_out"], nbins, dy, mmax=mmax), gen)


def test_beam_keeps_the_mean_and_lowers_the_variance(model):
    k = model.get_y_cumulants()
    kb = model.get_y_cumulants(fwhm=1.4 * np.pi / 180.0 / 60.0)
    print(f"beam 1.4': kappa_1 ratio - 1 = {kb[0] / k[0] - 1:.2e}, kappa_2 ratio = {kb[1] / k[1]:.4f}")
    assert abs(kb[0] / k[0] - 1.0) <= 1e-6
    assert kb[1] < k[1]


# ---------------------------------------------------------------- 5. the C ABI refuses without launching
def test_c_abi_rejects_bad_arguments():
    from hmvec_amd import _native as nat
    ctx = nat.Context(0)
    d = ctx.upload(np.linspace(0.1, 1.0, 64))
    p = d.ptr
    good_e = [2, 3, 4, p, p, None, p, p, p, 0, 3, 4, 0.5, p, None]
    good_m = [2, 3, 4, p, p, None, p, p, p, 0, 3, p, None]
    ctx.call("hmg_onepoint_exponent", *good_e)
    ctx.call("hmg_onepoint_moments", *good_m)

    def bad(entry, good, at, value, match):
        args = list(good)
        args[at] = value
        with pytest.raises(nat.NativeError, match=match):
            ctx.call(entry, *args)

    for entry, good, out in (("hmg_onepoint_exponent", good_e, 13), ("hmg_onepoint_moments", good_m, 11)):
        for at in (3, 4, 6, 7, 8):
            bad(entry, good, at, None, "NULL")
        bad(entry, good, out, None, "NULL")
        for at in (0, 1, 2):
            bad(entry, good, at, 0, "empty")
        bad(entry, good, 9, 3, "window")            # m_lo >= m_hi
        bad(entry, good, 9, -1, "window")
        bad(entry, good, 10, 4, "window")           # m_hi > nm
        bad(entry, good, 10, 0, "window")
    bad("hmg_onepoint_exponent", good_e, 11, 0, "nlambda")
    for v in (0.0, -1.0, float("nan"), float("inf")):
        bad("hmg_onepoint_exponent", good_e, 12, v, "dlambda")
    ctx.sync()
    ctx.close()
