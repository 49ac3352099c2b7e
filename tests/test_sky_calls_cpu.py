"""The native calls of the flat- and curved-sky covariance paths (hmvec_amd/angcov.py, hmvec_amd/curvedsky.py), pinned
without a GPU: every launch, in order, with every scalar argument, and which pointers are NULL.  The library runs against
tests/helpers/recording_context.py; EXPECTED was recorded from the library as it stood before the two modules were folded
onto one driver, so a launch that moves, disappears or changes an argument shows here."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import recording_context as rc  # noqa: E402

from hmvec_amd import _native as nat  # noqa: E402
from hmvec_amd import angcov, curvedsky  # noqa: E402

KEPT = ("hmg_angcov_", "hmg_curvedsky_", "hmg_angular_zsum", "hmg_memcpy_d2d")

NODES = [2, 10.5, 40, 300]
FLAT_EDGES = [0.01, 0.02, 0.05, 0.1]
CURVED_EDGES = [0.01, 0.02, 0.05, np.pi]
NOISE = [2e-9, 4e-10]
FSKY = 0.3
SPINS = [0, 2]
FLAT_PROBES = [(0, 0, 0), (0, 1, 2), (1, 1, 0)]                        # no order 4: its K pointer is NULL
CURVED_PROBES = [(0, 0, "w"), (0, 1, "gammat"), (1, 1, "xip")]          # no xim
MULTIPOLES = [2, 3, 4, 7, 8, 11]                                        # three runs of consecutive multipoles


def render(name, args):
    """Scalars as they are, device pointers as "p", NULL as None, the host copy of the probes as its ints."""
    if not name.startswith(KEPT):
        return None
    named = dict(zip(nat.PARAMS[name], args))
    out = []
    for par, v in list(named.items())[1:]:
        if par.startswith("d_"):
            out.append(None if v is None else "p")
        elif par == "h_probes":
            out.append([v[i] for i in range(3 * named["np"])])
        else:
            out.append(int(v) if isinstance(v, (int, np.integer)) else float(v))
    return out


def spectra():
    l = np.asarray(NODES, dtype=np.float64)
    C = np.empty((2, 2, l.size))
    C[0, 0], C[1, 1] = 3e-7 / (1.0 + l / 40.0), 5e-8 / (1.0 + l / 150.0)
    C[0, 1] = C[1, 0] = -0.5 * np.sqrt(C[0, 0] * C[1, 1])
    return C


def recorded():
    """{what was called: [(entry, rendered arguments)]}, each from a fresh recording context."""
    C = spectra()
    M = np.outer(C[0, 0], C[1, 1])
    runs = {
        "real_cov_gaussian_device": lambda ctx: angcov.real_cov_gaussian_device(NODES, C, NOISE, FLAT_EDGES, FLAT_PROBES, FSKY, ctx=ctx),
        "curved_cov_gaussian_device": lambda ctx: curvedsky.curved_cov_gaussian_device(
            NODES, C, NOISE, CURVED_EDGES, CURVED_PROBES, FSKY, spins=SPINS, ctx=ctx),
        "binned_angular_from_cl_device": lambda ctx: angcov.binned_angular_from_cl_device(NODES, C[0], FLAT_EDGES, 2, ctx=ctx),
        "curved_binned_from_cl_device": lambda ctx: curvedsky.curved_binned_from_cl_device(NODES, C[0], CURVED_EDGES, "xim", ctx=ctx),
        "project_cl_cov_device": lambda ctx: angcov.project_cl_cov_device(M, NODES, FLAT_EDGES, 0, 4, ctx=ctx),
        "curved_project_cl_cov_device": lambda ctx: curvedsky.curved_project_cl_cov_device(M, NODES, CURVED_EDGES, "gammat", "xim", ctx=ctx),
        "bin_averaged_bessel_device": lambda ctx: angcov.bin_averaged_bessel_device(MULTIPOLES, FLAT_EDGES, (4, 0), ctx=ctx),
        "bin_averaged_wigner_device": lambda ctx: curvedsky.bin_averaged_wigner_device(MULTIPOLES, CURVED_EDGES, ("xim", "w"), ctx=ctx),
    }
    out = {}
    for what, run in runs.items():
        ctx = rc.recording_context(render)
        run(ctx)
        out[what] = [(name, args) for name, args in ctx.lib.calls if args is not None]
        ctx.handle = None
    return out


P = "p"
AREA, SCALE = 3.7699111843077517, 0.15915494309189535           # 4 pi FSKY and 1 / (2 pi) as the library forms them
EXPECTED = {
    "real_cov_gaussian_device": [
        ("hmg_angcov_weights", [299, 3, P, P, P, P, None]),
        ("hmg_angcov_gaussian", [2, 4, P, P, P, 2, 299, 3, P, 3, [0, 0, 0, 0, 1, 1, 1, 1, 0], P, AREA, P, P, None, 54, P, P])],
    "curved_cov_gaussian_device": [
        ("hmg_curvedsky_weights", [2, 299, 3, P, P, P, P, P, None]),
        ("hmg_curvedsky_gaussian", [2, 4, P, P, P, 2, 299, 3, P, 3, [0, 0, 0, 0, 1, 1, 1, 1, 2], P, AREA, P, P, P, None, 54, P, P])],
    "binned_angular_from_cl_device": [
        ("hmg_angcov_weights", [299, 3, P, P, None, P, None]),
        ("hmg_angcov_node_weights", [4, P, 2, 299, 3, P, SCALE, 1, P]),
        ("hmg_angular_zsum", [1, 4, 3, 2, P, P, P])],
    "curved_binned_from_cl_device": [
        ("hmg_curvedsky_weights", [2, 299, 3, P, P, None, None, None, P]),
        ("hmg_curvedsky_node_weights", [4, P, 2, 299, 3, P, SCALE, 1, P]),
        ("hmg_angular_zsum", [1, 4, 3, 2, P, P, P])],
    "project_cl_cov_device": [
        ("hmg_angcov_weights", [299, 3, P, P, P, None, None]),
        ("hmg_angcov_node_weights", [4, P, 2, 299, 3, P, SCALE, 0, P]),
        ("hmg_angcov_weights", [299, 3, P, P, None, None, P]),
        ("hmg_angcov_node_weights", [4, P, 2, 299, 3, P, SCALE, 1, P]),
        ("hmg_angular_zsum", [1, 4, 4, 3, P, P, P]),
        ("hmg_angular_zsum", [1, 4, 3, 3, P, P, P])],
    "curved_project_cl_cov_device": [
        ("hmg_curvedsky_weights", [2, 299, 3, P, P, None, P, None, None]),
        ("hmg_curvedsky_node_weights", [4, P, 2, 299, 3, P, SCALE, 0, P]),
        ("hmg_curvedsky_weights", [2, 299, 3, P, P, None, None, None, P]),
        ("hmg_curvedsky_node_weights", [4, P, 2, 299, 3, P, SCALE, 1, P]),
        ("hmg_angular_zsum", [1, 4, 4, 3, P, P, P]),
        ("hmg_angular_zsum", [1, 4, 3, 3, P, P, P])],
    "bin_averaged_bessel_device": [
        ("hmg_angcov_weights", [6, 3, P, P, P, None, P])],
    "bin_averaged_wigner_device": [
        ("hmg_curvedsky_weights", [2, 10, 3, P, P, P, None, None, P]),
        ("hmg_memcpy_d2d", [P, P, 72]), ("hmg_memcpy_d2d", [P, P, 72]),         # l = 2, 3, 4 of each kind
        ("hmg_memcpy_d2d", [P, P, 48]), ("hmg_memcpy_d2d", [P, P, 48]),         # l = 7, 8
        ("hmg_memcpy_d2d", [P, P, 24]), ("hmg_memcpy_d2d", [P, P, 24])],        # l = 11
}


def test_the_covariance_paths_make_the_recorded_calls():
    got = recorded()
    assert list(got) == list(EXPECTED)
    for what, calls in got.items():
        assert calls == EXPECTED[what], what
