"""Curved-sky angular correlation functions and their Gaussian covariance on the GPU: the
bin-averaged Legendre / Wigner-d sums over integer multipoles that survey pipelines compare measurements with, where
sections 22 and 23 (``get_w_theta`` ..., ``angcov``) are flat-sky.

Four kinds, each a Wigner small-d function of theta: "w" d^l_{00} = P_l, "gammat" d^l_{02} = P_l^2 / sqrt((l-1) l (l+1) (l+2)),
"xip" d^l_{22}, "xim" d^l_{2,-2}; their flat-sky limits are J_0, J_2, J_0, J_4 of (l + 1/2) theta.

    xi_kind^{ab}(theta) = sum_l (2l + 1)/(4 pi) C_l^{ab} d_kind^l(theta)
    K_kind(l; a, b) = [G_kind(l; b) - G_kind(l; a)] / (cos a - cos b),   G_kind(l; theta) = int_0^theta sin d_kind^l,

the average of d_kind^l over the annulus [a, b], 0 < a < b <= pi, weighted with sin theta; a spin-2 kind is exactly 0
below l = 2.  Spectra, nodes, the integers L between the first and the last node, probes (f, g, kind) and noise levels
are angcov's (section 23): C is linear in l between nodes and zero outside.  With P = (a, b, kind), Q = (c, d, kind') and
A = 4 pi fsky,

    cov[P,i,Q,j] = 1/(4 pi A) sum_{l in L} (2l + 1) K_kind(l; i) K_kind'(l; j) [C^^ac C^^bd + C^^ad C^^bc - NN](l)
                 + delta_ij delta_kind,kind' (delta_ac delta_bd + delta_ad delta_bc) N_a N_b / (A 2 pi (cos a_i - cos b_i)):

section 23's formula with l -> l + 1/2 and pi (b^2 - a^2) -> 2 pi (cos a - cos b), the noise x noise term in closed form
(completeness: sum_l (2l + 1)/2 d^l(theta) d^l(theta') = delta(cos theta - cos theta')) and dropped between different
kinds.  Node weights R_kind[i, n] = sum_{l in L} (l + 1/2) K_kind(l; i) h_n(l): xi_kind(bin) = R_kind C / (2 pi), and
R_kind M R_kind'^T / (4 pi^2) projects an (l, l') matrix.

Shear factor: Limber spectra are those of the convergence; a spin-2 leg of a spectrum at node l carries
f(l) = sqrt((l + 2)(l - 1) / (l (l + 1))) (f for g-kappa -> g-E, f^2 for kappa-kappa -> E-E).  The free functions take
spectra as given - the caller's E-mode spectra; the model-level functions apply f to the fields flagged spin 2 unless
shear_factor=False.  The kernels are in hmvec_amd/csrc/kernels/curvedsky.hpp and angcov.hpp.

A sky is an angcov.Sky record, CURVED this one; the driver is in angcov.py, and covariance, binned xi and projection bind it.
"""
import ctypes as C_

import numpy as np

from . import _native as nat
from . import angcov
from .angcov import check_spins

__all__ = ["bin_averaged_wigner", "bin_averaged_wigner_device", "curved_cov_gaussian", "curved_cov_gaussian_device",
           "curved_binned_from_cl", "curved_binned_from_cl_device", "curved_project_cl_cov", "curved_project_cl_cov_device",
           "shear_factor", "curved_angular_spectra_device", "curved_angular_cov", "curved_angular_cov_device",
           "curved_angular_binned", "curved_angular_binned_device"]

KINDS = ("w", "gammat", "xip", "xim")
KIND_SPINS = {"w": (0, 0), "gammat": (0, 2), "xip": (2, 2), "xim": (2, 2)}


def lmax():
    """The largest multipole the weights kernel walks to (HMG_CURVEDSKY_LMAX of include/hmgrid.h)."""
    return nat.DEFINES["HMG_CURVEDSKY_LMAX"]


def check_nodes(ells):
    """angcov.check_nodes, and no multipole beyond lmax()."""
    nodes, l0, nl = angcov.check_nodes(ells)
    if l0 + nl - 1 > lmax():
        raise ValueError(f"the largest multipole of the curved-sky weights is {lmax()}, got {l0 + nl - 1}")
    return nodes, l0, nl


def check_kinds(kinds):
    """The kinds of a request as a tuple of names out of KINDS, and whether they were given as a sequence."""
    seq = isinstance(kinds, (tuple, list))
    out = tuple(kinds) if seq else (kinds,)
    if not out or any(not isinstance(k, str) or k not in KINDS for k in out):
        raise ValueError(f"a kind must be one of {KINDS}, got {kinds!r}")
    return out, seq


def check_edges(theta_edges):
    """angcov.check_edges, and no edge beyond pi."""
    e = angcov.check_edges(theta_edges)
    if e[-1] > np.pi:
        raise ValueError(f"theta_edges must lie in (0, pi], got {e[-1]}")
    return e


def cos_differences(edges):
    """cos a_i - cos b_i of the bins, as 2 sin((a + b)/2) sin((b - a)/2): what the weights and the noise term divide by."""
    a, b = edges[:-1], edges[1:]
    return 2.0 * (np.sin(0.5 * (a + b)) * np.sin(0.5 * (b - a)))


def check_probes(probes, nf, spins=None):
    return angcov.sky_check_probes(CURVED, probes, nf, spins)


def _weights_launch(ctx, l0, nl, edges, kinds):
    nt = edges.size - 1
    K = {k: ctx.empty((nl, nt)) for k in dict.fromkeys(kinds)}
    d_edges, d_cd = ctx.upload(edges), ctx.upload(cos_differences(edges))
    return ("hmg_curvedsky_weights", l0, nl, nt, d_edges.ptr, d_cd.ptr, *(nat.ptr(K.get(k)) for k in KINDS)), K, (d_edges, d_cd)


def weights_device(ctx, l0, nl, edges, kinds):
    """{kind: DeviceArray (nl, nt)} of K_kind on l0 .. l0 + nl - 1: one launch for all the kinds."""
    launch, K, _keepalive = _weights_launch(ctx, l0, nl, edges, kinds)
    ctx.call(*launch)
    return K


CURVED = angcov.Sky(names=KINDS, word="kind", check_names=check_kinds, spins=KIND_SPINS, check_nodes=check_nodes,
                    check_edges=check_edges, weights_launch=_weights_launch, geometry=cos_differences,
                    gaussian="hmg_curvedsky_gaussian", node_weights="hmg_curvedsky_node_weights")


def bin_averaged_wigner_device(ells_int, theta_edges, kinds, *, ctx=None):
    """bin_averaged_wigner with the results left on the device: a dict {kind: DeviceArray (len(ells_int), ntheta)}."""
    kinds, _ = check_kinds(kinds)
    ells, edges = angcov.check_multipoles(ells_int), check_edges(theta_edges)
    if ells.size and ells.max() > lmax():
        raise ValueError(f"the largest multipole of the curved-sky weights is {lmax()}, got {int(ells.max())}")
    ctx = nat.context_or_default(ctx)
    nt = edges.size - 1
    if ells.size == 0:
        return {k: ctx.empty((0, nt)) for k in kinds}
    l0, l1 = int(ells.min()), int(ells.max())
    full = weights_device(ctx, l0, l1 - l0 + 1, edges, kinds)          # the recurrences pass every multipole anyway
    if ells.size == l1 - l0 + 1 and np.array_equal(ells, np.arange(l0, l1 + 1)):
        return full
    rows = (ells - l0).astype(np.int64)
    cuts = np.flatnonzero(np.diff(rows) != 1) + 1                       # runs of consecutive multipoles: one copy each
    out = {k: ctx.empty((ells.size, nt)) for k in full}
    for a, b in zip(np.concatenate([[0], cuts]), np.concatenate([cuts, [rows.size]])):
        for k in full:
            ctx.call("hmg_memcpy_d2d", out[k].view(int(a) * nt, ((b - a) * nt,)).ptr,
                     full[k].view(int(rows[a]) * nt, ((b - a) * nt,)).ptr, int(b - a) * nt * 8)
    return out


def bin_averaged_wigner(ells_int, theta_edges, kinds, *, ctx=None):
    """K_kind[l, i] = [G_kind(l; b_i) - G_kind(l; a_i)] / (cos a_i - cos b_i), the average of d_kind^l(theta) over the
    annulus [a_i, b_i] = theta_edges[i : i + 2] weighted with sin theta, at the integer multipoles ells_int (>= 1).

    theta_edges: ntheta + 1 angles in radians, in (0, pi], strictly increasing.  kinds: "w", "gammat", "xip", "xim" or a
    sequence of them.  Returns a float64 array (len(ells_int), ntheta), or a tuple of them for a sequence of kinds; a
    value depends on its multipole and its two edges alone, and a spin-2 kind is exactly 0 at l = 1.  Anything else
    raises ValueError before a launch."""
    kinds, seq = check_kinds(kinds)
    K = bin_averaged_wigner_device(ells_int, theta_edges, kinds, ctx=ctx)
    outs = tuple(K[k].numpy() if K[k].size else np.empty(K[k].shape) for k in kinds)
    return outs if seq else outs[0]


def curved_cov_gaussian_device(ells, C, noise, theta_edges, probes, fsky, *, spins=None, ctx=None):
    """curved_cov_gaussian with the result left on the device: angcov.sky_cov_gaussian_device of the curved sky."""
    return angcov.sky_cov_gaussian_device(CURVED, ells, C, noise, theta_edges, probes, fsky, spins=spins, ctx=ctx)


def curved_cov_gaussian(ells, C, noise, theta_edges, probes, fsky, *, spins=None, ctx=None):
    """Gaussian covariance cov[P, i, Q, j] of the bin-averaged curved-sky correlation functions xi_kind^{ab}(bin i) of
    the probes P = (a, b, kind), shape (nprobe, ntheta, nprobe, ntheta); the definition is the module's.

    ells, C, noise, fsky: as for angcov.real_cov_gaussian (C WITHOUT noise; for a spin-2 field the E-mode spectra, see
    shear_factor).  theta_edges: ntheta + 1 bin edges in radians, in (0, pi], strictly increasing.  probes: a sequence of
    (f, g, kind).  spins: optionally 0 or 2 per field; a probe whose kind does not fit its fields' spins ("w" 0 and 0,
    "gammat" 0 and 2, "xip" and "xim" 2 and 2) is then refused.

    The noise x noise term is added in closed form on the diagonal i = j of blocks of one kind and dropped between
    different kinds; the signal x noise terms are in the sum.  An element depends on its own two probes, its two bins,
    the spectra and L alone: a subset of the probes or bins returns the bits of the full call, a repeat the same bits,
    cov[P,i,Q,j] == cov[Q,j,P,i], and swapping (f, g) inside a probe changes nothing.  Anything invalid raises
    ValueError before a launch."""
    return curved_cov_gaussian_device(ells, C, noise, theta_edges, probes, fsky, spins=spins, ctx=ctx).numpy()


def node_weights_device(ctx, nodes, l0, nl, edges, kind, scale=1.0, by_node=False):
    return angcov.sky_node_weights_device(CURVED, ctx, nodes, l0, nl, edges, kind, scale, by_node)


def curved_binned_from_cl_device(ells, C, theta_edges, kind, *, ctx=None):
    """curved_binned_from_cl with the result left on the device: angcov.sky_binned_device of the curved sky."""
    return angcov.sky_binned_device(CURVED, ells, C, theta_edges, kind, ctx=ctx)


def curved_binned_from_cl(ells, C, theta_edges, kind, *, ctx=None):
    """Bin-averaged curved-sky correlation function xi_kind(bin i) = R_kind[i, :] . C / (2 pi)
    = sum_{l in L} (2l + 1)/(4 pi) K_kind(l; i) C(l) of the spectra C[..., :] at the nodes ells: the discretisation
    curved_cov_gaussian is the covariance of.  Returns C's leading shape with ntheta last."""
    return angcov.sky_binned(CURVED, ells, C, theta_edges, kind, ctx=ctx)


def curved_project_cl_cov_device(M, ells, theta_edges, kind1, kind2, *, ctx=None):
    """curved_project_cl_cov with the result left on the device: angcov.sky_project_device of the curved sky."""
    return angcov.sky_project_device(CURVED, M, ells, theta_edges, kind1, kind2, ctx=ctx)


def curved_project_cl_cov(M, ells, theta_edges, kind1, kind2, *, ctx=None):
    """R_kind1 M R_kind2^T / (4 pi^2), shape (ntheta, ntheta): angcov.project_cl_cov with the curved-sky node weights."""
    return curved_project_cl_cov_device(M, ells, theta_edges, kind1, kind2, ctx=ctx).numpy()


def shear_factor(ells):
    """f(l) = sqrt((l + 2)(l - 1) / (l (l + 1))): what one spin-2 leg of a convergence spectrum is multiplied by to give
    the E-mode spectrum (0 at l = 1).  ells >= 1."""
    l = np.asarray(ells, dtype=np.float64)
    if not np.all(np.isfinite(l)) or np.any(l < 1):
        raise ValueError("ells must be finite and at least 1")
    return np.sqrt(((l + 2.0) * (l - 1.0)) / (l * (l + 1.0)))


def _split_fields(fields):
    """({label: (tracer, window, noise)}, spins) of fields = {label: (tracer, window, noise, spin)}."""
    plain, spins = {}, []
    for lab in fields:
        try:
            name, window, level, spin = fields[lab]
        except (TypeError, ValueError):
            raise ValueError(f"fields[{lab!r}] must be (tracer name, window, noise, spin)") from None
        if isinstance(spin, bool) or spin not in (0, 2):
            raise ValueError(f"the spin of field {lab!r} must be 0 or 2, got {spin!r}")
        plain[lab] = (name, window, level)
        spins.append(int(spin))
    return plain, spins


def curved_angular_spectra_device(model, fields, ells, term="total", shear_factor=True):
    """The spectra curved_angular_cov contracts, for a HaloModel `model`: (labels, C, noise, spins) with (labels, C,
    noise) = angcov.angular_cov_spectra_device(model, fields without their spins, ells, term) and then, unless
    shear_factor is False, every entry C[f, g] multiplied on the device by f(ells) per spin-2 field among f and g
    (f for one, (l + 2)(l - 1) / (l (l + 1)) for two).  fields: {label: (tracer name, window (nz,), noise level, spin 0
    or 2)}."""
    plain, spins = _split_fields(fields)
    labels, Ctab, noise = angcov.angular_cov_spectra_device(model, plain, ells, term)
    sp = check_spins(spins, len(labels))
    if shear_factor and np.any(sp == 2):
        ctx = model._ctx()
        nodes, _, _ = angcov.check_nodes(ells)
        ctx.call("hmg_curvedsky_scale_spectra", len(labels), nodes.size, ctx.upload(nodes).ptr,
                 sp.ctypes.data_as(C_.POINTER(C_.c_int)), ctx.upload_int32(sp).ptr, Ctab.ptr)
    return labels, Ctab, noise, spins


def curved_angular_cov_device(model, theta_edges, probes, fields, fsky, ells, term="total", shear_factor=True):
    """curved_angular_cov with the result left on the device."""
    labels, Ctab, noise, spins = curved_angular_spectra_device(model, fields, ells, term, shear_factor)
    return curved_cov_gaussian_device(ells, Ctab, noise, theta_edges, angcov.sky_by_index(CURVED, probes, labels), fsky,
                                      spins=spins, ctx=model._ctx())


def curved_angular_cov(model, theta_edges, probes, fields, fsky, ells, term="total", shear_factor=True):
    """Gaussian covariance cov[P, i, Q, j], shape (nprobe, ntheta, nprobe, ntheta), of the bin-averaged curved-sky
    correlation functions of a HaloModel's tracers: the probes are (label, label2, kind).  Bit for bit
    curved_cov_gaussian(ells, C, noise, theta_edges, probes by field index, fsky, spins=spins) with (labels, C, noise,
    spins) = curved_angular_spectra_device(model, fields, ells, term, shear_factor).  A function of the model, like
    angcov.angular_cov: the attribute surface of HaloModel is pinned and stays as it is."""
    return curved_angular_cov_device(model, theta_edges, probes, fields, fsky, ells, term, shear_factor).numpy()


def curved_angular_binned_device(model, theta_edges, probes, fields, ells, term="total", shear_factor=True):
    """curved_angular_binned with the result left on the device: a list of DeviceArrays (1, ntheta), one per probe."""
    labels, Ctab, _, spins = curved_angular_spectra_device(model, fields, ells, term, shear_factor)
    nf, nn = len(labels), Ctab.shape[2]
    pr = check_probes(angcov.sky_by_index(CURVED, probes, labels), nf, spins)
    check_edges(theta_edges)
    out = []
    for f, g, k in pr.tolist():
        lo, hi = min(f, g), max(f, g)
        out.append(curved_binned_from_cl_device(ells, Ctab.view((lo * nf + hi) * nn, (1, nn)), theta_edges, KINDS[k],
                                                ctx=model._ctx()))
    return out


def curved_angular_binned(model, theta_edges, probes, fields, ells, term="total", shear_factor=True):
    """The curved-sky data vector (nprobe, ntheta): xi_kind^{ab}(bin i) of the probes (label, label2, kind), row by row
    bit for bit curved_binned_from_cl(ells, C[a, b], theta_edges, kind) with C of curved_angular_spectra_device."""
    return np.concatenate([d.numpy() for d in curved_angular_binned_device(model, theta_edges, probes, fields, ells, term,
                                                                          shear_factor)], axis=0)
