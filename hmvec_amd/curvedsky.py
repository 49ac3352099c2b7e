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
"""
import ctypes as C_

import numpy as np

from . import _native as nat
from . import angcov

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


def check_spins(spins, nf):
    s = np.asarray(spins)
    if s.shape != (nf,) or any(isinstance(v, bool) or v not in (0, 2) for v in s.tolist()):
        raise ValueError(f"spins must hold 0 or 2 for each of the {nf} fields, got {spins!r}")
    return np.ascontiguousarray(s, dtype=np.int32)


def check_probes(probes, nf, spins=None):
    """The probes (f, g, kind) as an (np, 3) int32 array of (f, g, index of the kind); with spins (0 or 2 per field) a
    kind whose pair of spins is not its fields' is refused."""
    out = []
    for p in probes:
        if len(p) != 3:
            raise ValueError(f"a probe is (f, g, kind), got {p!r}")
        f, g, kind = p
        (kind,), _ = check_kinds(kind)
        if any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) for v in (f, g)) or not (0 <= f < nf and 0 <= g < nf):
            raise ValueError(f"probe {p!r} names a field outside 0 .. {nf - 1}")
        if spins is not None and tuple(sorted((int(spins[f]), int(spins[g])))) != KIND_SPINS[kind]:
            raise ValueError(f"probe {p!r}: kind {kind!r} needs fields of spin {KIND_SPINS[kind]}, these have spin "
                             f"{(int(spins[f]), int(spins[g]))}")
        out.append((int(f), int(g), KINDS.index(kind)))
    if not out:
        raise ValueError("at least one probe is needed")
    return np.ascontiguousarray(out, dtype=np.int32)


def weights_device(ctx, l0, nl, edges, kinds):
    """{kind: DeviceArray (nl, nt)} of K_kind on l0 .. l0 + nl - 1: one launch for all the kinds."""
    nt = edges.size - 1
    K = {k: ctx.empty((nl, nt)) for k in dict.fromkeys(kinds)}
    ctx.call("hmg_curvedsky_weights", l0, nl, nt, ctx.upload(edges).ptr, ctx.upload(cos_differences(edges)).ptr,
             *(nat.ptr(K.get(k)) for k in KINDS))
    return K


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
    """curved_cov_gaussian with the result left on the device: a DeviceArray (nprobe, ntheta, nprobe, ntheta).  C may be
    a DeviceArray (nf, nf, len(ells)): it is taken as it is, and of its entries those with f <= g are read."""
    nodes, l0, nl = check_nodes(ells)
    C, nf = angcov.check_spectra(C, nodes.size)
    noise, edges, fsky = angcov.check_noise(noise, nf), check_edges(theta_edges), angcov.check_fsky(fsky)
    if spins is not None:
        spins = check_spins(spins, nf)
    pr = check_probes(probes, nf, spins)
    ctx = nat.context_or_default(ctx)
    nt, np_ = edges.size - 1, pr.shape[0]
    K = weights_device(ctx, l0, nl, edges, [KINDS[k] for k in sorted(set(pr[:, 2].tolist()))])
    words = np_ * (np_ + 1) // 2 * ((nl - 1) // angcov.chunk() + 1) * nt * nt
    work, cov = ctx.empty((words,)), ctx.empty((np_, nt, np_, nt))
    d_nodes, d_C, d_noise, d_pr = ctx.upload(nodes), nat.as_device(ctx, C), ctx.upload(noise), ctx.upload_int32(pr)
    ctx.call("hmg_curvedsky_gaussian", nf, nodes.size, d_nodes.ptr, d_C.ptr, d_noise.ptr, l0, nl, nt,
             ctx.upload(cos_differences(edges)).ptr, np_, pr.ctypes.data_as(C_.POINTER(C_.c_int)), d_pr.ptr,
             4.0 * np.pi * fsky, *(nat.ptr(K.get(k)) for k in KINDS), words, work.ptr, cov.ptr)
    return cov


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
    """scale * R_kind as a DeviceArray (ntheta, nn), or (nn, ntheta) with by_node."""
    nt = edges.size - 1
    K = weights_device(ctx, l0, nl, edges, (kind,))[kind]
    R = ctx.empty((nodes.size, nt) if by_node else (nt, nodes.size))
    ctx.call("hmg_curvedsky_node_weights", nodes.size, ctx.upload(nodes).ptr, l0, nl, nt, K.ptr, float(scale), int(by_node),
             R.ptr)
    return R


def curved_binned_from_cl_device(ells, C, theta_edges, kind, *, ctx=None):
    """curved_binned_from_cl with the result left on the device: a DeviceArray (ns, ntheta) for C of shape (ns, nn) (a
    host array or a DeviceArray)."""
    (kind,), _ = check_kinds(kind)
    nodes, l0, nl = check_nodes(ells)
    edges = check_edges(theta_edges)
    if not isinstance(C, nat.DeviceArray):
        C = np.asarray(C, dtype=np.float64)
        if not np.all(np.isfinite(C)):
            raise ValueError("C must be finite")
    if len(C.shape) != 2 or C.shape[1] != nodes.size or C.shape[0] < 1:
        raise ValueError(f"C must have shape (ns, {nodes.size}) with ns >= 1, got {tuple(C.shape)}")
    ctx = nat.context_or_default(ctx)
    R = node_weights_device(ctx, nodes, l0, nl, edges, kind, 0.5 / np.pi, by_node=True)
    return angcov._matmul(ctx, nat.as_device(ctx, C), R)


def curved_binned_from_cl(ells, C, theta_edges, kind, *, ctx=None):
    """Bin-averaged curved-sky correlation function xi_kind(bin i) = R_kind[i, :] . C / (2 pi)
    = sum_{l in L} (2l + 1)/(4 pi) K_kind(l; i) C(l) of the spectra C[..., :] at the nodes ells: the discretisation
    curved_cov_gaussian is the covariance of.  Returns C's leading shape with ntheta last."""
    Ch = np.asarray(C, dtype=np.float64)
    if Ch.ndim < 1:
        raise ValueError("C must have the nodes as its last axis")
    flat = Ch.reshape(-1, Ch.shape[-1])
    nt = np.size(theta_edges) - 1
    if flat.shape[0] == 0:
        check_kinds(kind), check_nodes(ells), check_edges(theta_edges)
        return np.empty(Ch.shape[:-1] + (nt,))
    return curved_binned_from_cl_device(ells, flat, theta_edges, kind, ctx=ctx).numpy().reshape(Ch.shape[:-1] + (nt,))


def curved_project_cl_cov_device(M, ells, theta_edges, kind1, kind2, *, ctx=None):
    """curved_project_cl_cov with the result left on the device: a DeviceArray (ntheta, ntheta)."""
    (k1,), _ = check_kinds(kind1)
    (k2,), _ = check_kinds(kind2)
    nodes, l0, nl = check_nodes(ells)
    edges = check_edges(theta_edges)
    if not isinstance(M, nat.DeviceArray):
        M = np.asarray(M, dtype=np.float64)
        if not np.all(np.isfinite(M)):
            raise ValueError("M must be finite")
    if tuple(M.shape) != (nodes.size, nodes.size):
        raise ValueError(f"M must have shape ({nodes.size}, {nodes.size}), got {tuple(M.shape)}")
    ctx = nat.context_or_default(ctx)
    R1 = node_weights_device(ctx, nodes, l0, nl, edges, k1, 0.5 / np.pi)
    R2 = node_weights_device(ctx, nodes, l0, nl, edges, k2, 0.5 / np.pi, by_node=True)
    return angcov._matmul(ctx, angcov._matmul(ctx, R1, nat.as_device(ctx, M)), R2)


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


def _by_index(probes, labels):
    index = {lab: i for i, lab in enumerate(labels)}
    pr = []
    for p in probes:
        if len(p) != 3 or p[0] not in index or p[1] not in index:
            raise ValueError(f"probe {p!r} must be (label, label2, kind) with labels out of {labels}")
        pr.append((index[p[0]], index[p[1]], p[2]))
    return pr


def curved_angular_cov_device(model, theta_edges, probes, fields, fsky, ells, term="total", shear_factor=True):
    """curved_angular_cov with the result left on the device."""
    labels, Ctab, noise, spins = curved_angular_spectra_device(model, fields, ells, term, shear_factor)
    return curved_cov_gaussian_device(ells, Ctab, noise, theta_edges, _by_index(probes, labels), fsky, spins=spins,
                                      ctx=model._ctx())


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
    pr = check_probes(_by_index(probes, labels), nf, spins)
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
