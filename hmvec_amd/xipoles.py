"""Redshift-space correlation multipoles xi_0(s), xi_2(s), xi_4(s) on the GPU: what a
spectroscopic survey measures, from the multipole spectra P_0, P_2, P_4(k) of section 19.

With f_i = k_i P_l,i and f~ the interpolant of ``xi_from_power`` (piecewise linear in k on [ks[0], ks[-1]], zero
outside),

    xi_l(s) = i^l / (2 pi^2) int k f~(k) j_l(k s) dk,      l = 0, 2, 4      (i^l = +1, -1, +1),

the integral taken in closed form panel by panel - no quadrature in k s.  The monopole is ``xi_from_power`` of the P_0
row, bit for bit.  ``xi_multipoles_from_power`` transforms tabulated rows; ``xi_multipoles_device(model, ...)`` and
``get_xi_multipoles(model, ...)`` transform a HaloModel's own multipoles where ``multipoles_device`` left them.  They
are functions of the model, as section 23's ``angular_cov(model, ...)`` is, not methods: the attribute surface of the
class is a recorded fixture (tests/golden/facade_surface.json) that this section leaves as it is.  The kernel is in
hmvec_amd/csrc/kernels/realspace.hpp.
"""
import numpy as np

from . import _native as nat
from . import realspace, rsd

__all__ = ["xi_multipoles_from_power", "xi_multipoles_device", "get_xi_multipoles"]


def check_ells(ells):
    """The orders of a request as a tuple of 0, 2, 4 (rsd.check_ells), at least one."""
    ells = rsd.check_ells(ells)
    if not ells:
        raise ValueError("ells is empty: at least one of (0, 2, 4) is needed")
    return ells


def multipole_rows(ctx, d_ks, bases, rows, nk, row_stride, node_stride, ss):
    """xi_l, l in `bases` ({l: device address of P_l's first row}), of `rows` device-resident rows of nk values read
    through (row_stride, node_stride) at the checked separations ss (non-empty): ONE launch for all orders; a
    DeviceArray (len(bases), rows, ns) in the order of `bases`."""
    ns, order = ss.size, list(bases)
    out = ctx.empty((len(order), rows, ns))
    xi = {ell: out.ptr + 8 * i * rows * ns for i, ell in enumerate(order)}
    d_ss = ctx.upload(ss)
    ctx.call("hmg_xi_multipoles", rows, nk, ns, d_ks.ptr, *(bases.get(ell) for ell in rsd.ELLS), row_stride, node_stride,
             d_ss.ptr, *(xi.get(ell) for ell in rsd.ELLS))
    return out


def xi_multipoles_from_power(ks, P, ss, ells=(0, 2, 4), *, ctx=None):
    """Correlation multipoles xi[i, ..., j] = xi_l(ss[j]), l = ells[i], of the multipole spectra P[i, ..., :] tabulated
    on ks, the sign i^l included.

    ks: (nk,) with nk >= 2, finite, positive, strictly increasing.  P: (nl, nk), (nl, nz, nk) or (nl, n, nz, nk) with one
    leading entry per order of ells, finite, as a host array or a DeviceArray (a resident block is taken as it is: its
    shape is checked, its values stay on the device).  ss: separations, finite and positive, in the inverse units of ks.
    ells: orders out of (0, 2, 4).  Returns a float64 array of P's shape with len(ss) in place of nk; the monopole is bit
    for bit xi_from_power of its rows.  Anything else raises ValueError before a launch."""
    ells = check_ells(ells)
    ks = realspace.check_ks(ks)
    nk, nl = ks.size, len(ells)
    shape = tuple(P.shape) if isinstance(P, nat.DeviceArray) else np.shape(P)
    if not 2 <= len(shape) <= 4 or shape[0] != nl or shape[-1] != nk:
        raise ValueError(f"P must have shape ({nl}, {nk}), ({nl}, nz, {nk}) or ({nl}, n, nz, {nk}) - one leading entry per "
                         f"order of ells = {ells} - got {tuple(shape)}")
    lead = tuple(int(v) for v in shape[1:-1])
    rows = int(np.prod(lead, dtype=np.int64))
    flat = (P.view(0, (nl * rows, nk)) if isinstance(P, nat.DeviceArray)
            else np.asarray(P, dtype=np.float64).reshape(nl * rows, nk))
    ks, flat, ss, _, _ = realspace._request(ks, flat, ss, "ss")
    if ss.size == 0 or rows == 0:
        return np.empty((nl,) + lead + (ss.size,))
    ctx, d_ks, d_P = realspace._resident(ks, flat, ctx)
    bases = {}
    for i, ell in enumerate(ells):                       # (an order named twice is transformed once, from its first rows)
        bases.setdefault(ell, d_P.ptr + 8 * i * rows * nk)
    out = multipole_rows(ctx, d_ks, bases, rows, nk, nk, 1, ss).numpy()
    order = list(bases)
    return np.stack([out[order.index(ell)] for ell in ells]).reshape((nl,) + lead + (ss.size,))


# ---------------------------------------------------------------- a HaloModel's own multipoles
# The (2, nz, nk, 3) block of multipoles_device is read in place by one strided launch over 2 nz rows; no spectrum
# crosses to the host.  The model is reached by the names DESIGN.md lists for its sections.
def xi_multipoles_device(model, ss, name, name2=None, ells=(0, 2, 4), nmu=16, sigma_s=None, f=None, alphas=(1, 0, 1),
                         damping=True, kindex=None):
    """The correlation multipoles ells (of 0, 2, 4) of the redshift-space spectrum of the pair (name, name2; default
    name) of the HaloModel `model` on the device, (2, nl, nz, ns) = (1-halo, 2-halo), at the separations ss (finite,
    positive, at least one; in the inverse units of ks): the transform of xi_multipoles_from_power of
    model.multipoles_device's P_l at all nodes of the k grid.  nmu, sigma_s, f, alphas, damping: see
    HaloModel.multipoles_device.  The transform needs the whole grid: a kindex is refused, as is a pressure name, before
    any launch."""
    ells = check_ells(ells)
    ss = realspace.check_rs(ss, "ss")
    if ss.size == 0:
        raise ValueError("ss is empty: at least one separation is needed")
    if kindex is not None:
        raise ValueError("kindex: the transform needs the multipoles at every node of the k grid")
    realspace.check_ks(model.ks)
    pl = model.multipoles_device(name, name2, nmu=nmu, kindex=None, sigma_s=sigma_s, f=f, alphas=alphas, damping=damping)
    ctx, nz, nk, ns = pl.ctx, model._nz, model._nk, ss.size
    bases = {}
    for ell in ells:
        bases.setdefault(ell, pl.ptr + 8 * rsd.ELLS.index(ell))
    xi = multipole_rows(ctx, model._d_ks(), bases, 2 * nz, nk, 3 * nk, 3, ss)        # (order, 2, nz, ns)
    order = list(bases)
    out = ctx.empty((2, len(ells), nz, ns))
    for t in range(2):
        for i, ell in enumerate(ells):
            ctx.call("hmg_memcpy_d2d", out.ptr + 8 * (t * len(ells) + i) * nz * ns,
                     xi.ptr + 8 * (order.index(ell) * 2 + t) * nz * ns, 8 * nz * ns)
    model._sync_point()
    return out


def get_xi_multipoles(model, ss, name, name2=None, ells=(0, 2, 4), term="total", nmu=16, sigma_s=None, f=None,
                      alphas=(1, 0, 1), damping=True, kindex=None):
    """The correlation multipoles ells (of 0, 2, 4) of the redshift-space spectrum of the pair of the HaloModel `model`
    at the separations ss on the host, shape (len(ells), nz, ns); term: "1h", "2h" or "total".  "total" is the sum of
    the two transforms; the transform is linear, so it equals the transform of the summed P_l to rounding, not bit for
    bit.  The monopole of "1h" and of "2h" is bit for bit
    xi_from_power(ks, model.get_power_multipoles(..., ells=(0,), term=term)[0], ss).  See xi_multipoles_device."""
    ells = check_ells(ells)
    rsd.check_term(term, rsd.TERMS)
    ss = realspace.check_rs(ss, "ss")
    if ss.size == 0:
        if kindex is not None:
            raise ValueError("kindex: the transform needs the multipoles at every node of the k grid")
        model._rsd_request(name, name2, None, sigma_s, f, alphas, damping)          # (the refusals of a request)
        return np.empty((len(ells), model._nz, 0))
    out = xi_multipoles_device(model, ss, name, name2, ells=ells, nmu=nmu, sigma_s=sigma_s, f=f, alphas=alphas,
                               damping=damping, kindex=kindex).numpy()
    return rsd.pick_term(out, term)
