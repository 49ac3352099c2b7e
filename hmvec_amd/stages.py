"""The launch-only stages of a pass: a stage is a ``_native.*Part`` structure.  Alone it is one call of its own entry
point (ALONE: the part's fields in order are that entry's arguments); queued with others it shares a grouped launch
(plan).  Nothing here calls into the library: ``HaloModel`` issues what these functions return."""
import ctypes as C
from collections import namedtuple

from . import _native as nat

# kind -> (stand-alone entry, how many fields of the part come in front of the grid sizes, how many of (nz, nm, nk) the
# entry takes, fields of the part that are not arguments of it, does it run under the model's tag: see plan)
ALONE = {
    "nfw": ("hmg_nfw_analytic", 0, 3, (), False),
    "hod": ("hmg_hod", 0, 2, ("stage",), False),
    "rows": ("hmg_profile_rowparams", 1, 2, ("d_ks", "d_kts", "nk", "fft_m", "d_rowsc"), False),
    "fft": ("hmg_profile_fft", 0, 3, ("d_rowsc",), True),
}

# hmg_sigma2_halo_front's own arguments: sigma2 = (nz, nm, nq, d_PT, d_kq, d_wq, d_R, Wkr_taylor_switch), what every
# hmg_sigma2_* entry takes for the contraction; d_ms; halo = the HaloStageArgs
FrontArgs = namedtuple("FrontArgs", "sigma2 d_ms halo")

# Which queued stage must not run before which (a kind appears at most once in the queue): the HOD reads n, b; the
# profile FFT reads the row parameters.
RUNS_AFTER = {"hod": ("massfn",), "fft": ("rows",)}


def fields(part, skip=()):
    """The fields of a structure as a flat argument list: an embedded array by reference, a pointer as it is."""
    vals = [getattr(part, name) for name, _ in part._fields_ if name not in skip]
    return [C.byref(v) if isinstance(v, C.Array) else v for v in vals]


def alone(kind, part, dims):
    """The launch (entry, args, tagged) that runs one part alone on a grid of dims = (nz, nm, nk[, nq])."""
    entry, lead, ndims, skip, tagged = ALONE[kind]
    args = fields(part, skip)
    return entry, (*args[:lead], *dims[:ndims], *args[lead:]), tagged


def must_issue_first(pending_kinds, pending_dims, kind, dims):
    """Must the queue be issued before this stage joins it?  The same kind twice, a producer queued behind its own
    consumer (it would overwrite what the consumer still has to read), the front of a new pass (it rewrites what every
    queued stage reads), or a stage built for another grid than the queued ones."""
    return bool(pending_kinds) and (kind == "front" or kind in pending_kinds or dims != pending_dims
                                    or any(kind in RUNS_AFTER.get(k, ()) for k in pending_kinds))


def plan(stages, dims, prep, x):
    """The grouped launches a queue of (kind, part, keep) becomes, as ([(entry, args, tagged)], prepared): the front
    (sigma^2 contraction | halo stage | HOD occupations | Battaglia row parameters: inputs only), then the tensor group
    (per-z chain: sigma^2 second stage + n, b -> HOD sums -> coefficient rows of the mass integrals `prep` describes |
    profile FFT rows | NFW rows) - or, with no transform queued or its row parameters not riding with a front, the rows
    group (n, b tiles | row parameters | NFW rows), then the profile group (chain | profile FFT rows).  A `tagged` launch
    runs under the model's support tag and deferral flag; `prepared`: `prep` rides in one (hmg_power_batch_run then skips
    its preparation launch).  `x` is HMG_X, the experiment switches (tuning only).  No native call is made here."""
    st = {k: p for k, p, _ in stages}
    if not st:
        return [], False
    nz, nm, nk, nq = dims          # the sizes at queue time, not the model's current ones
    opt = lambda part: C.byref(part) if part is not None else None      # noqa: E731
    ref = lambda k: opt(st.get(k))      # noqa: E731
    prep = None if "prep_alone" in x else prep
    out, sums, d_prep = [], None, opt(prep)
    if "front" in st:
        occ = None
        if "hod" in st:      # the occupation numbers need inputs only: they ride in the front launch ...
            occ = nat.HodPart.from_buffer_copy(st["hod"])
            occ.stage, st["hod"].stage = nat.HOD_OCCUPATIONS, nat.HOD_SUMS
            sums = ref("hod")    # ... and n_gal, b_g, which need the n, b of this pass, in the chain of the tensor (or profile) group
        front = st.pop("front")
        # ... and so do the Battaglia row parameters: the thread that solves for M_200c goes on to them
        rows = st.pop("rows") if "rows" in st and "rows_alone" not in x else None
        out.append(("hmg_sigma2_halo_front", (*front.sigma2, front.d_ms, C.byref(front.halo), opt(occ), opt(rows)), False))
    elif "hod" in st:        # no front to ride with: the HOD's own kernel (n, b are there already)
        out.append(alone("hod", st.pop("hod"), dims))
    if "fft" in st and ("massfn" in st or "nfw" in st) and "rows" not in st and not x:
        # tensor group: chain (sigma^2 -> n, b -> HOD sums -> coefficient rows) | profile rows | NFW rows, one launch
        out.append(("hmg_group_tensors", (nz, nm, nk, nq, ref("massfn"), sums, d_prep, ref("nfw"), ref("fft")), True))
        return out, prep is not None
    nfw_alone = [alone("nfw", st.pop("nfw"), dims)] if "nfw_alone" in x and "nfw" in st else []
    if any(k in st for k in ("massfn", "rows", "nfw")):
        out.append(("hmg_group_rows", (nz, nm, nk, nq, ref("massfn"), None, ref("rows"), ref("nfw")), False))
    out += nfw_alone
    if "fft" not in st and sums is None:
        return out, False
    if "chain_alone" in x and "fft" in st and (sums is not None or prep is not None):
        # experiment: the per-z chain as a launch of its own in front of the stand-alone
        # row kernel (no private segment) instead of a role of the profile group
        out += [("hmg_group_profile", (nz, nm, nk, None, sums, d_prep), False),
                ("hmg_group_profile", (nz, nm, nk, ref("fft"), None, None), False)]
    else:
        out.append(("hmg_group_profile", (nz, nm, nk, ref("fft"), sums, d_prep), True))
    return out, prep is not None
