"""``HaloModel`` — the drop-in boundary of the hot path (hmvec/hmvec.py:75-572).

Same constructor, ``add_*`` and ``get_power_*`` surface, argument meaning, error types
and stdout messages as the reference class, but every array lives in HBM and every
stage is a HIP kernel behind the C ABI in ``include/hmgrid.h``.  Host Python here only
wires pointers and scalars.  There is no CPU fallback.

State mirrors the reference: ``uk_profiles`` / ``pk_profiles`` map name -> (nz,nm,nk)
array, ``hods`` maps name -> dict, plus ``sigma2``, ``nzm``, ``bh``, ``Pzk``.  Reads of
those return numpy arrays (copied from the device on first access, then cached);
assigning a numpy array to ``uk_profiles[name]`` uploads it.
"""
import ctypes as C
import itertools
import os
from collections import namedtuple
from collections.abc import MutableMapping

import numpy as np
import scipy.constants as constants

from . import _native as nat
from . import bispectrum as bispec
from . import cov as covmod
from . import angular, realspace, spectra, stages
from . import rsd as rsdmod
from . import onepoint
from . import hod_ensemble as hodens
from .cosmology import Cosmology, _is_shared_product, _trapz, sigma2_kgrid, sigma2_weights
from .params import battaglia_defaults, default_params
from .quadrature import gradient_is_uniform, simpson_weights, trapz_weights
from .functions import FN_BG_INTEGRAND, FN_ST_FSIGMA, FN_TINKER_FSIGMA, fn2d, ngal_from_mthresh, trapz_lastaxis
from .functions import context as fn_context
from .utils import vectorized_bisection_search

_trapz = getattr(np, "trapezoid", None) or np.trapz
_EPOCHS = itertools.count(1)      # content tags of the per-model (z,m) arrays (hmg_profile_support_epoch)
_DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data")
# A cached pair of spectra: the model's state version it was computed for, P_1h and P_2h on the device and, from a batched
# launch, the host block of that launch (_HostBlock) with the two spectra's places in it
_Spectra = namedtuple("_Spectra", "version p1h p2h host i1h i2h", defaults=(None, None, None))


def _tinker_alpha_table():
    """alpha(z) normalisation table of Tinker+10 f(nu) (values of the table the
    reference ships as hmvec/data/alpha_consistency.txt, read at hmvec/tinker.py:64-66)."""
    with np.load(os.path.join(_DATA, "tinker10_alpha_of_z.npz")) as f:
        return f["z"], f["alpha"]


class DeviceDict(MutableMapping):
    """name -> DeviceArray with numpy reads (lazy D2H, cached) and numpy writes (H2D)."""

    def __init__(self, ctx_getter, on_change=None):
        self._ctx_getter = ctx_getter
        self._on_change = on_change or (lambda: None)
        self._dev = {}
        self._host = {}
        self._hint = {}       # name -> (d_nconst, d_cconst): constant-prefix hint emitted with the tensor

    def dev(self, name, fill=True):
        """The tensor on the device.  A pass of the facade leaves the whole tiles of a hinted tensor's constant prefix
        unwritten (hmg_prefix_deferral: the batched mass integrals never load them); every other reader gets them
        filled first - the context knows per buffer whether there is anything to fill.  fill=False is for the
        batched mass integrals alone."""
        d = self._dev[name]
        if fill and name in self._hint:
            self._ctx_getter().call("hmg_prefix_fill", d.ptr)
        return d

    def on_device(self, name, shape):
        """Is there a tensor of that name and shape?  No copy, no fill."""
        d = self._dev.get(name)
        return d is not None and d.shape == tuple(shape)

    def _pending(self, name):
        """True if a transform has left the prefix of this tensor unwritten since it was last filled."""
        if name not in self._hint:
            return False
        ctx = self._ctx_getter()          # (a transform still in the queue came through set_dev: no cached copy to protect)
        n = C.c_int()
        nat.check(ctx.lib.hmg_prefix_pending(ctx.handle, self._dev[name].ptr, C.byref(n)))
        return bool(n.value)

    def hint(self, name):
        """(nconst, cconst) device arrays of a profile produced by hmg_profile_fft, else (None, None)."""
        return self._hint.get(name, (None, None))

    def set_dev(self, name, darr, hint=None):
        self._dev[name] = darr
        self._host.pop(name, None)
        if hint is None:
            self._hint.pop(name, None)      # any other way of (re)defining the tensor drops the hint
        else:
            self._hint[name] = hint
        self._on_change()

    def __getitem__(self, name):
        # (a pending prefix means a transform has rewritten the buffer since the cached copy was made - a replayed
        # or re-issued pass does not come through set_dev)
        if name in self._host and self._pending(name):
            del self._host[name]
        if name not in self._host:
            self._host[name] = self.dev(name).numpy()
        return self._host[name]

    def __setitem__(self, name, value):
        if isinstance(value, nat.DeviceArray):
            self.set_dev(name, value)
        else:
            self.set_dev(name, self._ctx_getter().upload(np.asarray(value, dtype=np.float64)))

    def __delitem__(self, name):
        del self._dev[name]
        self._host.pop(name, None)
        self._hint.pop(name, None)
        self._on_change()

    def __contains__(self, name):      # Mapping's default would call __getitem__ (a D2H copy)
        return name in self._dev

    def __iter__(self):
        return iter(self._dev)

    def __len__(self):
        return len(self._dev)


class HodEntry(MutableMapping):
    """``hods[name]`` — same keys as the reference (hmvec/hmvec.py:452-460); array values
    are fetched from the device on first read."""

    _ARR = ("Nc", "Ns", "NsNsm1", "NcNs", "ngal", "bg")

    def __init__(self, dev, meta):
        self.dev = dev          # key -> DeviceArray
        self._vals = dict(meta)  # python-side values

    def __getitem__(self, k):
        if k not in self._vals:
            self._vals[k] = self.dev[k].numpy()
        return self._vals[k]

    def __setitem__(self, k, v):
        self._vals[k] = v

    def __delitem__(self, k):
        self._vals.pop(k, None)
        self.dev.pop(k, None)

    def __contains__(self, k):
        return k in self._vals or k in self.dev

    def __iter__(self):
        seen = list(self.dev) + [k for k in self._vals if k not in self.dev]
        return iter(seen)

    def __len__(self):
        return len(set(self.dev) | set(self._vals))


def _same_lookups(recs, what):
    """Refuse a request of `what` that names something the 1-halo and 2-halo lookups resolve differently."""
    for r in recs:
        if not r.same:
            raise ValueError(f"{what}: the 1-halo and 2-halo lookups resolve {r.name!r} differently (it names both an HOD "
                             f"and a profile)")


def _R_from_M(M, rho, delta):
    """hmvec/hmvec.py:627-628 for the handful of grid radii the constructor needs (host input
    preparation; the public, device-backed R_from_M lives in functions.py)."""
    return (3.0 * M / 4.0 / np.pi / delta / rho) ** (1.0 / 3.0)


class HaloModel(Cosmology):
    def __init__(self, zs, ks, ms=None, params={}, mass_function="sheth-torman",
                 halofit=None, mdef="vir", nfw_numeric=False, skip_nfw=False, accuracy="medium",
                 engine="camb", *, device=0, ctx=None, background=None):
        self.zs = np.asarray(zs, dtype=np.float64)
        self.ks = np.asarray(ks, dtype=np.float64)
        self._device = device
        self.ctx = ctx
        self.ms = self._ms_key = self._sync_serial = self._rho_m0_val = None
        self._version = self._epoch = self._nq = 0      # spectra-cache version; content tag of the (z,m) arrays; sigma^2 grid size
        self._aux_pending = self._m200c_valid = False
        Cosmology.__init__(self, params, halofit, engine=engine, accuracy=accuracy, background=background)

        self.mdef = mdef
        self.mode = mass_function
        self.hods = {}
        self._dcache = {}
        self._pool = {}
        self._use_lanes = os.environ.get("HMG_LANES", "0") == "1"   # two-stream overlap
        # Grouped launches: the launch-only stages of a pass are queued and issued when
        # something consumes them, so that stages which do not depend on each other share a launch.
        # HMG_NO_GROUPS=1 issues every stage as its own launch at call time (A/B timing, debugging).
        self._groups = os.environ.get("HMG_NO_GROUPS", "0") != "1" and not self._use_lanes
        self._stages = []
        self._stage_dims = None
        # The transforms of this model leave the left fill of a hinted tensor to whoever reads it (DeviceDict.dev;
        # DESIGN.md section 3).  False (or HMG_NO_PREFIX_DEFERRAL=1): they write every tensor whole (A/B timing, tests).
        self.prefix_deferral = os.environ.get("HMG_NO_PREFIX_DEFERRAL", "0") != "1"

        # (name, name2) -> _Spectra: a fused launch yields both terms, so the usual get_power_1halo(a,b) followed by
        # get_power_2halo(a,b) streams the tensors once; a batched launch enters every pair it computed, in both orders
        self._pcache = {}
        self.uk_profiles = DeviceDict(self._ctx, self._bump)
        self.pk_profiles = DeviceDict(self._ctx, self._bump)

        if ms is not None:
            self.ms = np.asarray(ms, dtype=np.float64)
            self.init_mass_function(self.ms)

        if not skip_nfw:
            self.add_nfw_profile("nfw", numeric=nfw_numeric)

    # ------------------------------------------------------------------ cosmology inputs
    def _init_cosmology(self, params, halofit):
        """hmvec/hmvec.py:96-102."""
        Cosmology._init_cosmology(self, params, halofit)
        if self.accuracy == "low":
            self.Pzk = self.P_lin_approx(self.ks, self.zs)
        else:
            self.Pzk = self._get_matter_power(self.zs, self.ks, nonlinear=False)
        if halofit is not None:
            self.nPzk = self._get_matter_power(self.zs, self.ks, nonlinear=True)

    def deltav(self, z):
        """Bryan & Norman virial overdensity (hmvec/hmvec.py:105-109)."""
        x = self.omz(z) - 1.0
        return 18.0 * np.pi ** 2.0 + 82.0 * x - 39.0 * x ** 2.0

    def _mdef_delta_rho(self):
        """(delta[z], rho[z]) of the halo mass definition (hmvec/hmvec.py:111-115)."""
        if self.mdef == "vir":
            return self.deltav(self.zs), self.rho_critical_z(self.zs)
        if self.mdef == "mean":
            return 200.0 + 0.0 * self.zs, self.rho_matter_z(self.zs)
        raise NotImplementedError(self.mdef)

    def rvir(self, m, z):
        """Host helper with the reference's signature (hmvec/hmvec.py:111-115)."""
        if self.mdef == "vir":
            return _R_from_M(m, self.rho_critical_z(z), delta=self.deltav(z))
        elif self.mdef == "mean":
            return _R_from_M(m, self.rho_matter_z(z), delta=200.0)

    def R_of_m(self, ms):
        return _R_from_M(ms, self.rho_matter_z(0), delta=1.0)

    # ------------------------------------------------------------------ device plumbing
    def _bump(self):
        """Any change of profiles / HODs / mass function invalidates cached spectra."""
        self._version += 1

    def _release_inputs(self, keys):
        """Drop cached device inputs.  Stages queued earlier (the constructor queues three) hold raw pointers to
        them and to pool buffers of the shapes they were built for: the queue is issued before anything is
        released, with the grid sizes recorded when it was built (_stage_dims)."""
        if self._stages:
            self._ctx().flush()
        for k in keys:
            self._dcache.pop(k, None)

    def _dev(self, key, builder):
        """Host array -> device, uploaded once per key (inputs of the path stay resident)."""
        if key not in self._dcache:
            self._dcache[key] = self._ctx().upload(builder())
        return self._dcache[key]

    # -- lanes (two-stream dataflow, HMG_LANES=1).  The main lane (0) carries the chip-filling kernels
    # in sequence - c, rvir -> NFW -> mass conversion + rows -> FFT -> spectra - and the auxiliary lane
    # (1) the short latency-bound chain sigma2 -> n(z,m), b(z,m) -> HOD, which only needs a few CUs
    # for a few microseconds at a time and so hides inside the big kernels' ramps and tails.  Ordering:
    # an auxiliary launch waits for the last SYNC POINT of the main lane (start of a pass / end of the
    # last spectra launch: whatever still reads n, b or the HOD arrays was enqueued before it), the
    # spectra wait for the auxiliary lane.  All events used inside a capture are recorded inside it.
    # Event slots 0..3 are reserved for this class (ShardedSpectra: 8-9, bench.py: 40 and up).
    _AUX = 1
    _EV_SYNC, _EV_AUX = 0, 1

    def _sync_point(self):
        if self._use_lanes:
            ctx = self._ctx()
            ctx.lane(0)
            ctx.record(self._EV_SYNC)
            self._sync_serial = ctx.capture_serial

    def _aux(self):
        """Route the next launches to the auxiliary lane (no-op without lanes)."""
        ctx = self._ctx()
        if self._use_lanes:
            if self._sync_serial != ctx.capture_serial:
                self._sync_point()          # first auxiliary launch of this capture / eager epoch
            ctx.lane(self._AUX)
            ctx.wait(self._EV_SYNC)
        return ctx

    def _aux_done(self):
        if self._use_lanes:
            ctx = self._ctx()
            ctx.record(self._EV_AUX)
            self._aux_pending = True
            ctx.lane(0)

    def _main(self, needs_aux=False):
        """Main lane; with needs_aux the launches that follow also wait for the auxiliary lane."""
        ctx = self._ctx()
        if self._use_lanes:
            ctx.lane(0)
            if needs_aux and self._aux_pending:
                ctx.wait(self._EV_AUX)
        return ctx

    def _buf(self, key, shape):
        """Output/workspace buffer allocated once per key, so that re-running a stage is
        launch-only: no allocation, no free, no host synchronisation."""
        shape = tuple(int(x) for x in shape)
        b = self._pool.get(key)
        if b is None or b.shape != shape:
            if b is not None:
                self._ctx().flush()       # a queued stage may still point at the block being replaced
            b = self._ctx().empty(shape)
            self._pool[key] = b
        return b

    @property
    def _nz(self):
        return self.zs.size

    @property
    def _nm(self):
        return self.ms.size

    @property
    def _nk(self):
        return self.ks.size

    def _d_zs(self):
        return self._dev("zs", lambda: self.zs)

    def _d_ks(self):
        return self._dev("ks", lambda: self.ks)

    def _d_ms(self):
        return self._dev("ms", lambda: self.ms)

    def _d_wm(self):
        return self._dev("wm", lambda: trapz_weights(self.ms))

    def _d_Pzk(self):
        return self._dev("Pzk", lambda: self.Pzk)

    def _lazy_host(self, name):
        h = "_h_" + name
        if getattr(self, h, None) is None:
            setattr(self, h, getattr(self, "_d_" + name).numpy())
        return getattr(self, h)

    sigma2 = property(lambda self: self._lazy_host("sigma2"))
    nzm = property(lambda self: self._lazy_host("nzm"))
    bh = property(lambda self: self._lazy_host("bh"))

    # ------------------------------------------------------------------ grouped launches
    def _stage(self, kind, part, keep=()):
        """One launch-only stage (stages.py).  With groups it is queued: anything that reads device state goes through
        the context, which issues the queue first (Context.flush), so deferral is invisible to callers.  Without, it is
        issued here as its own launch."""
        ctx = self._ctx()
        # The grid sizes a stage was built for travel with it: the raw pointers inside `part` belong to buffers
        # of exactly these sizes, whatever self.ms / self.ks are by the time the queue is issued.
        dims = (self._nz, self._nm if self.ms is not None else 0, self._nk, self._nq)
        if not self._groups:
            ctx.flush()          # deferred stages of ANY model on this context first: their own flush resets the tag
            return self._issue(ctx.call, [stages.alone(kind, part, dims)])
        if stages.must_issue_first([st[0] for st in self._stages], self._stage_dims, kind, dims):
            ctx.flush()
        self._stage_dims = dims
        self._stages.append((kind, part, keep))
        ctx.defer(self)

    def _drop_queue(self):       # (Context.capture: the capture these stages were queued in has failed)
        self._stages = []

    def _issue(self, call, launches):
        """Issue (entry, args, tagged) launches with `call` (ctx.call_now or ctx.call), a tagged one between this model's
        support tag and deferral flag.  Both are context state: set right around the ONE call they describe and restored
        whatever that call does (a call that raises inside a capture must not leave this model's tag behind: ADVICE r05)."""
        for entry, args, tagged in launches:
            if not tagged:
                call(entry, *args)
                continue
            call("hmg_profile_support_epoch", self._epoch)
            call("hmg_prefix_deferral", int(self.prefix_deferral))
            try:
                call(entry, *args)
            finally:
                call("hmg_prefix_deferral", 0)
                call("hmg_profile_support_epoch", 0)

    def _ks_ascending(self):
        """Is the target k grid ascending (the promise of the hint arrays and the row scalars)?  Cached per model."""
        if "ks_ascending" not in self._dcache:
            self._dcache["ks_ascending"] = (bool(np.all(np.diff(self.ks) > 0))
                                            and os.environ.get("HMG_NO_HINTS", "0") != "1")   # debugging switch
        return self._dcache["ks_ascending"]

    def _flush(self, prep=None):
        """Issue the queued stages as the grouped launches stages.plan makes of them.  Returns True if `prep` was issued
        with them (hmg_power_batch_run then skips its preparation launch)."""
        queued, self._stages = self._stages, []
        launches, prepared = stages.plan(queued, self._stage_dims, prep, os.environ.get("HMG_X", ""))
        self._issue(self._ctx().call_now, launches)
        return prepared

    # ------------------------------------------------------------------ mass function
    def get_sigma2(self):
        """hmvec/hmvec.py:121-124 — evaluated by hmg_sigma2."""
        return self.sigma2

    def _tinker_z_params(self):
        """Per-z scalars of Tinker+10 f(nu) (hmvec/tinker.py:53-66): z clamp with the
        heaviside(.,0) quirk (z == 3 -> 0, z > 3 -> 3) and alpha(z) from the table."""
        zs = self.zs
        zc = zs * np.heaviside(3 - zs, 0) + 3 * np.heaviside(zs - 3, 0)
        tz, ta = _tinker_alpha_table()
        if np.any(zc < tz[0]) or np.any(zc > tz[-1]):
            raise ValueError("A value in x_new is outside the interpolation range.")
        alpha = np.interp(zc, tz, ta)
        beta = 0.589 * (1 + zc) ** 0.20
        phi = -0.729 * (1 + zc) ** (-0.08)
        eta = -0.243 * (1 + zc) ** 0.27
        gamma = 0.864 * (1 + zc) ** (-0.01)
        return np.stack([alpha, beta, phi, eta, gamma], axis=1)

    def init_mass_function(self, ms):
        """sigma2, n(z,m), b(z,m), c(z,m), rvir(z,m) on the device (hmvec/hmvec.py:127-185).
        Inputs are uploaded on the first call; later calls only launch kernels."""
        ms = np.asarray(ms, dtype=np.float64)
        if self._ms_key is None or not np.array_equal(ms, self._ms_key):
            self._release_inputs([k for k in self._dcache if k != "zs" and k != "ks" and k != "Pzk"
                                  and not (isinstance(k, tuple) and k[0] == "fftgrid")])
            self._ms_key = ms.copy()
            # concentrations, radii and with them the support of every profile row and the modes it needs are
            # functions of (cosmology, zs, ks, ms): fixed per model until the mass grid changes.  The tag lets the
            # long-grid profile routes reuse the bound they measured once (hmg_profile_support_epoch) instead of
            # synchronising the stream in every call.
            self._epoch = next(_EPOCHS)
        self.ms = ms
        self._bump()
        if self.mode not in ("sheth-torman", "tinker"):
            raise NotImplementedError
        if self.mdef not in ("vir", "mean"):
            raise NotImplementedError
        ctx = self._ctx()
        nz, nm = self._nz, self._nm
        self._h_sigma2 = self._h_nzm = self._h_bh = None
        # sigma^2: inputs (P(k) on the sigma2 grid, Simpson weights, Lagrangian radii)
        if "sig_in" not in self._dcache:
            kmin, kmax, numks = self.p["sigma2_kmin"], self.p["sigma2_kmax"], self.p["sigma2_numks"]
            kq = sigma2_kgrid(kmin, kmax, numks)
            if self.accuracy == "high":
                self.sPzk = self.P_lin_slow(kq, self.zs, kmax=kmax)
            elif self.accuracy == "medium":
                self.sPzk = self.P_lin(kq, self.zs)
            else:
                self.sPzk = self._P_lin_approx_shared(kq, self.zs)
            wq = sigma2_weights(kq)
            # P(k',z) is an input of the path: uploaded and laid out once as the contraction reads it - once per
            # MODEL, or once per host array when the provider hands out the same read-only array again (the analytic
            # provider does for a repeated cosmology: Cosmology.P_lin_approx), together with the grid and its weights
            owned = _is_shared_product(self.sPzk)       # (the provider's own cached product: nothing modifies it)
            shared = ctx.shared.get(id(self.sPzk)) if owned else None
            if shared is None or shared[0] is not self.sPzk:
                d_sP = ctx.upload(self.sPzk)
                n = C.c_size_t()
                nat.check(ctx.lib.hmg_sigma2_layout_size(nz, kq.size, C.byref(n)))
                d_PT = ctx.empty((n.value,))
                ctx.call("hmg_sigma2_prepare", nz, kq.size, d_sP.ptr, d_PT.ptr)
                shared = (self.sPzk, d_PT, ctx.upload(kq), ctx.upload(wq))
                if owned:
                    if len(ctx.shared) >= 4:
                        ctx.flush()           # (queued stages of other models may hold addresses of an evicted entry)
                        ctx.shared.clear()
                    ctx.shared[id(self.sPzk)] = shared
            self._dcache["sig_in"] = shared[1:] + (ctx.upload(self.R_of_m(ms)),)
        d_PT, d_kq, d_wq, d_R = self._dcache["sig_in"]
        self._sync_point()               # start of a pass: everything launched so far precedes it
        ctx = self._aux()
        self._d_sigma2 = self._buf("sigma2", (nz, nm))
        # n(z,m), b(z,m): same launch as the second stage of the sigma^2 contraction
        if "mf_in" not in self._dcache:
            lnm = np.log(ms)
            uniform, step = gradient_is_uniform(lnm)
            par = nat.MassFnParams(
                mode=nat.MF_SHETH_TORMEN if self.mode == "sheth-torman" else nat.MF_TINKER10,
                deltac=self.p["st_deltac"], st_A=self.p["st_A"], st_a=self.p["st_a"], st_p=self.p["st_p"],
                rho_m0=float(self.rho_matter_z(0)[0]), lnm_uniform=int(uniform), lnm_step=step)
            d_tz = ctx.upload(self._tinker_z_params()) if self.mode == "tinker" else None
            delta, rho = self._mdef_delta_rho()
            self._dcache["mf_in"] = (par, ctx.upload(lnm), d_tz, ctx.upload(delta), ctx.upload(rho))
            ctx = self._aux()            # (the uploads above synchronise on whatever lane is current)
        par, d_lnm, d_tz, d_delta, d_rho = self._dcache["mf_in"]
        self._d_nzm, self._d_bh = self._buf("nzm", (nz, nm)), self._buf("bh", (nz, nm))
        d_ms = self._d_ms()
        # c(z,m), rvir(z,m), rs(z,m), the series rows of the analytic NFW kernel and the vir -> 200c mass
        # conversion the Battaglia profiles need: one thread per (z,m), independent of sigma2
        self._d_cs, self._d_rvir, self._d_rs = (self._buf(k, (nz, nm)) for k in ("cs", "rvir", "rs"))
        self._d_nfw_series = self._buf("nfw_series", (nz, nm, nat.NFW_SERIES_STRIDE))
        m2, r2, d_drho1, d_rhoc = self._m200c_io()
        duffy = tuple(float(self.p[f"duffy_{k}_{self.mdef}"]) for k in ("A", "alpha", "beta"))
        halo = nat.HaloStageArgs(self._d_zs().ptr, d_delta.ptr, d_rho.ptr, *duffy, float(self.h),
                                 self._d_cs.ptr, self._d_rvir.ptr, self._d_rs.ptr, self._d_nfw_series.ptr,
                                 d_drho1.ptr, 200.0, d_rhoc.ptr, m2.ptr, r2.ptr)
        massfn = nat.MassFnPart(C.pointer(par), d_ms.ptr, d_lnm.ptr, nat.ptr(d_tz), self._d_sigma2.ptr, self._d_nzm.ptr, self._d_bh.ptr)
        front = stages.FrontArgs((nz, nm, d_kq.size, d_PT.ptr, d_kq.ptr, d_wq.ptr, d_R.ptr,
                                  float(self.p["Wkr_taylor_switch"])), d_ms.ptr, halo)
        if self._groups:
            # front group: the contraction beside the halo stage (both need inputs only); the second stage of
            # the contraction and n(z,m), b(z,m) are queued as the first link of the per-z chain
            self._nq = int(d_kq.size)
            self._stage("front", front)
            self._stage("massfn", massfn, keep=(par,))
        elif not self._use_lanes:
            # one launch behind the contraction: mass function and halo stage side by side
            ctx.call("hmg_sigma2_massfn_halo", *front.sigma2, *stages.fields(massfn), C.byref(halo))
        else:
            # two-lane scheme: n, b on the auxiliary lane, the halo stage on the main lane ahead of the profiles
            ctx.call("hmg_sigma2_massfn", *front.sigma2, *stages.fields(massfn))
            self._aux_done()
            ctx = self._main()
            ctx.call("hmg_halo_stage", nz, nm, d_ms.ptr, *stages.fields(halo))
        self._m200c_valid = True

    def get_fsigmaz(self):
        """Multiplicity function f(sigma, z) on the (z,m) grid (hmvec/hmvec.py:133-147).  The path
        itself never materialises it (hmg_massfn goes from sigma^2 straight to n and b); this
        getter evaluates it on the device for callers that ask."""
        dc = self.p["st_deltac"]
        with fn_context(self._ctx()):
            if self.mode == "sheth-torman":
                return fn2d(FN_ST_FSIGMA, [self.sigma2], [self.p["st_A"], self.p["st_a"], self.p["st_p"], dc])
            if self.mode == "tinker":
                tz, ta = _tinker_alpha_table()
                return fn2d(FN_TINKER_FSIGMA, [self.sigma2, self.zs[:, None]], [1.0, 0.368, float(tz.size), dc],
                            tables=(tz, ta))
        raise NotImplementedError

    def get_bh(self):
        return self.bh

    def get_nzm(self):
        return self.nzm

    def concentration(self, mode="duffy"):
        """hmvec/hmvec.py:163-176."""
        if mode != "duffy":
            raise NotImplementedError
        return self._d_cs.numpy()

    # ------------------------------------------------------------------ profiles
    def _m200c_io(self):
        """Outputs and inputs of the vir -> 200c mass conversion on the device: (m200c, r200c, Delta rho_vir(z), rho_crit(z))."""
        return (self._buf("m200c", (self._nz, self._nm)), self._buf("r200c", (self._nz, self._nm)), self._d_drho1(),
                self._dev("rhocz", lambda: self.rho_critical_z(self.zs)))

    def _m200c(self):
        """(m200c, r200c) on the device (hmvec/hmvec.py:216-225)."""
        m2, r2, d1, d_rhoc = self._m200c_io()
        if not self._m200c_valid:
            self._ctx().call("hmg_mdelta_convert", self._nz, self._nm, self._d_ms().ptr, self._d_cs.ptr, d1.ptr, 200.0,
                             d_rhoc.ptr, m2.ptr, r2.ptr)
            self._m200c_valid = True
        return m2, r2

    def _d_drho1(self):
        """Delta * rho(z) of the model's own mass definition (hmvec/hmvec.py:217-220)."""
        def drho1():
            delta, rho = self._mdef_delta_rho()
            return rho * delta if self.mdef == "vir" else rho * 200.0
        return self._dev("drho1", drho1)

    def _fft_grids(self, xmax, nxs):
        """x grid and FFT wavenumber grid exactly as hmvec/fft.py:45-50,73 build them."""
        key = ("fftgrid", float(xmax), int(nxs))
        if key not in self._dcache:
            xs = np.linspace(0.0, xmax, nxs + 1)[1:]
            step = (xs[-1] - xs[0]) / xs.size
            kts = np.fft.rfftfreq(xs.size, step) * 2 * np.pi
            ctx = self._ctx()
            d_xs = ctx.upload(xs)
            d_lx = ctx.empty((xs.size,))            # ln x_n, shared by every row of every pass
            ctx.call("hmg_profile_fft_logx", xs.size, d_xs.ptr, d_lx.ptr)
            self._dcache[key] = (d_xs, ctx.upload(kts), float(step), d_lx)
        return self._dcache[key]

    def _profile_fft(self, key, nxs, xmax, rowp, consts, gamma, d_cmax, d_rss, do_mass_norm, d_post=None, d_rowsc=None):
        """One hmg_profile_fft launch; returns (tensor, hint).  The hint - how many leading target wavenumbers of each row
        lie below the row's first FFT mode, and the value np.interp's left fill gives them all - lets the batched mass
        integrals skip those parts of the tensor.  It is only requested when the target k grid is ascending."""
        nz, nm, nk = self._nz, self._nm, self._nk
        d_xs, d_kts, step, d_lx = self._fft_grids(xmax, nxs)
        out = self._buf(key, (nz, nm, nk))
        # nconst is an int32 array: allocated as (nz*nm+1)//2 doubles, viewed as integers on read
        hint = ((self._buf((key, "nconst"), ((nz * nm + 1) // 2,)), self._buf((key, "cconst"), (nz, nm)))
                if self._ks_ascending() else None)
        # (the row scalars only travel with the hint arrays: they carry the left-fill count, which needs ks ascending)
        self._stage("fft", nat.ProfileFftPart(
            int(nxs), step, d_xs.ptr, d_kts.ptr, *(nat.ptr(r) for r in rowp), *(float(c) for c in consts), float(gamma),
            d_cmax.ptr, d_rss.ptr, self._d_zs().ptr, self._d_ks().ptr, int(do_mass_norm), nat.ptr(d_post), out.ptr,
            nat.ptr(hint[0] if hint else None), nat.ptr(hint[1] if hint else None), d_lx.ptr,
            nat.ptr(d_rowsc if hint else None)))
        return out, hint

    def _battaglia_rowparams(self, key, kind, fit9, gamma, alpha_const, pref, post_pref, nxs=None, xmax=None):
        """Row parameters of a Battaglia family; returns (outs, d_rowsc): with a radial grid (nxs, xmax) and an ascending
        k grid the queued stage also leaves the output-side scalars of every row for the transform (hmg_rows_part,
        ABI 8), d_rowsc is then the buffer to hand to _profile_fft, else None."""
        nz, nm = self._nz, self._nm
        outs = [self._buf((key, "rowp", i), (nz, nm)) for i in range(7)]
        fit = (C.c_double * 9)(*fit9)
        d_hz = self._dev("hz", lambda: self.h_of_z(self.zs))
        m200c, r200c, d_drho1, d_rhoc = self._m200c_io()
        if not self._m200c_valid:
            # mass conversion and row parameters in one launch
            self._ctx().call("hmg_profile_rows_from_mvir", kind, nz, nm, self._d_ms().ptr, self._d_cs.ptr,
                             self._d_rvir.ptr, self._d_zs().ptr, d_drho1.ptr, 200.0, d_rhoc.ptr, d_hz.ptr,
                             C.byref(fit), float(gamma), float(alpha_const), float(pref), float(post_pref),
                             m200c.ptr, r200c.ptr, *[o.ptr for o in outs])
            self._m200c_valid = True
            return outs, None
        d_rowsc, extra = None, (None, None, 0, 0, None)
        if (self._groups and nxs is not None and nxs % 2 == 0 and os.environ.get("HMG_NO_ROWSC", "0") != "1"
                and self._ks_ascending()):
            d_kts = self._fft_grids(xmax, nxs)[1]
            d_rowsc = self._buf((key, "rowsc"), (nz, nm, nat.ROWSC_STRIDE))
            extra = (self._d_ks().ptr, d_kts.ptr, self._nk, int(nxs) // 2, d_rowsc.ptr)
        self._stage("rows", nat.RowsPart(kind, m200c.ptr, r200c.ptr, self._d_rvir.ptr, self._d_zs().ptr, d_rhoc.ptr,
                                         d_hz.ptr, fit, float(gamma), float(alpha_const), float(pref),
                                         float(post_pref), *[o.ptr for o in outs], *extra))
        return outs, d_rowsc

    def _battaglia_pparams(self, own, family_key, family, param_override):
        """Fit numbers of a Battaglia family: the model's own parameters `own`, the family's defaults, then the overrides
        that name one of them (other keys are ignored, hmvec/hmvec.py:198-213, 261-276)."""
        if family is None:
            family = self.p[family_key]
        pparams = {k: self.p[k] for k in own}
        pparams.update(battaglia_defaults[family])
        if param_override is not None:
            for key in param_override.keys():
                if key in own or key in battaglia_defaults[family]:
                    pparams[key] = param_override[key]
        return pparams

    def _battaglia_gas_pparams(self, family, param_override):
        return self._battaglia_pparams(("battaglia_gas_gamma",), "battaglia_gas_family", family, param_override)

    def _battaglia_pres_pparams(self, family, param_override):
        return self._battaglia_pparams(("battaglia_pres_gamma", "battaglia_pres_alpha"), "battaglia_pres_family", family,
                                       param_override)

    def add_battaglia_profile(self, name, family=None, param_override=None, nxs=None, xmax=None,
                              ignore_existing=False):
        """Battaglia+16 gas density profile -> uk_profiles[name] (hmvec/hmvec.py:188-250)."""
        if not (ignore_existing):
            assert name not in self.uk_profiles.keys(), "Profile name already exists."
        assert name != "nfw", "Name nfw is reserved."
        if nxs is None:
            nxs = self.p["electron_density_profile_integral_numxs"]
        if xmax is None:
            xmax = self.p["electron_density_profile_integral_xmax"]
        if param_override is not None:
            print(param_override)
        pparams = self._battaglia_gas_pparams(family, param_override)
        omb = self.p["ombh2"] / self.h ** 2.0
        gamma = pparams["battaglia_gas_gamma"]
        fit9 = [pparams[a + b] for a in ("rho0_", "alpha_", "beta_") for b in ("A0", "alpham", "alphaz")]
        key = ("uk", name)
        self._main()
        (amp, xc, alpha, expo, cmax, rscale, _post), rowsc = self._battaglia_rowparams(
            key, nat.PROF_BATTAGLIA_GAS, fit9, gamma, 0.0, omb / self.omm0, 0.0, nxs=nxs, xmax=xmax)
        out, hint = self._profile_fft(key, nxs, xmax, (amp, None, alpha, expo), (0.0, 1.0, 0.0, 0.0), gamma,
                                      cmax, rscale, True, d_rowsc=rowsc)
        self.uk_profiles.set_dev(name, out, hint)

    def add_battaglia_pres_profile(self, name, family=None, param_override=None, nxs=None, xmax=None,
                                   ignore_existing=False):
        """Battaglia+12 electron pressure profile -> pk_profiles[name] (hmvec/hmvec.py:252-316)."""
        if not (ignore_existing):
            assert name not in self.pk_profiles.keys(), "Profile name already exists."
        assert name != "nfw", "Name nfw is reserved."
        if nxs is None:
            nxs = self.p["electron_pressure_profile_integral_numxs"]
        if xmax is None:
            xmax = self.p["electron_pressure_profile_integral_xmax"]
        pparams = self._battaglia_pres_pparams(family, param_override)
        omb = self.p["ombh2"] / self.h ** 2.0
        gamma, alpha = pparams["battaglia_pres_gamma"], pparams["battaglia_pres_alpha"]
        fit9 = [pparams[a + b] for a in ("P0_", "xc_", "beta_") for b in ("A0", "alpham", "alphaz")]
        XH = 0.76
        eFrac = 2.0 * (XH + 1.0) / (5.0 * XH + 3.0)
        G_newt = constants.G / (default_params["parsec"] * 1e6) ** 3 * default_params["mSun"]
        pref = eFrac * (omb / self.omm0) * 200 * G_newt
        sigmaT = constants.physical_constants["Thomson cross section"][0]
        mElect = constants.physical_constants["electron mass"][0] / default_params["mSun"]
        post_pref = 4 * np.pi * (sigmaT / (mElect * constants.c ** 2))
        key = ("pk", name)
        self._main()
        (amp, xc, _alpha, expo, cmax, rscale, post), rowsc = self._battaglia_rowparams(
            key, nat.PROF_BATTAGLIA_PRES, fit9, gamma, alpha, pref, post_pref, nxs=nxs, xmax=xmax)
        out, hint = self._profile_fft(key, nxs, xmax, (amp, xc, None, expo), (0.0, 0.0, alpha, 0.0), gamma,
                                      cmax, rscale, False, d_post=post, d_rowsc=rowsc)
        self.pk_profiles.set_dev(name, out, hint)

    def add_nfw_profile(self, name, numeric=False, nxs=None, xmax=None, ignore_existing=False):
        """NFW u(k|m,z): analytic Si/Ci or numeric FFT branch (hmvec/hmvec.py:318-355).
        Returns (ks, uk) like the reference."""
        if not (ignore_existing):
            assert name not in self.uk_profiles.keys(), "Profile name already exists."
        if nxs is None:
            nxs = self.p["nfw_integral_numxs"]
        if xmax is None:
            xmax = self.p["nfw_integral_xmax"]
        self._main()
        if numeric:
            # rho = 1/x/(1+x)^2 is the gamma=-1, alpha=1, expo=2 member of the family
            out, hint = self._profile_fft(("uk", name), nxs, xmax, (None, None, None, None), (1.0, 1.0, 1.0, 2.0),
                                          -1.0, self._d_cs, self._d_rs, True)
        else:
            out, hint = self._buf(("uk", name), (self._nz, self._nm, self._nk)), None
            self._stage("nfw", nat.NfwPart(self._d_cs.ptr, self._d_rs.ptr, self._d_zs().ptr, self._d_ks().ptr,
                                           self._d_nfw_series.ptr, out.ptr))
        self.uk_profiles.set_dev(name, out, hint)
        return self.ks, _LazyArray(self.uk_profiles, name)

    # ------------------------------------------------------------------ HOD
    _HOD_PARAMS = ["hod_sig_log_mstellar", "hod_bisection_search_min_log10mthresh",
                   "hod_bisection_search_max_log10mthresh", "hod_bisection_search_rtol",
                   "hod_bisection_search_warn_iter", "hod_alphasat", "hod_Bsat",
                   "hod_betasat", "hod_Bcut", "hod_betacut", "hod_A_log10mthresh"]

    def _hod_device(self, key, log10mstar_thresh, pparams, corr):
        """One hmg_hod launch into the buffers of `key`; returns dict of DeviceArrays."""
        ctx = self._ctx()
        nz, nm = self._nz, self._nm
        par = nat.HodParams(pparams["hod_sig_log_mstellar"], pparams["hod_alphasat"], pparams["hod_Bsat"],
                            pparams["hod_betasat"], pparams["hod_Bcut"], pparams["hod_betacut"], {"max": 0, "min": 1}[corr])
        thr = np.ascontiguousarray(log10mstar_thresh, dtype=np.float64)
        cached = self._dcache.get(("thr", key))
        if cached is None or cached[0].shape != thr.shape:
            if cached is not None:
                self._release_inputs([("thr", key)])
            cached = (thr.copy(), ctx.upload(thr))
            self._dcache[("thr", key)] = cached
        elif not np.array_equal(cached[0], thr):
            # new thresholds go into the SAME device buffer (stream-ordered behind the launches that
            # read the old ones): nothing is freed, so nothing synchronises the other lanes
            ctx.write(cached[1], thr)
            cached[0][...] = thr
        d_thr = cached[1]
        out = {k: self._buf((key, k), (nz, nm)) for k in ("Nc", "Ns", "NsNsm1", "NcNs")}
        out["ngal"], out["bg"] = self._buf((key, "ngal"), (nz,)), self._buf((key, "bg"), (nz,))      # (HodPart's order)
        d_wm, d_ms, d_zs = self._d_wm(), self._d_ms(), self._d_zs()     # (uploads, if any, before the lane switch)
        self._aux()              # (both are no-ops without lanes, and a model with lanes queues nothing)
        self._stage("hod", nat.HodPart(nat.HOD_ALL, C.pointer(par), d_zs.ptr, d_ms.ptr, d_thr.ptr, self._d_nzm.ptr,
                                       self._d_bh.ptr, d_wm.ptr, *(o.ptr for o in out.values())), keep=(par,))
        self._aux_done()
        return out

    def add_hod(self, name, mthresh=None, ngal=None, corr="max", satellite_profile_name="nfw",
                central_profile_name=None, ignore_existing=False, param_override=None):
        """Specify an HOD by stellar-mass threshold or by number density (hmvec/hmvec.py:357-460)."""
        if not (ignore_existing):
            assert name not in self.uk_profiles.keys(), "HOD name already used by profile."
        assert satellite_profile_name in self.uk_profiles.keys(), "No matter profile by that name exists."
        if central_profile_name is not None:
            assert central_profile_name in self.uk_profiles.keys(), "No matter profile by that name exists."
        if not (ignore_existing):
            assert name not in self.hods.keys(), "HOD with that name already exists."
        pparams = {ip: self.p[ip] for ip in self._HOD_PARAMS}
        if param_override is not None:
            for key in param_override.keys():
                if key in self._HOD_PARAMS:
                    pparams[key] = param_override[key]
                else:
                    raise ValueError  # not an HOD parameter
        if corr not in ("max", "min"):
            raise ValueError(corr)

        if ngal is not None:
            ngal = np.asarray(ngal)
            if ngal.size != self.zs.size:
                raise ValueError("ngal has to be a vector of size self.zs")
            assert mthresh is None
            log10mthresh = self._bisect_mthresh(ngal.astype(np.float64), pparams)
            mthresh = 10 ** (log10mthresh * pparams["hod_A_log10mthresh"])
        try:
            assert mthresh.size == self.zs.size
        except Exception:
            raise ValueError("mthresh has to be a vector of size self.zs")

        l10 = np.log10(np.asarray(mthresh, dtype=np.float64))
        dev = self._hod_device(("hod", name), l10, pparams, corr)
        self._bump()
        self.hods[name] = HodEntry(dev, dict(satellite_profile=satellite_profile_name,
                                             central_profile=central_profile_name,
                                             log10mthresh=np.log10(mthresh[:, None])))

    def _bisect_mthresh(self, ngal, pparams, full_model=None):
        """Bisection on log10 mthresh with the reference's GLOBAL stop test over z
        (hmvec/utils.py:9-42 called at hmvec/hmvec.py:426-433).  Every z keeps bisecting
        until all z meet rtol, so the answer depends on the whole z vector."""
        def ngal_of(log10mthresh):       # the device HOD kernel's n_gal(z) for trial thresholds
            return self._hod_device(("hod", "_bisect"), log10mthresh, pparams, "max")["ngal"].numpy()

        return vectorized_bisection_search(ngal, ngal_of,
                                           [pparams["hod_bisection_search_min_log10mthresh"],
                                            pparams["hod_bisection_search_max_log10mthresh"]],
                                           "decreasing", rtol=pparams["hod_bisection_search_rtol"], verbose=True,
                                           hang_check_num_iter=pparams["hod_bisection_search_warn_iter"])

    def get_ngal(self, Nc, Ns):
        """hmvec/hmvec.py:462."""
        with fn_context(self._ctx()):
            return ngal_from_mthresh(nzm=self.nzm, ms=self.ms, Ncs=Nc, Nss=Ns)

    def get_bg(self, Nc, Ns, ngal):
        """hmvec/hmvec.py:464-466."""
        with fn_context(self._ctx()):
            return trapz_lastaxis(fn2d(FN_BG_INTEGRAND, [self.nzm, Nc, Ns, self.bh]), self.ms) / ngal

    # ------------------------------------------------------------------ spectra
    # What a request becomes is decided in spectra.py, on records: a public call resolves each of its names once
    # (_resolve) and hands the records on.
    def _resolve(self, *names):
        """One spectra.Resolved per name."""
        memo = {}
        for nm_ in names:
            if nm_ not in memo:
                memo[nm_] = spectra.resolve(nm_, self.hods, self.uk_profiles, self.pk_profiles)
        return [memo[nm_] for nm_ in names]

    def _resolve_pairs(self, pairs):
        recs = self._resolve(*[nm_ for a, b in pairs for nm_ in (a, a if b is None else b)])
        return list(zip(recs[0::2], recs[1::2]))

    def _tracer(self, rec, term, fill=True):
        """The hmg_tracer of a resolved name as the 1-halo (term 1) or the 2-halo lookup (term 2) finds it.  fill=False:
        the tracer is for the batched mass integrals (they read no deferred tile of a hinted tensor) - nothing is enqueued."""
        kind, tensors = rec.found(term)
        shape = (self._nz, self._nm, self._nk)
        got = []          # per tensor: its pointer and those of its hint arrays
        for tag, nm_ in tensors:
            dd = self.uk_profiles if tag == "uk" else self.pk_profiles
            # (a kernel trusts the pointer it is handed: a hand-assigned entry of another shape must stop here - numpy
            # would refuse to broadcast it in the reference, hmvec/hmvec.py:516-550)
            d_ = dd.dev(nm_, fill=fill)
            if d_.shape != shape:
                raise ValueError(f"profile {nm_!r} has shape {d_.shape}, the model's grid is {shape}")
            nconst, cconst = dd.hint(nm_)
            got.append((d_.ptr, nat.ptr(nconst), nat.ptr(cconst)))
        prof, nconst, cconst = got[0]
        if kind != "h":
            return nat.Tracer(nat.TRACER_MATTER if kind == "m" else nat.TRACER_PRESSURE, prof, None, None, None, None, None,
                              None, None, nconst, cconst)
        d = self.hods[rec.name].dev
        cprof, cnconst, ccconst = got[1] if len(got) > 1 else (None, None, None)
        return nat.Tracer(nat.TRACER_HOD, prof, cprof, d["Nc"].ptr, d["Ns"].ptr, d["NcNs"].ptr, d["NsNsm1"].ptr, d["ngal"].ptr,
                          None, nconst, cconst, cnconst, ccconst)

    def _power_launch(self, ta, tb, want1, want2, out1=None, out2=None):
        ctx = self._main(needs_aux=True)
        nz, nm, nk = self._nz, self._nm, self._nk
        d1 = (out1 if out1 is not None else ctx.empty((nz, nk))) if want1 else None
        d2 = (out2 if out2 is not None else ctx.empty((nz, nk))) if want2 else None
        ctx.call("hmg_power", nz, nm, nk, C.byref(ta), C.byref(tb), self._d_nzm.ptr, self._d_bh.ptr,
                 self._d_ms().ptr, self._d_wm().ptr, self._d_ks().ptr, self._d_Pzk().ptr,
                 self._rho_m0(), float(self.p["kstar_damping"]), nat.ptr(d1), nat.ptr(d2))
        self._sync_point()
        return d1, d2

    def _rho_m0(self):
        if self._rho_m0_val is None:
            self._rho_m0_val = float(self.rho_matter_z(0)[0])
        return self._rho_m0_val

    def power_device(self, name, name2=None, b1_in=None, b2_in=None, want=("1h", "2h"), out1=None, out2=None):
        """Device-resident (P1h, P2h) DeviceArrays of shape (nz, nk) — one fused pass over the
        profile tensors when the 1-halo and 2-halo code paths resolve the names identically."""
        return self._power_pair(*self._resolve(name, name if name2 is None else name2), b1_in, b2_in, want, out1, out2)

    def _power_pair(self, ra, rb, b1_in=None, b2_in=None, want=("1h", "2h"), out1=None, out2=None):
        keep = []
        want1, want2 = "1h" in want, "2h" in want
        same = ra.same and rb.same
        self._main()          # (the tracers below may enqueue a fill: on the lane of the transforms)
        a1, b1 = self._tracer(ra, 1), self._tracer(rb, 1)
        a2, b2 = (self._tracer(ra, 2), self._tracer(rb, 2)) if want2 and not same else (a1, b1)
        if want2:
            if b1_in is not None:
                keep.append(self._ctx().upload(np.asarray(b1_in, dtype=np.float64).reshape(-1)))
                a2.d_bias_override = keep[-1].ptr
            if b2_in is not None:
                n = b1_in.shape[0]     # reference reshapes b2_in with b1_in's length (hmvec.py:561)
                keep.append(self._ctx().upload(np.asarray(b2_in, dtype=np.float64).reshape((n, 1))))
                b2.d_bias_override = keep[-1].ptr
        if want1 and want2 and same:
            d1, d2 = self._power_launch(a2, b2, True, True, out1, out2)
        else:
            d1 = self._power_launch(a1, b1, True, False, out1, None)[0] if want1 else None
            d2 = self._power_launch(a2, b2, False, True, None, out2)[1] if want2 else None
        if keep:
            self._ctx().sync()
        return d1, d2

    def power_device_batch(self, pairs, outs1=None, outs2=None):
        """(P1h, P2h) DeviceArrays for SEVERAL (name, name2) pairs with every distinct profile
        tensor streamed from HBM once for the whole batch (hmg_power_batch) instead of once
        per pair.  Falls back to one fused launch per pair when the batch cannot express the
        reference's semantics (spectra.batchable: two different HOD / two different pressure names, a name
        that the 1-halo and 2-halo code paths resolve differently, more than 4 tracers)."""
        return self._power_batch(self._resolve_pairs(pairs), outs1, outs2)

    def _power_batch(self, pairs, outs1=None, outs2=None):
        ctx = self._ctx()
        nz, nm, nk = self._nz, self._nm, self._nk
        recs, uniq, alias, first = spectra.pair_plan(pairs)
        # (every tensor of the request is checked before anything is allocated or launched)
        tr = [self._tracer(r, 1, fill=False) for r in recs]
        for r in recs:
            if not r.same:
                self._tracer(r, 2, fill=False)
        o1 = [outs1[i] if outs1 is not None else ctx.empty((nz, nk)) for i in range(len(pairs))]
        o2 = [outs2[i] if outs2 is not None else ctx.empty((nz, nk)) for i in range(len(pairs))]
        if not spectra.batchable(recs, pairs):
            for i, (a, b) in enumerate(pairs):
                self._power_pair(a, b, out1=o1[i], out2=o2[i])
            return o1, o2
        n = len(uniq)
        ctx = self._main(needs_aux=True)
        tr = (nat.Tracer * len(recs))(*tr)
        pa = (C.c_int * n)(*[u[0] for u in uniq])
        pb = (C.c_int * n)(*[u[1] for u in uniq])
        p1 = (C.c_void_p * n)(*[o1[i].ptr for i in first])
        p2 = (C.c_void_p * n)(*[o2[i].ptr for i in first])
        d_wm, d_Pzk = self._d_wm(), self._d_Pzk()         # (uploads, if any, before the queue is issued)
        desc = nat.PowerBatchDesc(len(recs), tr, n, pa, pb, self._d_nzm.ptr, self._d_bh.ptr, self._d_ms().ptr,
                                  d_wm.ptr, self._d_ks().ptr, d_Pzk.ptr, self._rho_m0(),
                                  float(self.p["kstar_damping"]), p1, p2)
        # the coefficient rows of this batch ride in the tensor / profile group of the queued stages, if there is one
        prepared = self._flush(prep=desc) if self._stages else False
        ctx.call("hmg_power_batch_run", nz, nm, nk, C.byref(desc), nat.PB_PREPARED if prepared else 0)
        self._sync_point()
        for i, u in enumerate(alias):      # (a, b) and (b, a) are the same spectrum here: computed once, copied
            if first[u] != i:
                ctx.call("hmg_memcpy_d2d", o1[i].ptr, o1[first[u]].ptr, o1[i].nbytes)
                ctx.call("hmg_memcpy_d2d", o2[i].ptr, o2[first[u]].ptr, o2[i].nbytes)
        return o1, o2

    def spectra_block(self, pairs, nbuf=1):
        """A reusable result block for several (name, name2) spectra: one contiguous device buffer
        for the 2*len(pairs) (nz,nk) outputs and one page-locked host buffer of the same shape.
        ``compute()`` enqueues the batched mass integrals into it, ``fetch()`` brings all of them to
        the host with ONE asynchronous copy at link speed and returns numpy views (valid until the
        next ``fetch`` of the same block).  For parameter sweeps that read every spectrum back."""
        return SpectraBlock(self, pairs, nbuf)

    def get_power_all(self, pairs):
        """Extension of the reference API: {(name, name2): P_1h + P_2h} for several pairs in one
        pass over the profile tensors."""
        rpairs = self._resolve_pairs(pairs)
        self._tsz_notice(*dict.fromkeys(r for rp in rpairs for r in rp))
        o1, o2 = self._power_batch(rpairs)
        return {tuple(p): self._sum_on_device(a, b) for p, a, b in zip(pairs, o1, o2)}

    @staticmethod
    def _tsz_notice(*recs):
        """The reference prints this once per pressure tracer in every 2-halo evaluation
        (hmvec/hmvec.py:544)."""
        for r in recs:
            if r.kind2 == "p":
                print("Check the consistency relation for tSZ")

    _SMALL_GRID_BYTES = 32 << 20       # tensors up to this size: every registered tracer rides in the first batch

    def _power_cached(self, ra, rb):
        """The cache entry of a pair, computed if it is not there or older than the model's state."""
        ent = self._pcache.get((ra.name, rb.name))
        if ent is not None and ent.version == self._version:
            return ent
        nz, nm, nk = self._nz, self._nm, self._nk
        dicts = {"uk": self.uk_profiles, "pk": self.pk_profiles}
        # Batchable requests always go through the batched kernel, also when nothing rides along: a pair's
        # sums do not depend on what else is in the batch (foreign tensors enter with exact-zero coefficients),
        # so a spectrum has the same bits whatever was asked for before it.  The one-pair kernel (another
        # summation order, ~1e-16 away) is left with what the batch cannot do: bias overrides, the verbose
        # terms, names the 1-halo and 2-halo lookups resolve differently, two different HOD/pressure names.
        # On a small grid (a tensor below 32 MB: the README grid's are 32 MB for all three) every registered tracer rides.
        registered = (spectra.resolve(nm_, self.hods, self.uk_profiles, self.pk_profiles)
                      for nm_ in itertools.chain(self.hods, self.uk_profiles, self.pk_profiles))
        pairs = spectra.with_riders(ra, rb, registered, lambda tag, nm_: dicts[tag].on_device(nm_, (nz, nm, nk)),
                                    nz * nm * nk * 8 <= self._SMALL_GRID_BYTES)
        if pairs:
            # every spectrum of the batch in ONE device block: the host side then fetches the block in one copy the
            # first time any of them is asked for (_HostBlock) instead of one synchronising copy per spectrum
            n = len(pairs)
            blk = self._ctx().empty((2 * n, nz, nk))
            o1 = [blk.view(i * nz * nk, (nz, nk)) for i in range(n)]
            o2 = [blk.view((n + i) * nz * nk, (nz, nk)) for i in range(n)]
            # Issued once: what rides was validated above, so whatever this raises is a failure of the pass itself
            # (its queued stages are gone with it) - it reaches the caller and nothing is cached.
            self._power_batch(pairs, o1, o2)
            hb = _HostBlock(blk)
            for i, ((a, b), d1, d2) in enumerate(zip(pairs, o1, o2)):
                self._pcache[(a.name, b.name)] = self._pcache[(b.name, a.name)] = _Spectra(self._version, d1, d2, hb, i, n + i)
        else:
            self._pcache[(ra.name, rb.name)] = _Spectra(self._version, *self._power_pair(ra, rb))
        return self._pcache[(ra.name, rb.name)]

    def _power_host(self, ra, rb, term):
        """Host copy of P_1h (term 0) or P_2h (term 1) of a cached pair."""
        ent = self._power_cached(ra, rb)
        if ent.host is not None:
            return ent.host.take((ent.i1h, ent.i2h)[term])
        return (ent.p1h, ent.p2h)[term].numpy()

    def get_power(self, name, name2=None, verbose=False, b1=None, b2=None):
        """P_1h + P_2h in one pass (hmvec/hmvec.py:500-502)."""
        ra, rb = self._resolve(name, name if name2 is None else name2)
        self._tsz_notice(ra, rb)
        if b1 is None and b2 is None:
            ent = self._power_cached(ra, rb)
            d1, d2 = ent.p1h, ent.p2h
        else:
            d1, d2 = self._power_pair(ra, rb, b1, b2)
        if verbose:
            self._print_consistency(ra, rb)
        return self._sum_on_device(d1, d2)

    def _sum_on_device(self, d1, d2):
        """P_1h + P_2h added on the device: one array crosses PCIe (hmvec/hmvec.py:500-502)."""
        return self._sum_device(d1, d2).numpy()

    def _sum_device(self, d1, d2):
        ctx = self._ctx()
        out = ctx.empty(d1.shape)
        ctx.call("hmg_add", d1.size, d1.ptr, d2.ptr, out.ptr)
        return out

    def get_power_1halo(self, name="nfw", name2=None):
        """hmvec/hmvec.py:504-526."""
        return self._power_host(*self._resolve(name, name if name2 is None else name2), 0)

    def get_power_2halo(self, name="nfw", name2=None, verbose=False, b1_in=None, b2_in=None):
        """hmvec/hmvec.py:528-572."""
        ra, rb = self._resolve(name, name if name2 is None else name2)
        self._tsz_notice(ra, rb)
        if b1_in is None and b2_in is None:
            out = self._power_host(ra, rb, 1)
        else:
            out = self._power_pair(ra, rb, b1_in, b2_in, want=("2h",))[1].numpy()
        if verbose:
            self._print_consistency(ra, rb)
        return out

    def two_halo_terms(self, name, name2=None):
        """(I_1, C_1, I_2, C_2) of the 2-halo term (hmvec/hmvec.py:563-568): the mass integrals
        I(z,k) = int dm n b W(k), shape (nz,nk), and their k -> 0 consistency limits C(z), shape (nz,1)."""
        return self._two_halo_terms(*self._resolve(name, name if name2 is None else name2))

    def _two_halo_terms(self, ra, rb):
        ctx = self._main(needs_aux=True)
        nz, nm, nk = self._nz, self._nm, self._nk
        ta, tb = self._tracer(ra, 2), self._tracer(rb, 2)
        d_i1, d_i2, d_c = ctx.empty((nz, nk)), ctx.empty((nz, nk)), ctx.empty((nz, 2))
        ctx.call("hmg_power_2halo_terms", nz, nm, nk, C.byref(ta), C.byref(tb), self._d_nzm.ptr, self._d_bh.ptr,
                 self._d_ms().ptr, self._d_wm().ptr, self._d_ks().ptr, self._rho_m0(), d_i1.ptr, d_i2.ptr, d_c.ptr)
        c = d_c.numpy()
        return d_i1.numpy(), c[:, 0:1].copy(), d_i2.numpy(), c[:, 1:2].copy()

    def _print_consistency(self, ra, rb):
        """The two lines get_power_2halo(verbose=True) prints (hmvec/hmvec.py:569-571)."""
        i1, c1, i2, c2 = self._two_halo_terms(ra, rb)
        print("Two-halo consistency1: ", c1, i1)
        print("Two-halo consistency2: ", c2, i2)

    # ------------------------------------------------------- configuration-space statistics (DESIGN.md sections 13, 14)
    # xi(r), w_p(r_p), Sigma(R) and Delta Sigma(R) of the model's spectra: the rows stay on the device from the mass
    # integrals to the transform (realspace.py); only the (nz, nr) results cross to the host.
    _XI_TERMS = ("total", "1h", "2h")

    def _xi_request(self, rs, term, what="rs"):
        """The checked radii (or angles: `what`) of a transform request (everything that can be refused is, before any
        launch)."""
        if term not in self._XI_TERMS:
            raise ValueError(f"term must be one of {self._XI_TERMS}, got {term!r}")
        realspace.check_ks(self.ks)
        return realspace.check_rs(rs, what)

    def _xi_rows(self, d1, d2, term):
        """The device rows a term transforms; "total" is the device sum get_power brings to the host."""
        return d1 if term == "1h" else d2 if term == "2h" else self._sum_device(d1, d2)

    def _transform_rows(self, rows, nrows, rs, orders, zsum=None):
        """The transforms of nrows device rows at the radii rs as a tuple of (nrows, nr) host arrays: (xi,) for
        orders=None, else (W_n for n in orders), one launch either way.  With zsum = (chis, zw) rs are angles, the row
        at z is transformed at chis[z] rs and the rows of a block are summed with the (nw, nz) weights zw (section
        22): a tuple of (nrows / nz, nw, nr) arrays from one transform launch and one contraction."""
        if orders is None:
            return (realspace.transform_rows(self._ctx(), self._d_ks(), rows, nrows, self._nk, rs),)
        if zsum is not None:
            return angular.angular_rows(self._ctx(), self._d_ks(), rows, nrows // self._nz, self._nz, self._nk, rs,
                                        *zsum, orders)
        return realspace.hankel_rows(self._ctx(), self._d_ks(), rows, nrows, self._nk, rs, orders)

    def _realspace_pair(self, rs, name, name2, term, orders, zsum=None):
        """What get_xi, the projected and the angular statistics of one pair share: the request's checks, the tSZ
        notice, the pair's cached device spectra and one transform launch.  A tuple of (nz, nr) arrays, with zsum of
        (1, nw, nr) arrays (see _transform_rows)."""
        rs = self._xi_request(rs, term, "rs" if zsum is None else "thetas")
        ra, rb = self._resolve(name, name if name2 is None else name2)
        if term != "1h":          # (get_power and get_power_2halo print it, get_power_1halo does not)
            self._tsz_notice(ra, rb)
        if rs.size == 0:
            shape = (self._nz, 0) if zsum is None else (1, zsum[1].shape[0], 0)
            return tuple(np.empty(shape) for _ in (orders or (None,)))
        ent = self._power_cached(ra, rb)
        return self._transform_rows(self._xi_rows(ent.p1h, ent.p2h, term), self._nz, rs, orders, zsum)

    def _realspace_all(self, pairs, rs, term, orders, zsum=None):
        """The same for several pairs: their spectra from one pass over the profile tensors (get_power_all's) into one
        block and all of them through ONE transform launch of len(pairs) * nz rows.  (pairs, tuple of (n, nz, nr)
        arrays, with zsum of (n, nw, nr) arrays); every [i] is bit for bit what _realspace_pair gives for pairs[i]."""
        rs = self._xi_request(rs, term, "rs" if zsum is None else "thetas")
        pairs = [tuple(p) for p in pairs]
        rpairs = self._resolve_pairs(pairs)
        if term != "1h":
            self._tsz_notice(*dict.fromkeys(r for rp in rpairs for r in rp))
        n, nz, nk = len(pairs), self._nz, self._nk
        if rs.size == 0 or n == 0:
            shape = (n, nz, rs.size) if zsum is None else (n, zsum[1].shape[0], rs.size)
            return pairs, tuple(np.empty(shape) for _ in (orders or (None,)))
        ctx = self._ctx()
        blk = ctx.empty((2 * n, nz, nk))
        o1 = [blk.view(i * nz * nk, (nz, nk)) for i in range(n)]
        o2 = [blk.view((n + i) * nz * nk, (nz, nk)) for i in range(n)]
        if spectra.batchable(spectra.pair_plan(rpairs)[0], rpairs):
            self._power_batch(rpairs, o1, o2)
        else:
            # one pair the batch cannot express sends all of them to the one-pair kernel there (another summation
            # order): take each pair's spectra as the one-pair call does, so that the entries keep its bits
            for (ra, rb), d1, d2 in zip(rpairs, o1, o2):
                ent = self._power_cached(ra, rb)
                ctx.call("hmg_memcpy_d2d", d1.ptr, ent.p1h.ptr, d1.nbytes)
                ctx.call("hmg_memcpy_d2d", d2.ptr, ent.p2h.ptr, d2.nbytes)
        rows = self._xi_rows(blk.view(0, (n * nz, nk)), blk.view(n * nz * nk, (n * nz, nk)), term)
        outs = self._transform_rows(rows, n * nz, rs, orders, zsum)
        return pairs, tuple(o.reshape(n, -1, rs.size) for o in outs)

    def get_xi(self, rs, name="nfw", name2=None, term="total"):
        """Correlation function xi(z, r), shape (nz, nr), of the spectrum of (name, name2) - of P_1h + P_2h
        (term="total"), P_1h ("1h") or P_2h ("2h") - by the exact transform of realspace.xi_from_power: bit for bit
        xi_from_power(ks, get_power(name, name2), rs) and its get_power_1halo / get_power_2halo counterparts."""
        return self._realspace_pair(rs, name, name2, term, None)[0]

    def get_xi_all(self, pairs, rs, term="total"):
        """{(name, name2): xi(z, r)} for several pairs: their spectra from one pass over the profile tensors
        (get_power_all's) and all of them through ONE transform launch of len(pairs) * nz rows.  Each entry is bit for
        bit get_xi of that pair."""
        pairs, (xi,) = self._realspace_all(pairs, rs, term, None)
        return {p: xi[i] for i, p in enumerate(pairs)}

    def get_wp(self, rps, name, name2=None, term="total"):
        """Projected correlation function w_p(z, r_p), shape (nz, nr), of the spectrum of (name, name2) - term as for
        get_xi - integrated along the whole line of sight (pi_max -> infinity): W_0 of
        realspace.projected_from_power, bit for bit projected_from_power(ks, get_power(name, name2), rps).  r_p is
        comoving, in the inverse units of ks; w_p has the units of P times those of ks squared (a length for a
        three-dimensional spectrum)."""
        return self._realspace_pair(rps, name, name2, term, (0,))[0]

    def get_surface_density(self, Rs, name, name2=None, term="total"):
        """Surface density Sigma(z, R) = rho_m0 W_0(R), shape (nz, nr), of the spectrum of (name, name2), e.g. P_gm -
        term as for get_xi; W_0 of realspace.projected_from_power.  Comoving units: rho_m0 = rho_matter_z(0) is the
        comoving matter density, R a comoving transverse distance in the inverse units of ks, Sigma a mass per comoving
        area with the mean density's contribution left out (the line-of-sight integral of rho_m0 xi).  The physical
        convention of sigma_2h_profiles (physical radius R_phys = R / (1 + z), mass per
        physical area, at the angle theta = R_phys / d_A(z) = R / chi(z)) is
        Sigma_phys(R_phys) = (1 + z)^2 Sigma(R_phys (1 + z))."""
        w0 = self._realspace_pair(Rs, name, name2, term, (0,))[0]          # (the request is checked first)
        return self._rho_m0() * w0

    def get_excess_surface_density(self, Rs, name, name2=None, term="total"):
        """Excess surface density Delta Sigma(z, R) = mean Sigma(< R) - Sigma(R) = rho_m0 W_2(R), shape (nz, nr), of
        the spectrum of (name, name2); units and the conversion to the physical convention of
        delta_sigma_2h_profiles as for get_surface_density: Delta Sigma_phys(R_phys) = (1 + z)^2 Delta Sigma(R_phys (1 + z))."""
        w2 = self._realspace_pair(Rs, name, name2, term, (2,))[0]
        return self._rho_m0() * w2

    def get_wp_all(self, pairs, rps, term="total"):
        """{(name, name2): w_p(z, r_p)} for several pairs, spectra and launches as for get_xi_all.  Each entry is bit
        for bit get_wp of that pair."""
        pairs, (wp,) = self._realspace_all(pairs, rps, term, (0,))
        return {p: wp[i] for i, p in enumerate(pairs)}

    def get_surface_density_all(self, pairs, Rs, term="total"):
        """{(name, name2): (Sigma(z, R), Delta Sigma(z, R))} for several pairs, spectra as for get_xi_all and both
        statistics from ONE transform launch.  Each entry is bit for bit get_surface_density and
        get_excess_surface_density of that pair."""
        pairs, (w0, w2) = self._realspace_all(pairs, Rs, term, (0, 2))
        rho = self._rho_m0()
        return {p: (rho * w0[i], rho * w2[i]) for i, p in enumerate(pairs)}

    # ------------------------------------------------------------------ angular correlation functions
    # w(theta), gamma_t(theta), xi+-(theta): the rows at the model's redshifts are transformed at chi(z) theta and summed
    # over z with the windows' weights on the device (angular.py); only the (nw, ntheta) results cross to the host.
    def _angular_request(self, zweights, order, term):
        """(zsum, orders, stacked) of an angular request: the distances of self.zs, the checked (nw, nz) weights
        (None: the z measure alone, both windows 1) and orders, and whether the weights came with the nw axis."""
        if term not in self._XI_TERMS:
            raise ValueError(f"term must be one of {self._XI_TERMS}, got {term!r}")
        orders = angular.check_order(order)
        nz = np.size(self.zs)
        if zweights is None:
            zweights = self.angular_weights(self.zs, 1.0, 1.0)
        zw, stacked = angular.check_zweights(zweights, nz)
        chis = angular.check_chis(np.reshape(self.comoving_radial_distance(self.zs), -1), nz)
        return (chis, zw), orders, stacked

    def get_angular(self, thetas, name, name2=None, zweights=None, order=0, term="total"):
        """Angular correlation function zeta_order(theta) = sum_z zweights[z] W_order^(z)(chi(z) theta) of the spectrum
        of (name, name2) - term as for get_xi - on the model's redshifts self.zs, chi = comoving_radial_distance(zs)
        (every z must be positive): bit for bit angular.angular_from_power(ks, get_power(name, name2), thetas, chi,
        zweights, order).  thetas in radians.  zweights: (nz,) or (nw, nz), the z measure times the two windows
        (angular_weights(zs, W1, W2)); None is the measure alone.  order: 0, 2, 4 or a strictly increasing tuple of
        them.  Returns (ntheta,), or (nw, ntheta) for two-dimensional weights; a tuple of them for a tuple of
        orders."""
        zsum, orders, stacked = self._angular_request(zweights, order, term)
        outs = self._realspace_pair(thetas, name, name2, term, orders, zsum)
        outs = tuple(o[0] if stacked else o[0, 0] for o in outs)
        return outs if isinstance(order, (tuple, list)) else outs[0]

    def _dndz_window(self, dndz, what):
        """dndz / int dndz dz on self.zs (C_gg's convention); None is a uniform distribution over the range of zs."""
        zs = np.reshape(self.zs, -1)
        if zs.size < 2:
            raise ValueError(f"{what} needs at least two redshifts in the model")
        dndz = np.ones(zs.size) if dndz is None else np.asarray(dndz, dtype=np.float64)
        if dndz.shape != zs.shape or not np.all(np.isfinite(dndz)):
            raise ValueError(f"{what} must be a finite vector of {zs.size} values on the model's redshifts")
        norm = _trapz(dndz, zs)
        if not norm > 0:
            raise ValueError(f"{what} must have a positive integral over the model's redshifts")
        return dndz / norm

    def _source_window(self, zsource, sdndz, what):
        """lensing_window on self.zs of a source plane (zsource a scalar) or of sources sdndz on the grid zsource."""
        if zsource is None:
            raise ValueError(f"{what} is required: a source redshift, or the grid of a source distribution")
        zsource = np.asarray(zsource, dtype=np.float64).reshape(-1)
        if (zsource.size == 1) != (sdndz is None) or (sdndz is not None and np.shape(sdndz) != zsource.shape):
            raise ValueError(f"{what}: one source redshift without a distribution, or a grid with its distribution")
        return self.lensing_window(np.reshape(self.zs, -1), zsource, sdndz)

    def get_w_theta(self, thetas, name, name2=None, dndz=None, dndz2=None, term="total"):
        """Angular clustering w(theta), shape (ntheta,): order 0 with the windows dndz / int dndz dz of the two samples
        on self.zs (C_gg's convention; dndz None: uniform over the range of zs, dndz2 None: the first sample's) -
        bit for bit get_angular(thetas, name, name2, angular_weights(zs, W1, W2), 0, term)."""
        if term not in self._XI_TERMS:
            raise ValueError(f"term must be one of {self._XI_TERMS}, got {term!r}")
        W1 = self._dndz_window(dndz, "dndz")
        W2 = W1 if dndz2 is None else self._dndz_window(dndz2, "dndz2")
        return self.get_angular(thetas, name, name2, self.angular_weights(self.zs, W1, W2), 0, term)

    def get_gamma_t(self, thetas, name, name2="nfw", dndz=None, zsource=None, sdndz=None, term="total"):
        """Tangential shear gamma_t(theta), shape (ntheta,), of the lenses `name` (window dndz / int dndz dz as for
        get_w_theta) about sources at zsource (a single redshift, or a grid with the distribution sdndz: the arguments
        of lensing_window): order 2 of the lens-matter spectrum - bit for bit
        get_angular(thetas, name, name2, angular_weights(zs, W_lens, lensing_window(zs, zsource, sdndz)), 2, term)."""
        if term not in self._XI_TERMS:
            raise ValueError(f"term must be one of {self._XI_TERMS}, got {term!r}")
        W1 = self._dndz_window(dndz, "dndz")
        W2 = self._source_window(zsource, sdndz, "zsource")
        return self.get_angular(thetas, name, name2, self.angular_weights(self.zs, W1, W2), 2, term)

    def get_xi_pm(self, thetas, name="nfw", name2=None, zsource=None, sdndz=None, zsource2=None, sdndz2=None,
                  term="total"):
        """Shear correlation functions (xi+(theta), xi-(theta)), each (ntheta,), of sources at zsource (and zsource2,
        default the same; arguments as for get_gamma_t): orders 0 and 4 of the matter spectrum from ONE launch - bit
        for bit get_angular(thetas, name, name2, angular_weights(zs, W_kappa1, W_kappa2), (0, 4), term)."""
        if term not in self._XI_TERMS:
            raise ValueError(f"term must be one of {self._XI_TERMS}, got {term!r}")
        W1 = self._source_window(zsource, sdndz, "zsource")
        W2 = W1 if zsource2 is None else self._source_window(zsource2, sdndz2, "zsource2")
        return self.get_angular(thetas, name, name2, self.angular_weights(self.zs, W1, W2), (0, 4), term)

    def get_angular_all(self, pairs, thetas, zweights, order=0, term="total"):
        """{(name, name2): zeta_order(theta)} for several pairs: their spectra from one pass over the profile tensors
        (get_power_all's), ONE transform launch of len(pairs) * nz rows and one contraction over z.  zweights: (nz,)
        or (nw, nz) shared by all pairs, or a dict {pair: weights}.  Each entry is bit for bit get_angular of that
        pair with its weights."""
        pairs = [tuple(p) for p in pairs]
        if isinstance(zweights, dict):
            missing = [p for p in pairs if p not in zweights]
            if missing:
                raise ValueError(f"zweights has no entry for {missing}")
            per = [angular.check_zweights(zweights[p], np.size(self.zs)) for p in pairs]
        else:
            per = [angular.check_zweights(zweights, np.size(self.zs))] * len(pairs)
        # every pair's rows of weights go stacked into the one contraction and the pair keeps its own: an output's
        # chain reads its row of weights alone, so its bits are those of the pair's own call
        shared = not isinstance(zweights, dict)
        stack = None if not per else per[0][0] if shared else np.concatenate([zw for zw, _ in per])
        zsum, orders, _ = self._angular_request(stack, order, term)
        pairs, outs = self._realspace_all(pairs, thetas, term, orders, zsum)
        res, lo = {}, 0
        for i, (p, (zw, stacked)) in enumerate(zip(pairs, per)):
            ent = tuple(o[i, lo:lo + zw.shape[0]] if stacked else o[i, lo] for o in outs)
            res[p] = ent if isinstance(order, (tuple, list)) else ent[0]
            lo += 0 if shared else zw.shape[0]
        return res

    # ------------------------------------------------------------------ 1-halo trispectrum
    # T[z,i,j] = sum_m wm nzm s_ab[z,m,i] s_cd[z,m,j]: the mass integral of get_power_1halo with one more free index,
    # contracted on the device over the resident tensors (hmg_trispectrum_1h); only (nz, n, n) or (n, n) results cross.
    TRISPECTRUM_MAX_SAMPLES = 1024

    def _sample_tables(self, kindex, idx, frac, scale, damping, max_samples, what):
        """The checked (nz, n) sample tables of a request of `what` ("the trispectrum", ...), which takes at most
        max_samples per redshift: int32 idx, frac, scale (damping=True: folded in).  Everything that can be refused is,
        here, before any launch."""
        nz, nk = self._nz, self._nk
        if idx is None:
            if frac is not None:
                raise ValueError("frac needs idx")
            kindex = np.arange(nk) if kindex is None else np.asarray(kindex)
            if kindex.ndim != 1 or not np.issubdtype(kindex.dtype, np.integer):
                raise ValueError("kindex must be a one-dimensional integer array of indices into ks")
            idx = np.broadcast_to(kindex[None, :], (nz, kindex.size))
        else:
            if kindex is not None:
                raise ValueError("give kindex or the idx / frac tables, not both")
            idx = np.asarray(idx)
            if not np.issubdtype(idx.dtype, np.integer):
                raise ValueError("idx must be an integer array")
            if idx.ndim == 1:
                idx = np.broadcast_to(idx[None, :], (nz, idx.size))
            if idx.ndim != 2 or idx.shape[0] != nz:
                raise ValueError(f"idx must have shape (n,) or (nz, n) with nz = {nz}, got {idx.shape}")
        n = idx.shape[1]
        if n < 1:
            raise ValueError(f"kindex / idx is empty: {what} needs at least one sample")
        if n > max_samples:
            raise ValueError(f"kindex / idx asks for {n} samples per redshift; {what} takes at most {max_samples}: pass "
                             f"a shorter kindex")
        if idx.min() < 0 or idx.max() > nk - 1:
            raise ValueError(f"kindex / idx must lie in 0 .. nk - 1 = {nk - 1}, got {idx.min()} .. {idx.max()}")
        frac = np.zeros((nz, n)) if frac is None else np.broadcast_to(np.asarray(frac, dtype=np.float64), (nz, n))
        if not np.all((frac >= 0.0) & (frac <= 1.0)):
            raise ValueError("frac must lie in [0, 1]")
        if np.any((idx == nk - 1) & (frac != 0.0)):
            raise ValueError("idx = nk - 1 needs frac = 0 (there is no node to its right)")
        scale = np.ones((nz, n)) if scale is None else np.broadcast_to(np.asarray(scale, dtype=np.float64), (nz, n))
        if not np.all(np.isfinite(scale)):
            raise ValueError("scale must be finite")
        if damping:
            ks = self.ks
            k = np.where(frac == 0.0, ks[idx], (1.0 - frac) * ks[idx] + frac * ks[np.minimum(idx + 1, nk - 1)])
            scale = scale * (1.0 - np.exp(-(k / self.p["kstar_damping"]) ** 2.0))
        return (np.ascontiguousarray(idx, dtype=np.int32), np.ascontiguousarray(frac, dtype=np.float64),
                np.ascontiguousarray(scale, dtype=np.float64))

    def _trispectrum_tables(self, kindex, idx, frac, scale, damping):
        """_sample_tables of a trispectrum request (the result has nz * n * n entries: at most 1024 samples)."""
        return self._sample_tables(kindex, idx, frac, scale, damping, self.TRISPECTRUM_MAX_SAMPLES, "the trispectrum")

    # what the requests of sections 15, 16, 17 and 19 share
    def _zweights(self, zweights):
        zweights = np.ascontiguousarray(zweights, dtype=np.float64).reshape(-1)
        if zweights.size != self._nz:
            raise ValueError(f"zweights must have one entry per redshift ({self._nz}), got {zweights.size}")
        return zweights

    @staticmethod
    def _upload_tables(ctx, tables):
        """(d_idx, d_frac, d_scale).  They may go back to the free list as soon as the call that reads them is enqueued:
        whatever reuses them is enqueued behind it."""
        return ctx.upload_int32(tables[0]), ctx.upload(tables[1]), ctx.upload(tables[2])

    _MODEL_BLOCK = {"d_nzm": lambda h: h._d_nzm.ptr, "d_bh": lambda h: h._d_bh.ptr, "d_ms": lambda h: h._d_ms().ptr,
                    "d_wm": lambda h: h._d_wm().ptr, "d_ks": lambda h: h._d_ks().ptr, "d_Pzk": lambda h: h._d_Pzk().ptr,
                    "rho_m0": lambda h: h._rho_m0()}

    def _model_block(self, entry):
        """The model block of a native call, by the header's parameter names: those of d_nzm, d_bh, d_ms, d_wm, d_ks,
        d_Pzk, rho_m0 that `entry` declares, in its order."""
        return {n: self._MODEL_BLOCK[n](self) for n in nat.PARAMS[entry] if n in self._MODEL_BLOCK}

    def trispectrum_device(self, name, name2=None, name3=None, name4=None, kindex=None, damping=True, idx=None,
                           frac=None, scale=None, zweights=None, per_z=True):
        """(T, Tz) on the device: T (nz, n, n) the 1-halo trispectrum of the spectra (name, name2) and (name3, name4) -
        per_z=False: None - and Tz (n, n) = sum_z zweights[z] T[z], in z order, if zweights (nz,) is given, else None.

        Samples: kindex (nodes of ks, the same for every z; default all of them), or tables idx / frac (n,) or (nz, n) -
        sample i of redshift z is the square term interpolated linearly between the nodes idx and idx + 1 at the
        fraction frac (default 0; idx = nk - 1 needs frac = 0), times scale (default 1).  damping=True multiplies scale
        by 1 - exp(-(k / kstar)^2) at the sample's wavenumber, as get_power_1halo damps P_1h.  At most 1024 samples.
        name3 / name4 default to the first pair; the square terms are get_power_1halo's, first-name-only rules
        included."""
        name2 = name if name2 is None else name2
        name3, name4 = (name if name3 is None else name3), (name2 if name4 is None else name4)
        recs = self._resolve(name, name2, name3, name4)
        tables = self._trispectrum_tables(kindex, idx, frac, scale, damping)
        if zweights is not None:
            zweights = self._zweights(zweights)
        elif not per_z:
            raise ValueError("nothing asked for: per_z=False needs zweights")
        nz, nm, nk, n = self._nz, self._nm, self._nk, tables[0].shape[1]
        ctx = self._main(needs_aux=True)
        # (another reader of the tensors than the batched mass integrals: a deferred left fill is written first)
        tr = [self._tracer(r, 1) for r in recs]
        d_idx, d_frac, d_scale = self._upload_tables(ctx, tables)
        d_g = ctx.upload(zweights) if zweights is not None else None
        T = ctx.empty((nz, n, n)) if per_z else None
        Tz = ctx.empty((n, n)) if zweights is not None else None
        ha, hb, hc, hd = (C.byref(t) for t in tr)
        ctx.call("hmg_trispectrum_1h", nz=nz, nm=nm, nk=nk, n=n, h_a=ha, h_b=hb, h_c=hc, h_d=hd,
                 **self._model_block("hmg_trispectrum_1h"), d_idx=d_idx.ptr, d_frac=d_frac.ptr, d_scale=d_scale.ptr,
                 d_zweights=nat.ptr(d_g), d_T=nat.ptr(T), d_Tz=nat.ptr(Tz))
        self._sync_point()
        return T, Tz

    def get_trispectrum_1halo(self, name, name2=None, name3=None, name4=None, kindex=None, damping=True):
        """1-halo trispectrum T(z; k_i, k_j) = int dm n(z,m) S_ab(z,m,k_i) S_cd(z,m,k_j), shape (nz, n, n), of the spectra
        (name, name2) and (name3, name4; default: the first pair) at the nodes ks[kindex] (default: all; at most 1024).
        S is the square term get_power_1halo integrates, so without damping T[z,i,i] of a pair with itself is the mass
        integral of its square.  damping=True (default) multiplies by D(k_i) D(k_j), D = 1 - exp(-(k/kstar)^2), which
        makes T consistent with the damped P_1h the model returns; damping=False leaves it out."""
        return self.trispectrum_device(name, name2, name3, name4, kindex=kindex, damping=damping)[0].numpy()

    # ------------------------------------------------------------------ bispectrum of three tracers
    # B1h, B2h, B3h at triangles of sample wavenumbers, contracted on the device over the resident tensors
    # (hmg_bispectrum); only (3, nz, nt) or (3, nt) results cross.  The host side of the contract is bispectrum.py.
    def bispectrum_device(self, name, name2=None, name3=None, triangles=None, kindex=None, damping=True, idx=None,
                          frac=None, scale=None, zweights=None, per_z=True):
        """(B, Bz) on the device: B (3, nz, nt) the 1-halo, 2-halo and 3-halo terms of the bispectrum of the tracers
        (name, name2, name3) - per_z=False: None - and Bz (3, nt) = sum_z zweights[z] B[:, z], in z order, if zweights
        (nz,) is given, else None.  Missing names default to the first.

        Samples as for trispectrum_device (kindex, or idx / frac / scale tables; at most 256), except that damping is
        not folded into scale: the factors D = 1 - exp(-(k / kstar)^2) multiply the 1-halo term and the 1-halo factor of
        each 2-halo term.  triangles: (nt, 3) integer array of sample indices, the same for every redshift - leg
        `name` sits at column 0, name2 at 1, name3 at 2; default: all i <= j <= l that close at every redshift; at most
        2^20.  A triangle must close at every redshift.  At most one of the names may be an HOD."""
        return self._bispectrum(name, name2, name3, triangles, kindex, damping, idx, frac, scale, zweights, per_z)[:2]

    def _bispectrum(self, name, name2, name3, triangles, kindex, damping, idx, frac, scale, zweights, per_z, want_J=False):
        """(B, Bz, J) of bispectrum_device; J (3, nz, n), the 2-halo bracket (I + b) - C of each leg at the samples, if
        want_J, else None.  Every refusal happens here on the host, before any launch."""
        name2 = name if name2 is None else name2
        name3 = name if name3 is None else name3
        triple = (name, name2, name3)
        recs = self._resolve(*triple)
        if sum(r.kind1 == "h" for r in recs) >= 2:
            raise NotImplementedError(
                f"bispectrum of {triple!r}: two or more HOD names in one triple need the third factorial moments of the "
                f"HOD for the 1-halo term, which the model does not carry (the product of two galaxy weights would "
                f"count self-pairs)")
        _same_lookups(recs, f"bispectrum of {triple!r}")
        tables = self._sample_tables(kindex, idx, frac, scale, False, bispec.MAX_SAMPLES, "the bispectrum")
        n = tables[0].shape[1]
        tri = bispec.check_triangles(triangles, bispec.sample_wavenumbers(self.ks, tables[0], tables[1]), self.zs)
        if zweights is not None:
            zweights = self._zweights(zweights)
        elif not per_z and not want_J:
            raise ValueError("nothing asked for: per_z=False needs zweights")
        nz, nm, nk, nt = self._nz, self._nm, self._nk, tri.shape[0]
        ctx = self._main(needs_aux=True)
        # (another reader of the tensors than the batched mass integrals: a deferred left fill is written first)
        tr = [self._tracer(r, 1) for r in recs]
        d_idx, d_frac, d_scale = self._upload_tables(ctx, tables)
        d_tri = ctx.upload_int32(tri)
        d_g = ctx.upload(zweights) if zweights is not None else None
        B = ctx.empty((3, nz, nt)) if per_z else None
        Bz = ctx.empty((3, nt)) if zweights is not None else None
        J = ctx.empty((3, nz, n)) if want_J else None
        ha, hb, hc = (C.byref(t) for t in tr)
        ctx.call("hmg_bispectrum", nz=nz, nm=nm, nk=nk, n=n, nt=nt, h_a=ha, h_b=hb, h_c=hc,
                 **self._model_block("hmg_bispectrum"), kstar=float(self.p["kstar_damping"]) if damping else 0.0,
                 d_idx=d_idx.ptr, d_frac=d_frac.ptr, d_scale=d_scale.ptr, d_tri=d_tri.ptr, d_zweights=nat.ptr(d_g),
                 d_B=nat.ptr(B), d_Bz=nat.ptr(Bz), d_J=nat.ptr(J))
        self._sync_point()
        return B, Bz, J

    def get_bispectrum(self, name, name2=None, name3=None, triangles=None, kindex=None, term="total", damping=True):
        """The halo-model bispectrum B(z; k_1, k_2, k_3) of three tracers (missing names: the first), shape (nz, nt), at
        triangles of the nodes ks[kindex] (default: all nodes; at most 256) - triangles (nt, 3) indexes kindex, leg
        `name` at column 0; default: all i <= j <= l that close.  term: "1h", "2h", "3h" or "total" (their sum in that
        order).  Linear halo bias only (no b_2 term); the 3-halo term uses the tree-level matter bispectrum of the
        model's P_lin.  damping as in get_power_1halo, per leg."""
        if term not in bispec.TERMS:
            raise ValueError(f"term must be one of {bispec.TERMS}, got {term!r}")
        B = self.bispectrum_device(name, name2, name3, triangles=triangles, kindex=kindex, damping=damping)[0]
        return bispec.pick_term(B.numpy(), term)

    # ------------------------------------------------------------------ response and super-sample covariance (section 17)
    # R_ab = dP_ab / d delta_b at sample wavenumbers for several pairs at once (hmg_response) and the rank-nz contraction
    # Cov = sum_z g r r of such responses (hmg_ssc); only (np, nz, n) and (np n)^2 results cross.  The host side of the
    # contract - sigma_b, the Limber tables, the slope table - is cov.py.
    RESPONSE_MAX_PAIRS = 16

    def _response_request(self, pairs, kindex, idx, frac, scale):
        """(pairs as names, records, tables) of a response request.  Every refusal happens here on the host, before any
        launch."""
        pairs = [(a, a if b is None else b) for a, b in ([p, None] if isinstance(p, str) else p for p in pairs)]
        if len(pairs) < 1:
            raise ValueError("pairs is empty: the response needs at least one (name, name2)")
        if len(pairs) > self.RESPONSE_MAX_PAIRS:
            raise ValueError(f"{len(pairs)} pairs; at most {self.RESPONSE_MAX_PAIRS} are taken in one call")
        recs = self._resolve(*[nm_ for p in pairs for nm_ in p])
        _same_lookups(recs, f"response of {pairs!r}")
        return pairs, recs, self._sample_tables(kindex, idx, frac, scale, False, bispec.MAX_SAMPLES, "the response")

    def _response_launch(self, recs, tables, damping, parts):
        nz, nm, nk, n, npairs = self._nz, self._nm, self._nk, tables[0].shape[1], len(recs) // 2
        ctx = self._main(needs_aux=True)
        # (another reader of the tensors than the batched mass integrals: a deferred left fill is written first)
        tr = (nat.Tracer * len(recs))(*[self._tracer(r, 1) for r in recs])
        d_idx, d_frac, d_scale = self._upload_tables(ctx, tables)
        d_dlnP = self._dev("dlnP", lambda: covmod.dlnp_table(self.ks, self.Pzk))
        R = ctx.empty((npairs, nz, n))
        P = ctx.empty((3, npairs, nz, n)) if parts else None
        ctx.call("hmg_response", nz=nz, nm=nm, nk=nk, n=n, np=npairs, h_pairs=tr, **self._model_block("hmg_response"),
                 d_dlnP=d_dlnP.ptr, kstar=float(self.p["kstar_damping"]) if damping else 0.0, d_idx=d_idx.ptr,
                 d_frac=d_frac.ptr, d_scale=d_scale.ptr, d_R=R.ptr, d_parts=nat.ptr(P))
        self._sync_point()
        return R, P

    def response_device(self, pairs, kindex=None, damping=True, idx=None, frac=None, scale=None, parts=False):
        """R on the device, (np, nz, n): the response dP_ab / d delta_b of the halo-model spectrum of each pair (a, b) of
        `pairs` (1 to 16; a lone name or (a, None) is (a, a)) to a long-wavelength density mode,

            R = scale [ (47/21 - n_s/3) P2h + D I1 - (beta_a + beta_b) (P2h + D A1) ],

        A1 the undamped 1-halo integral of get_power_1halo (first-name-only rules included), I1 the same integral weighted
        with the halo bias, P2h = P_lin J_a J_b the 2-halo term of get_power_2halo, n_s the logarithmic slope of P_lin,
        D the damping factor of get_power_1halo (damping=False: 1) and beta the mean galaxy bias of an HOD name (0 of a
        matter or pressure name: a galaxy overdensity is defined against the local mean density).  The growth and
        dilation factor takes the slope of P_lin only, not of the 2-halo brackets - the usual halo-model approximation.
        Samples as for bispectrum_device (kindex, or idx / frac / scale tables; at most 256).  parts=True: (R, parts),
        parts (3, np, nz, n) = (A1, I1, P2h), unscaled and undamped.  Two HOD names in one pair are allowed."""
        _, recs, tables = self._response_request(pairs, kindex, idx, frac, scale)
        R, P = self._response_launch(recs, tables, damping, parts)
        return (R, P) if parts else R

    def get_power_response(self, name, name2=None, kindex=None, damping=True):
        """dP_ab(z, k) / d delta_b of the pair (name, name2; default name) at the nodes ks[kindex] (default: all, at most
        256), shape (nz, n); see response_device."""
        return self.response_device([(name, name2)], kindex=kindex, damping=damping).numpy()[0]

    def ssc_device(self, pairs, zweights, zscale=None, kindex=None, damping=True, idx=None, frac=None, scale=None):
        """Cov on the device, (np, n, np, n): Cov[p,i,q,j] = sum_z zweights[z] r[p,z,i] r[q,z,j], in z order, of the
        responses r[p,z,s] = zscale[p][z] R_p[z,s] (response_device's; zscale (np, nz), default 1).  Each term is formed
        as fma(r r, g, acc) with the weight on neither side: Cov[p,i,q,j] has the bits of Cov[q,j,p,i]."""
        pairs, recs, tables = self._response_request(pairs, kindex, idx, frac, scale)
        nz, n, npairs = self._nz, tables[0].shape[1], len(pairs)
        zweights = np.ascontiguousarray(zweights, dtype=np.float64)
        if zweights.shape != (nz,):
            raise ValueError(f"zweights must have one entry per redshift ({nz}), got shape {zweights.shape}")
        if zscale is not None:
            zscale = np.ascontiguousarray(zscale, dtype=np.float64)
            if zscale.shape != (npairs, nz):
                raise ValueError(f"zscale must have shape (np, nz) = {(npairs, nz)}, got {zscale.shape}")
        R, _ = self._response_launch(recs, tables, damping, False)
        return self._ssc_launch(R, zweights, zscale)

    def _ssc_launch(self, R, zweights, zscale):
        npairs, nz, n = R.shape
        ctx = self._main()
        d_g = ctx.upload(zweights)
        d_zs = ctx.upload(zscale) if zscale is not None else None
        cov_ = ctx.empty((npairs, n, npairs, n))
        ctx.call("hmg_ssc", nz, n, npairs, R.ptr, nat.ptr(d_zs), d_g.ptr, cov_.ptr)
        self._sync_point()
        return cov_

    # ------------------------------------------------------------------ redshift-space spectra
    # Wedges P^s(k, mu) and multipoles P_0, P_2, P_4 of one pair at nodes of the k grid (hmg_rsd_wedges,
    # hmg_rsd_multipoles): a mass integral with a Gaussian of the bin's line-of-sight dispersion inside it.  The host side
    # of the contract - the default dispersion, the rule in mu, the checks - is rsd.py.
    def _rsd_request(self, name, name2, kindex, sigma_s, f, alphas, damping):
        """(records, uploaded tables, alphas) of a redshift-space request.  Every refusal happens here on the host,
        before any launch."""
        pair = (name, name if name2 is None else name2)
        recs = self._resolve(*pair)
        for r in recs:
            if r.kind1 == "p" or r.kind2 == "p":
                raise ValueError(f"redshift-space spectrum of {pair!r}: {r.name!r} is a pressure profile, which has no "
                                 f"line-of-sight velocity in this model")
        _same_lookups(recs, f"redshift-space spectrum of {pair!r}")
        nz, nm, nk = self._nz, self._nm, self._nk
        kindex = rsdmod.check_kindex(kindex, nk)
        sigma_s = rsdmod.check_sigma(rsdmod.virial_dispersion(self) if sigma_s is None else sigma_s, nz, nm)
        f = rsdmod.check_f(self.get_growth_rate_f(self.zs) if f is None else f, nz)
        alphas = rsdmod.check_alphas(alphas)
        damp = bispec.damping(self.ks[kindex], self.p["kstar_damping"]) if damping else np.ones(kindex.size)
        return recs, (kindex, np.ascontiguousarray(damp, dtype=np.float64), sigma_s, f), alphas

    def _rsd_launch(self, entry, recs, tables, alphas, mus, wl, out_last, parts_shape):
        nz, nm, nk, n, nmu = self._nz, self._nm, self._nk, tables[0].size, mus.size
        ctx = self._main(needs_aux=True)
        # (another reader of the tensors than the batched mass integrals: a deferred left fill is written first)
        ta, tb = (self._tracer(r, 1) for r in recs)
        d_k, d_damp, d_sig, d_f = ctx.upload_int32(tables[0]), ctx.upload(tables[1]), ctx.upload(tables[2]), ctx.upload(tables[3])
        d_mus = ctx.upload(mus)
        d_wl = None if wl is None else ctx.upload(np.ascontiguousarray(wl, dtype=np.float64))
        out = ctx.empty((2, nz, n, out_last))
        parts = ctx.empty(parts_shape(nz, n)) if parts_shape else None
        own = dict(d_parts=nat.ptr(parts)) if wl is None else dict(d_wl=d_wl.ptr, d_Q=nat.ptr(parts))
        ctx.call(entry, nz=nz, nm=nm, nk=nk, n=n, nmu=nmu, h_a=C.byref(ta), h_b=C.byref(tb), **self._model_block(entry),
                 d_kindex=d_k.ptr, d_damp=d_damp.ptr, d_mus=d_mus.ptr, d_sigma=d_sig.ptr, d_f=d_f.ptr, alpha_m=alphas[0],
                 alpha_c=alphas[1], alpha_s=alphas[2], d_out=out.ptr, **own)
        self._sync_point()
        return out, parts      # (the tables go back to the free list: whatever reads them was enqueued before)

    def rsd_device(self, name, name2=None, mus=None, kindex=None, sigma_s=None, f=None, alphas=(1, 0, 1), damping=True,
                   parts=False):
        """The redshift-space wedges of the pair (name, name2; default name) on the device, (2, nz, n, nmu) = (P1h, P2h),
        at the nodes ks[kindex] (default: all) and the values mus of mu in [0, 1] (default: rsd.mu_rule(16)'s nodes; at
        most 32).  Dispersion halo model: a halo's members of species i are displaced along the line of sight with the
        Gaussian dispersion alphas[i] sigma_s[z, m] - alphas = (alpha_m, alpha_c, alpha_s) for matter, centrals and
        satellites; sigma_s (nz, nm) in comoving Mpc, default rsd.virial_dispersion(self) - so every product of two species
        in a mass integral carries exp(-(alpha_i^2 + alpha_j^2) (k sigma_s mu)^2 / 2), and the 2-halo term is

            P2h = P_lin (J_a + f mu^2 K_a) (J_b + f mu^2 K_b),

        J the bracket of get_power_2halo with the damped weights, K the same bracket without the halo bias (the Kaiser
        term of the tracer's own velocity) and f (nz,) the growth rate, default get_growth_rate_f(zs).  The square term
        of P1h is get_power_1halo's, first-name-only rule for two HOD names included; damping=True multiplies P1h by
        1 - exp(-(k / kstar)^2) as get_power_1halo does.  A matter or an HOD name is taken, a pressure name refused.
        parts=True: (out, parts), parts (4, nz, n, nmu) = (I_a, V_a, I_b, V_b), the damped mass sums of the brackets."""
        mus = rsdmod.mu_rule(rsdmod.DEFAULT_NMU)[0] if mus is None else mus
        mus = rsdmod.check_mus(mus)
        recs, tables, alphas = self._rsd_request(name, name2, kindex, sigma_s, f, alphas, damping)
        out, P = self._rsd_launch("hmg_rsd_wedges", recs, tables, alphas, mus, None, mus.size,
                                  (lambda nz, n: (4, nz, n, mus.size)) if parts else None)
        return (out, P) if parts else out

    def get_power_rsd(self, name, name2=None, mus=None, kindex=None, sigma_s=None, f=None, alphas=(1, 0, 1), damping=True):
        """{"1h", "2h", "total"}: the redshift-space wedges P^s(z, k, mu) of the pair on the host, each (nz, n, nmu); see
        rsd_device."""
        out = self.rsd_device(name, name2, mus=mus, kindex=kindex, sigma_s=sigma_s, f=f, alphas=alphas,
                              damping=damping).numpy()
        return {"1h": out[0], "2h": out[1], "total": out[0] + out[1]}

    def multipoles_device(self, name, name2=None, nmu=16, kindex=None, sigma_s=None, f=None, alphas=(1, 0, 1), damping=True,
                          parts=False):
        """The multipoles P_l = (2l + 1) int_0^1 L_l(mu) P^s dmu, l = 0, 2, 4, of rsd_device's wedges on the device,
        (2, nz, n, 3) = (1-halo, 2-halo).  The 1-halo multipoles are exact in mu (the moments of the Gaussians in closed
        form inside the mass integral); the 2-halo ones are defined as the nmu-node Gauss-Legendre rule on [0, 1]
        (rsd.mu_rule, rsd.legendre_weights; 1 <= nmu <= 32) of the 2-halo wedge.  parts=True: (out, Q), Q (3, nz, n) the
        moment sums Q_0, Q_1, Q_2 of the 1-halo term (undamped by get_power_1halo's factor)."""
        mus, _ = rsdmod.mu_rule(nmu)
        wl = rsdmod.legendre_weights(nmu)
        recs, tables, alphas = self._rsd_request(name, name2, kindex, sigma_s, f, alphas, damping)
        out, Q = self._rsd_launch("hmg_rsd_multipoles", recs, tables, alphas, np.ascontiguousarray(mus), wl, 3,
                                  (lambda nz, n: (3, nz, n)) if parts else None)
        return (out, Q) if parts else out

    def get_power_multipoles(self, name, name2=None, ells=(0, 2, 4), term="total", nmu=16, kindex=None, sigma_s=None,
                             f=None, alphas=(1, 0, 1), damping=True):
        """The multipoles ells (of 0, 2, 4) of the redshift-space spectrum of the pair at the nodes ks[kindex], shape
        (len(ells), nz, n); term: "1h", "2h" or "total".  See multipoles_device."""
        ells = rsdmod.check_ells(ells)
        if term not in rsdmod.TERMS:
            raise ValueError(f"term must be one of {rsdmod.TERMS}, got {term!r}")
        out = self.multipoles_device(name, name2, nmu=nmu, kindex=kindex, sigma_s=sigma_s, f=f, alphas=alphas,
                                     damping=damping).numpy()
        picked = rsdmod.pick_term(out, term)
        return np.stack([picked[..., rsdmod.ELLS.index(e)] for e in ells])

    # ------------------------------------------------------------------ cluster lensing
    # The per-halo scalars are formed on the host one lens redshift at a time (a few values per halo), so that a z slice
    # of a model with several redshifts is the same computation as a model of that redshift alone.  With one redshift
    # the results have the reference's shapes; with nz > 1 a leading z axis is added.
    @staticmethod
    def _lensing_thetas(thetas):
        th = np.atleast_1d(np.asarray(thetas, dtype=np.float64)).ravel()
        if not np.all(np.isfinite(th)) or np.any(th <= 0):
            raise ValueError("thetas must be finite and positive")
        return th

    def _lensing_halos(self, Ms, concs, delta, rho, rho_at_z):
        """(Ms, concs, [(D_A, r_s, delta_c, rho_crit) per z]) of sigma_1h_profiles (hmvec/hmvec.py:574-589)."""
        Ms = np.atleast_1d(np.asarray(Ms, dtype=np.float64)).ravel()
        concs = np.atleast_1d(np.asarray(concs, dtype=np.float64)).ravel()
        if Ms.size != concs.size:
            raise ValueError("Ms and concs must have the same length")
        if not (np.all(np.isfinite(Ms)) and np.all(Ms > 0) and np.all(np.isfinite(concs)) and np.all(concs > 0)):
            raise ValueError("masses and concentrations must be finite and positive")
        if rho == "critical":
            rhofunc = self.rho_critical_z
        elif rho == "mean":
            rhofunc = self.rho_matter_z
        else:
            raise ValueError(f"rho must be 'mean' or 'critical', got {rho!r}")
        fcon = np.log(1.0 + concs) - (concs / (1.0 + concs))      # Fcon (hmvec/hmvec.py:737)
        rows = []
        for z in self.zs:
            zz = np.array([z])
            rhoz = zz if rho_at_z else zz * 0
            rs = _R_from_M(Ms, rhofunc(rhoz), delta=delta) / concs
            rhoc = self.rho_critical_z(zz)
            delta_c = Ms / 4 / np.pi / rs ** 3 / rhoc / fcon
            rows.append((float(self.angular_diameter_distance(zz)[0]), rs, delta_c, float(rhoc[0])))
        return Ms, concs, rows

    def sigma_1h_profiles(self, thetas, Ms, concs, sig_theta=None, delta=200, rho="mean", rho_at_z=True):
        """One-halo surface density Sigma [Msun/Mpc^2] of NFW halos (masses Ms, concentrations concs) at angles
        thetas [rad] (hmvec/hmvec.py:574-590): (nM, ntheta), or (nz, nM, ntheta) with several lens redshifts.
        sig_theta [rad] averages over Rayleigh-distributed miscentring of width D_A(z) sig_theta; 0 is the centred
        profile."""
        from .lensing import sigma_nfw
        return self._lensing_1h(sigma_nfw, thetas, Ms, concs, sig_theta, delta, rho, rho_at_z)

    def delta_sigma_1h_profiles(self, thetas, Ms, concs, sig_theta=None, delta=200, rho="mean", rho_at_z=True):
        """One-halo excess surface density Delta Sigma = Sigmabar(<R) - Sigma(R) [Msun/Mpc^2],
        with the arguments, conventions and shapes of sigma_1h_profiles: (nM, ntheta), or (nz, nM, ntheta)."""
        from .lensing import delta_sigma_nfw
        return self._lensing_1h(delta_sigma_nfw, thetas, Ms, concs, sig_theta, delta, rho, rho_at_z)

    def gamma_t_1h_profiles(self, thetas, Ms, concs, zsource, sig_theta=None, delta=200, rho="mean", rho_at_z=True):
        """One-halo tangential shear: delta_sigma_1h_profiles / Sigma_crit(z, zsource)."""
        dsigma = self.delta_sigma_1h_profiles(thetas, Ms, concs, sig_theta=sig_theta, delta=delta, rho=rho,
                                              rho_at_z=rho_at_z)
        return self._over_sigma_crit(dsigma, zsource)

    def _lensing_1h(self, profile, thetas, Ms, concs, sig_theta, delta, rho, rho_at_z):
        """sigma_1h_profiles / delta_sigma_1h_profiles: `profile` is lensing.sigma_nfw or lensing.delta_sigma_nfw."""
        th = self._lensing_thetas(thetas)
        Ms, _, rows = self._lensing_halos(Ms, concs, delta, rho, rho_at_z)
        if sig_theta is not None and (not np.isfinite(sig_theta) or sig_theta < 0):
            raise ValueError("sig_theta must be finite and non-negative")
        nz, nM, nt = self._nz, Ms.size, th.size
        rs = np.concatenate([r[1] for r in rows])
        dc = np.concatenate([r[2] for r in rows])
        rhoc = np.repeat([r[3] for r in rows], nM)
        rbins = np.repeat(np.stack([r[0] * th for r in rows]), nM, axis=0)           # (nz nM, ntheta)
        offsets = None
        if sig_theta is not None and sig_theta > 0:
            offsets = np.repeat([r[0] * float(sig_theta) for r in rows], nM)
        prof = profile(rs, dc, rhoc, rbins, offsets=offsets, ctx=self._main()).reshape(nz, nM, nt)
        return prof[0] if nz == 1 else prof

    def kappa_1h_profiles(self, thetas, Ms, concs, zsource, sig_theta=None, delta=200, rho="mean", rho_at_z=True):
        """sigma_1h_profiles / Sigma_crit(z, zsource) (hmvec/hmvec.py:592-595)."""
        sigma = self.sigma_1h_profiles(thetas, Ms, concs, sig_theta=sig_theta, delta=delta, rho=rho,
                                       rho_at_z=rho_at_z)
        return self._over_sigma_crit(sigma, zsource)

    def _over_sigma_crit(self, prof, zsource):
        """A one-halo profile ((nM, ntheta), or (nz, nM, ntheta)) over Sigma_crit(z, zsource) of its lens redshift."""
        sigmac = np.concatenate([np.atleast_1d(self.sigma_crit(np.array([z]), zsource)) for z in self.zs])
        return prof / sigmac[0] if self._nz == 1 else prof / sigmac[:, None, None]

    def kappa_2h_profiles(self, thetas, Ms, zsource, delta=200, rho="mean", rho_at_z=True, lmin=100, lmax=10000,
                          verbose=True):
        """Two-halo convergence (hmvec/hmvec.py:597-625) at angles thetas [rad] for halo masses Ms: (ntheta, nM), or
        (nz, ntheta, nM) with several lens redshifts.  delta, rho and rho_at_z are accepted and unused, as in the
        reference.  Ms outside the model's mass grid raise ValueError (the reference's interp1d does)."""
        from .lensing import kappa_2h_integral
        return self._lensing_2h(kappa_2h_integral, thetas, Ms, zsource, lmin, lmax, verbose)

    def gamma_t_2h_profiles(self, thetas, Ms, zsource, delta=200, rho="mean", rho_at_z=True, lmin=100, lmax=10000,
                            verbose=True):
        """Two-halo tangential shear: kappa_2h_profiles with J0(l theta) replaced by J2(l theta)
        (Oguri & Takada 2011), same arguments, conventions and shapes: (ntheta, nM), or (nz, ntheta, nM)."""
        from .lensing import gamma_t_2h_integral
        return self._lensing_2h(gamma_t_2h_integral, thetas, Ms, zsource, lmin, lmax, verbose)

    def delta_sigma_2h_profiles(self, thetas, Ms, delta=200, rho="mean", rho_at_z=True, lmin=100, lmax=10000,
                                verbose=True):
        """Two-halo excess surface density Sigma_crit(z, zsource) gamma_t^2h [Msun/Mpc^2]: gamma_t_2h_profiles without
        its 1/Sigma_crit, so no source redshift.  Shapes and keywords as kappa_2h_profiles; verbose prints the bias."""
        from .lensing import gamma_t_2h_integral
        return self._lensing_2h(gamma_t_2h_integral, thetas, Ms, None, lmin, lmax, verbose)

    def sigma_2h_profiles(self, thetas, Ms, delta=200, rho="mean", rho_at_z=True, lmin=100, lmax=10000,
                          verbose=True):
        """Two-halo surface density Sigma_crit(z, zsource) kappa_2h [Msun/Mpc^2]: kappa_2h_profiles without its
        1/Sigma_crit, so no source redshift.  Shapes and keywords as kappa_2h_profiles; verbose prints the bias."""
        from .lensing import kappa_2h_integral
        return self._lensing_2h(kappa_2h_integral, thetas, Ms, None, lmin, lmax, verbose)

    def _lensing_2h(self, integral, thetas, Ms, zsource, lmin, lmax, verbose):
        """The two-halo profiles: `integral` is lensing.kappa_2h_integral (J0) or gamma_t_2h_integral (J2); pre(z)
        carries 1/Sigma_crit(z, zsource) unless zsource is None."""
        th = self._lensing_thetas(thetas)
        Ms = np.atleast_1d(np.asarray(Ms, dtype=np.float64)).ravel()       # (finite and positive: `integral` checks)
        if np.any(Ms < self.ms[0]) or np.any(Ms > self.ms[-1]):
            raise ValueError("A value in x_new is outside the interpolation range of the model's mass grid")
        chi, pre, sigmac = [], [], []
        for z in self.zs:
            zz = np.array([z])
            dA = self.angular_diameter_distance(zz)
            if zsource is None:
                pre.append((self.rho_matter_z(zz) / (1 + zz) ** 3.0 / dA ** 2)[0])
            else:
                sc = np.atleast_1d(self.sigma_crit(zz, zsource))
                pre.append((self.rho_matter_z(zz) / (1 + zz) ** 3.0 / sc / dA ** 2)[0])
                sigmac.append(sc[0])
            chi.append(np.atleast_1d(self.comoving_radial_distance(zz))[0])
        ctx = self._main(needs_aux=True)
        out = integral(self.ks, np.array(chi), np.array(pre), self._d_Pzk(), th, lmin, lmax, self.ms, self._d_bh, Ms,
                       ctx=ctx)
        if verbose:
            bhs = np.stack([np.interp(Ms, self.ms, b) for b in self.bh])
            print("bias ", bhs)
            if zsource is not None:
                print("sigmacr ", np.array(sigmac))
        return out[0] if self._nz == 1 else out

    # ------------------------------------------------------------------ projected gas and pressure
    # Per-halo scalars on the host, one redshift at a time, as for the cluster-lensing profiles above: a z slice of a
    # batch is bit for bit a single-z model's result.
    def _gas_halos(self, Ms, concs, truncate):
        """(Ms, [(z, D_A, rho_crit, r_vir, M200c, R200c) per z]) with the mass conversion of add_battaglia_profile
        (hmvec/hmvec.py:215-225): the model's mass definition -> 200 rho_crit(z), concs=None the Duffy concentration."""
        Ms = np.atleast_1d(np.asarray(Ms, dtype=np.float64)).ravel()
        if not np.all(np.isfinite(Ms)) or np.any(Ms <= 0):
            raise ValueError("Ms must be finite and positive")
        if concs is not None:
            concs = np.atleast_1d(np.asarray(concs, dtype=np.float64)).ravel()
            if concs.size != Ms.size:
                raise ValueError("Ms and concs must have the same length")
            if not np.all(np.isfinite(concs)) or np.any(concs <= 0):
                raise ValueError("concs must be finite and positive")
        if not np.isfinite(truncate) or truncate <= 0:
            raise ValueError("truncate must be finite and positive")
        A, al, be = (float(self.p[f"duffy_{k}_{self.mdef}"]) for k in ("A", "alpha", "beta"))
        rows = []
        for z in self.zs:
            zz = np.array([z])
            rhoc = float(self.rho_critical_z(zz)[0])
            if self.mdef == "vir":
                drho1 = rhoc * float(self.deltav(zz)[0])
            elif self.mdef == "mean":
                drho1 = float(self.rho_matter_z(zz)[0]) * 200.0
            else:
                raise NotImplementedError(self.mdef)
            cs = A * (self.h * Ms / 2.0e12) ** al * (1.0 + z) ** be if concs is None else concs
            m200c = _mdelta_host(Ms, cs, drho1, 200.0 * rhoc)
            rows.append((float(z), float(self.angular_diameter_distance(zz)[0]), rhoc,
                         _R_from_M(Ms, drho1, delta=1.0), m200c, _R_from_M(m200c, rhoc, delta=200.0)))
        return Ms, rows

    def _projected_profile(self, kind, thetas, Ms, concs, truncate, fwhm, rowfn, norm="fit"):
        """prefactor x projected_gnfw(kind) for every (z, M, theta).  rowfn(z, rho_crit, M200c, R200c) returns the halo's
        (scale radius, alpha, gamma, eta, prefactor) with gamma one number.  norm="mass": the prefactor is M / (N r^2)
        instead, N = 4 pi int_0^xcut x^2 f dx from the "mean" kind at s = xcut."""
        from .gasprofiles import projected_gnfw
        th = self._lensing_thetas(thetas)
        if norm not in ("fit", "mass"):
            raise ValueError(f"norm must be 'fit' or 'mass', got {norm!r}")
        if fwhm is not None and (not np.isfinite(fwhm) or fwhm < 0):
            raise ValueError("fwhm must be finite and non-negative")
        Ms, halos = self._gas_halos(Ms, concs, truncate)
        x, alpha, eta, xcut, pref, smooth, rscale = [], [], [], [], [], [], []
        for z, da, rhoc, rvir, m200c, r200c in halos:
            r, al, gamma, et, pf = rowfn(z, rhoc, m200c, r200c)
            x.append(da * th[None, :] / r[:, None])
            alpha.append(al + 0.0 * r)
            eta.append(et)
            xcut.append(truncate * rvir / r)
            pref.append(pf)
            rscale.append(r)
            smooth.append(da * float(fwhm or 0.0) / np.sqrt(8.0 * np.log(2.0)) / r)
        x, alpha, eta, xcut, pref, smooth, rscale = (np.concatenate(a) for a in (x, alpha, eta, xcut, pref, smooth, rscale))
        ctx = self._main()
        if norm == "mass":
            N = projected_gnfw(xcut[:, None], alpha, gamma, eta, xcut, kind="mean", ctx=ctx)[:, 0] * np.pi * xcut ** 2
            pref = np.tile(Ms, self._nz) / (N * rscale ** 2)
        prof = projected_gnfw(x, alpha, gamma, eta, xcut, kind=kind, smooth=smooth if fwhm else None, ctx=ctx)
        prof = (pref[:, None] * prof).reshape(self._nz, Ms.size, th.size)
        return prof[0] if self._nz == 1 else prof

    def _gas_rowfn(self, family, param_override):
        """Battaglia gas density (hmvec/hmvec.py:844-860) as a member of the family: x = r / (R200c / 2),
        eta = (beta + gamma) / alpha, amplitude (Omega_b / Omega_m) rho_crit(z) rho0 times the scale radius."""
        pp = self._battaglia_gas_pparams(family, param_override)
        gamma = float(pp["battaglia_gas_gamma"])
        fb = self.p["ombh2"] / self.h ** 2.0 / self.omm0

        def rowfn(z, rhoc, m200c, r200c):
            rho0, alpha, beta = (_battaglia_fit(m200c, z, *(pp[q + s] for s in ("A0", "alpham", "alphaz")))
                                 for q in ("rho0_", "alpha_", "beta_"))
            rg = 0.5 * r200c
            return rg, alpha, gamma, (beta + gamma) / alpha, fb * rhoc * rho0 * rg
        return rowfn

    def gas_sigma_1h_profiles(self, thetas, Ms, concs=None, family=None, param_override=None, truncate=1.0, norm="fit",
                              fwhm=None):
        """Projected gas surface density Sigma_gas [Msun/Mpc^2] of the Battaglia gas profile (the profile of
        add_battaglia_profile) around halos of mass Ms (the model's mass definition; concs=None: Duffy) at angles thetas
        [rad]: (nM, ntheta), or (nz, nM, ntheta) with several redshifts.  The profile is cut at truncate r_vir.
        norm="fit": the amplitude of the fit, (Omega_b / Omega_m) rho_crit(z) rho0; norm="mass": the same shape holding
        the halo mass Ms inside the cut (the profile whose transform uk_profiles approximates).  fwhm [rad]: convolved
        with a circular Gaussian beam of that full width at half maximum.  family and param_override as in
        add_battaglia_profile."""
        return self._projected_profile("sigma", thetas, Ms, concs, truncate, fwhm,
                                       self._gas_rowfn(family, param_override), norm)

    def gas_delta_sigma_1h_profiles(self, thetas, Ms, concs=None, family=None, param_override=None, truncate=1.0,
                                    norm="fit"):
        """Excess gas surface density Sigmabar_gas(<R) - Sigma_gas(R) [Msun/Mpc^2]; arguments, conventions and shapes of
        gas_sigma_1h_profiles (no beam)."""
        return self._projected_profile("excess", thetas, Ms, concs, truncate, None,
                                       self._gas_rowfn(family, param_override), norm)

    def tau_1h_profiles(self, thetas, Ms, concs=None, family=None, param_override=None, truncate=1.0, fwhm=None):
        """Thomson optical depth tau(theta) = sigma_T (1 + X_H) / (2 m_p) Sigma_gas of fully ionised gas with hydrogen
        mass fraction X_H = 0.76 (norm="fit"); dimensionless.  Arguments and shapes of gas_sigma_1h_profiles."""
        sigma_gas = self.gas_sigma_1h_profiles(thetas, Ms, concs=concs, family=family, param_override=param_override,
                                               truncate=truncate, norm="fit", fwhm=fwhm)
        sigmaT = constants.physical_constants["Thomson cross section"][0] / (default_params["parsec"] * 1e6) ** 2
        m_p = constants.physical_constants["proton mass"][0] / default_params["mSun"]
        return sigmaT * (1.0 + _X_H) / (2.0 * m_p) * sigma_gas

    def y_1h_profiles(self, thetas, Ms, concs=None, family=None, param_override=None, truncate=1.0, fwhm=None):
        """Compton-y profile y(theta) = sigma_T / (m_e c^2) int P_e dl of the Battaglia pressure profile (the profile of
        add_battaglia_pres_profile; hmvec/hmvec.py:906-927, units of 313-316), dimensionless: (nM, ntheta), or
        (nz, nM, ntheta).  Arguments as gas_sigma_1h_profiles; family and param_override as in
        add_battaglia_pres_profile."""
        return self._projected_profile("sigma", thetas, Ms, concs, truncate, fwhm, self._pres_rowfn(family, param_override))

    def _pres_rowfn(self, family, param_override):
        """Battaglia pressure profile as a member of the family, in Compton-y units: x = r / (xc R200c), eta = beta,
        amplitude sigma_T / (m_e c^2) A_P times the scale radius."""
        pp = self._battaglia_pres_pparams(family, param_override)
        gamma, alpha = float(pp["battaglia_pres_gamma"]), float(pp["battaglia_pres_alpha"])
        eFrac = 2.0 * (_X_H + 1.0) / (5.0 * _X_H + 3.0)
        G_newt = constants.G / (default_params["parsec"] * 1e6) ** 3 * default_params["mSun"]
        sigmaT = constants.physical_constants["Thomson cross section"][0]
        mElect = constants.physical_constants["electron mass"][0] / default_params["mSun"]
        fb = self.p["ombh2"] / self.h ** 2.0 / self.omm0

        def rowfn(z, rhoc, m200c, r200c):
            P0, xc, beta = (_battaglia_fit(m200c, z, *(pp[q + s] for s in ("A0", "alpham", "alphaz")))
                            for q in ("P0_", "xc_", "beta_"))
            rp = xc * r200c
            A_P = eFrac * fb * 200.0 * m200c * G_newt * rhoc / (2.0 * r200c) * P0
            return rp, alpha, gamma, beta, sigmaT / (mElect * constants.c ** 2) * A_P * rp
        return rowfn

    # ------------------------------------------------------------------ one-point PDF
    # P(y) of a Compton-y map and the PDF of any field that is a sum of halo profiles on the sky, for Poisson-placed halos
    # (hmg_onepoint_exponent, hmg_onepoint_moments).  The host side of the contract - the grid in lambda, the ring rule,
    # the transform, the checks - is onepoint.py.  Every refusal happens on the host before a context is touched: the
    # *_request methods check and build host arrays, _onepoint_launch is the only one that reaches the device.
    def _onepoint_request(self, ntheta, mmin, mmax, zweights):
        """(u, w, (m_lo, m_hi), zw) of the shared tail of the one-point methods."""
        u, w = onepoint.ring_rule(ntheta)
        ms = np.asarray(self.ms, dtype=np.float64)
        for name, v in (("mmin", mmin), ("mmax", mmax)):
            if v is not None and not (np.isscalar(v) and np.isfinite(v) and v > 0):
                raise ValueError(f"{name} must be a finite positive mass or None, got {v!r}")
        keep = np.nonzero((ms >= (ms[0] if mmin is None else mmin)) & (ms <= (ms[-1] if mmax is None else mmax)))[0]
        if keep.size == 0:
            raise ValueError(f"no point of the mass grid lies in mmin .. mmax = {mmin!r} .. {mmax!r}")
        if zweights is None:
            if self._nz < 2:
                raise ValueError("zweights=None needs at least two redshifts (the default is a trapezoid rule over zs times "
                                 "the comoving volume per steradian); give the weight of the one redshift")
            zs = np.asarray(self.zs, dtype=np.float64)
            chi = np.asarray(self.comoving_radial_distance(zs), dtype=np.float64).reshape(-1)
            hz = np.asarray(self.hubble_parameter(zs), dtype=np.float64).reshape(-1)
            zweights = trapz_weights(zs) * (constants.c / 1.0e3) * chi ** 2 / hz       # dz dV/dz/dOmega, comoving Mpc^3/sr
        return u, w, (int(keep[0]), int(keep[-1]) + 1), onepoint.check_zweights(zweights, self._nz)

    def _profile_request(self, profiles, theta_out, ntheta, mmin, mmax, zweights):
        u, w, window, zw = self._onepoint_request(ntheta, mmin, mmax, zweights)
        shape = (self._nz, self._nm, u.size)
        got = profiles.shape if isinstance(profiles, nat.DeviceArray) else np.shape(profiles)
        if tuple(got) != shape:
            raise ValueError(f"profiles must have shape (nz, nm, ntheta) = {shape}, got {tuple(got)}")
        if not isinstance(profiles, nat.DeviceArray):
            profiles = np.ascontiguousarray(profiles, dtype=np.float64)
            if not np.all(np.isfinite(profiles)):
                raise ValueError("profiles must be finite")
        theta_out = np.asarray(theta_out, dtype=np.float64)
        if theta_out.shape != shape[:2]:
            raise ValueError(f"theta_out must have shape (nz, nm) = {shape[:2]}, got {theta_out.shape}")
        if not np.all(np.isfinite(theta_out)) or np.any(theta_out <= 0):
            raise ValueError("theta_out must be finite and positive")
        area = (2.0 * np.pi * theta_out ** 2)[:, :, None] * (u * w)[None, None, :]
        return dict(signal=profiles, amp=None, area=area, window=window, zw=zw)

    def _y_request(self, truncate, fwhm, family, param_override, ntheta, mmin, mmax, zweights):
        """The rings of every (zs, ms) halo's Compton-y profile: the arguments of the projection in scaled units, the
        amplitudes and the solid angles, all on the host."""
        u, w, window, zw = self._onepoint_request(ntheta, mmin, mmax, zweights)
        if fwhm is not None and not (np.isscalar(fwhm) and np.isfinite(fwhm) and fwhm >= 0):
            raise ValueError("fwhm must be finite and non-negative")
        beam = float(fwhm or 0.0) / np.sqrt(8.0 * np.log(2.0))
        rowfn = self._pres_rowfn(family, param_override)
        Ms, halos = self._gas_halos(self.ms, None, truncate)
        x, alpha, eta, xcut, pref, smooth, theta_out = [], [], [], [], [], [], []
        for z, da, rhoc, rvir, m200c, r200c in halos:
            r, al, gamma, et, pf = rowfn(z, rhoc, m200c, r200c)
            tout = truncate * rvir / da + 5.0 * beam
            x.append(da * (tout[:, None] * u[None, :]) / r[:, None])       # (the operations of y_1h_profiles at tout u)
            alpha.append(al + 0.0 * r)
            eta.append(et)
            xcut.append(truncate * rvir / r)
            pref.append(pf)
            smooth.append(da * beam / r)
            theta_out.append(tout)
        x, alpha, eta, xcut, smooth = (np.concatenate(a) for a in (x, alpha, eta, xcut, smooth))
        pref, theta_out = np.stack(pref), np.stack(theta_out)
        for name, a in (("the profile's parameters", np.concatenate([alpha, eta, xcut, pref.ravel()])), ("the ring radii", x)):
            if not np.all(np.isfinite(a)):
                raise ValueError(f"{name} are not finite")
        area = (2.0 * np.pi * theta_out ** 2)[:, :, None] * (u * w)[None, None, :]
        return dict(signal=None, proj=(x, alpha, gamma, eta, xcut, smooth if beam > 0 else None), amp=pref, area=area,
                    window=window, zw=zw)

    def _onepoint_launch(self, req, grid, per_z):
        """The contraction of a checked request on the device; grid = (nlambda, dlambda), or None for the cumulants."""
        ctx = self._main(needs_aux=True)
        signal = req["signal"]
        if signal is None:          # the profiles stay on the device
            from .gasprofiles import projected_gnfw_device
            signal = projected_gnfw_device(*req["proj"], ctx=ctx)
        arrays = (signal, req["area"], self._d_nzm, self._d_wm(), req["zw"])
        dims = (self._nz, self._nm, req["area"].shape[-1])
        if grid is None:
            out = onepoint._moments(ctx, arrays, req["amp"], dims, req["window"], per_z)
        else:
            out = onepoint._exponent(ctx, arrays, req["amp"], dims, req["window"], *grid, per_z)
        self._sync_point()
        return out

    def profile_char_exponent(self, profiles, theta_out, nbins, ds, ntheta=onepoint.DEFAULT_RINGS, mmin=None, mmax=None,
                              zweights=None, per_z=False):
        """The exponent A(lambda_j) of the characteristic function exp A of a field that is the sum of the profiles of
        Poisson-placed halos of the model's mass function, on onepoint.lambda_grid(nbins, ds): complex (nbins / 2 + 1,),
        or with per_z=True its rows (nz, nbins / 2 + 1).  profiles (nz, nm, ntheta), a host array or a device buffer, is
        the profile of a halo of mass ms[m] at zs[z] at the angles theta_out[z, m] u_t [rad], u = onepoint.ring_rule(ntheta)
        [0], and zero beyond theta_out (nz, nm) - built from kappa_1h_profiles, for instance.  zweights (nz,): the weight
        of a redshift, default trapz_weights(zs) c chi^2 / H, the comoving volume per steradian that goes with the comoving
        mass function; mmin, mmax: only the masses of the grid in [mmin, mmax].  onepoint.pdf_from_exponent turns the
        result into the PDF.  Halo clustering is neglected; overlapping halos are not."""
        grid = onepoint.lambda_grid(nbins, ds)
        req = self._profile_request(profiles, theta_out, ntheta, mmin, mmax, zweights)
        return self._onepoint_launch(req, grid, bool(per_z))

    def get_y_char_exponent(self, nbins, dy, truncate=1.0, fwhm=None, family=None, param_override=None,
                            ntheta=onepoint.DEFAULT_RINGS, mmin=None, mmax=None, zweights=None, per_z=False):
        """profile_char_exponent of the Compton-y profile of y_1h_profiles (the Battaglia pressure profile cut at
        truncate r_vir, Duffy concentrations; family and param_override as in add_battaglia_pres_profile) of every
        (zs, ms) halo, on lambda_grid(nbins, dy).  The rings end at theta_out = truncate r_vir / D_A, with fwhm [rad] (the
        beam the profile is convolved with) at 5 beam widths sigma = fwhm / sqrt(8 ln 2) beyond.  The profiles are
        evaluated and contracted on the device."""
        grid = onepoint.lambda_grid(nbins, dy)
        req = self._y_request(truncate, fwhm, family, param_override, ntheta, mmin, mmax, zweights)
        return self._onepoint_launch(req, grid, bool(per_z))

    def get_y_pdf(self, nbins, dy, ymin=0.0, noise_sigma=0.0, truncate=1.0, fwhm=None, family=None, param_override=None,
                  ntheta=onepoint.DEFAULT_RINGS, mmin=None, mmax=None, zweights=None, per_z=False):
        """(ys, p): the one-point PDF of the Compton-y map in nbins bins of width dy from ymin, p the probability per bin
        (nbins,), with Gaussian map noise of width noise_sigma - onepoint.pdf_from_exponent of get_y_char_exponent; see
        there for the periodicity and for why noise_sigma >~ 2 dy.  per_z=True: p (nz, nbins), the PDF of each redshift's
        halos alone."""
        grid = onepoint.lambda_grid(nbins, dy)
        noise_sigma = onepoint.check_noise(noise_sigma)
        if not (np.isscalar(ymin) and np.isfinite(ymin)):
            raise ValueError("ymin must be finite")
        req = self._y_request(truncate, fwhm, family, param_override, ntheta, mmin, mmax, zweights)
        A = self._onepoint_launch(req, grid, bool(per_z))
        if not per_z:
            return onepoint.pdf_from_exponent(A, dy, ymin, noise_sigma)
        rows = [onepoint.pdf_from_exponent(a, dy, ymin, noise_sigma) for a in A]
        return rows[0][0], np.stack([p for _, p in rows])

    def get_y_cumulants(self, truncate=1.0, fwhm=None, family=None, param_override=None, ntheta=onepoint.DEFAULT_RINGS,
                        mmin=None, mmax=None, zweights=None, per_z=False):
        """[<y>, kappa_2, kappa_3, kappa_4]: the mean and the second to fourth cumulant of the Compton-y map of
        get_y_char_exponent (without noise), kappa_p = sum zw wm n a y^p; (4,), or with per_z=True (nz, 4)."""
        req = self._y_request(truncate, fwhm, family, param_override, ntheta, mmin, mmax, zweights)
        return self._onepoint_launch(req, None, bool(per_z))

    # ------------------------------------------------------------------ HOD parameter ensembles
    # P_gg and P_gm of S parameter sets in one pass over the tensors (hmg_hod_ensemble, hmg_hod_ensemble_power).  The host
    # side of the contract - the table of sets, the stencil, the checks - is hod_ensemble.py.  Nothing is registered in
    # hods and the model's version does not change: cached spectra stay valid.
    def _hodens_request(self, sets, mthresh, ngal, corr):
        """(sets (S, 6), corr flag, log10 thresholds (S, nz) or None, n_gal targets (S, nz) or None): every refusal of the
        HOD half of a request, on the host."""
        sets = hodens.as_sets(sets)
        if (mthresh is None) == (ngal is None):
            raise ValueError("give exactly one of mthresh and ngal")
        S, nz = sets.shape[0], self._nz
        flag = hodens.check_corr(corr)
        if ngal is not None:
            return sets, flag, None, hodens.per_set(ngal, S, nz, "ngal")
        return sets, flag, np.log10(hodens.per_set(mthresh, S, nz, "mthresh")), None

    def _hodens_occ(self, ctx, d_par, flag, l10, S, occ=None, coef=None):
        """One hmg_hod_ensemble launch at the thresholds l10 (S, nz): (d_lthr, d_ngal, d_bg)."""
        nz, nm = self._nz, self._nm
        d_thr, d_ngal, d_bg = ctx.upload(np.ascontiguousarray(l10)), ctx.empty((S, nz)), ctx.empty((S, nz))
        ctx.call("hmg_hod_ensemble", S=S, nz=nz, nm=nm, corr=flag, d_par=d_par.ptr, d_lthr=d_thr.ptr, d_zs=self._d_zs().ptr,
                 **self._model_block("hmg_hod_ensemble"), d_ngal=d_ngal.ptr, d_bg=d_bg.ptr, d_occ=nat.ptr(occ),
                 d_coef=nat.ptr(coef))
        return d_thr, d_ngal, d_bg

    def _hodens_bisect(self, ctx, d_par, target):
        """log10 mthresh (S, nz) by one batched bisection, and its number of launches.  The rules are those of
        utils.vectorized_bisection_search with the stop test per set: a set stops updating once all of its redshifts meet
        hod_bisection_search_rtol - the thresholds add_hod(ngal=target[s]) finds for that set alone - while the others go
        on; the number of launches is the largest iteration count."""
        p = self.p
        S = target.shape[0]
        lo = np.zeros_like(target) + p["hod_bisection_search_min_log10mthresh"]
        hi = np.zeros_like(target) + p["hod_bisection_search_max_log10mthresh"]
        out = np.zeros_like(target)
        active = np.ones(S, dtype=bool)
        n_iter, warned = 0, False
        while active.any():
            mid = np.where(active[:, None], (lo + hi) / 2.0, out)
            got = self._hodens_occ(ctx, d_par, 0, mid, S)[1].numpy()
            miss = (got - target) / target
            out[active] = mid[active]
            hodens.bisection_step(lo, hi, mid, miss, active)
            active &= np.any(np.abs(miss) > p["hod_bisection_search_rtol"], axis=1)
            n_iter += 1
            if n_iter > p["hod_bisection_search_warn_iter"] and not warned:
                print("WARNING: Bisection search has done more than ", p["hod_bisection_search_warn_iter"],
                      " loops. Still searching...")
                warned = True
        return out, n_iter

    def _hodens_thresholds(self, ctx, d_par, l10, target):
        """The log10 thresholds of a request as add_hod forms them, and the bisection's launches."""
        if l10 is not None:
            return l10, 0
        lm, n_iter = self._hodens_bisect(ctx, d_par, target)
        return np.log10(10 ** (lm * self.p["hod_A_log10mthresh"])), n_iter

    def _hodens_tensor(self, name, what):
        if name in self.pk_profiles and name not in self.uk_profiles:
            raise ValueError(f"{what} {name!r} is a pressure profile: an HOD ensemble takes matter profiles")
        if name not in self.uk_profiles:
            raise ValueError(f"{what} {name!r} is not a matter profile of this model")
        return name

    def hod_ensemble_device(self, sets, mthresh=None, ngal=None, corr="max", satellite_profile_name="nfw", matter_name=None,
                            kindex=None, damping=True, parts=False):
        """P_gg and P_gm of S HOD parameter sets at once, on the device: a hod_ensemble.HodEnsembleResult with power
        (4, S, nz, n) = (P1h_gg, P2h_gg, P1h_gm, P2h_gm), ngal, bg and log10mthresh (S, nz) and parts (3, S, nz, n) =
        (G, X, I) or None.  sets: (S, 6) as hod_ensemble.hod_sets makes them; exactly one of mthresh and ngal, each (nz,),
        shared by the sets, or (S, nz) - ngal runs one batched bisection whose thresholds are those add_hod(ngal=...)
        finds for each set alone.  Plane by plane the result is get_power_1halo / get_power_2halo of (g_s, g_s) and
        (g_s, matter_name) for g_s = add_hod(mthresh=..., corr=corr, satellite_profile_name=..., param_override=set s)
        without a central profile; matter_name defaults to the satellite profile.  kindex: the nodes of the k grid
        (default: all); damping as in get_power_1halo.  Nothing is registered in hods; cached spectra stay valid."""
        sets, flag, l10, target = self._hodens_request(sets, mthresh, ngal, corr)
        sat = self._hodens_tensor(satellite_profile_name, "satellite_profile_name")
        mat = sat if matter_name is None else self._hodens_tensor(matter_name, "matter_name")
        nz, nm, nk = self._nz, self._nm, self._nk
        kindex = hodens.check_kindex(kindex, nk)
        S, n = sets.shape[0], nk if kindex is None else kindex.size
        nodes = self.ks if kindex is None else self.ks[kindex]
        damp = bispec.damping(nodes, self.p["kstar_damping"]) if damping else np.ones(n)
        ctx = self._main(needs_aux=True)
        shape = (nz, nm, nk)
        # (another reader of the tensors than the batched mass integrals: a deferred left fill is written first)
        d_us = self.uk_profiles.dev(sat, fill=True)
        d_um = d_us if mat == sat else self.uk_profiles.dev(mat, fill=True)
        for nm_, d_ in ((sat, d_us), (mat, d_um)):
            if d_.shape != shape:
                raise ValueError(f"profile {nm_!r} has shape {d_.shape}, the model's grid is {shape}")
        d_par = ctx.upload(sets)
        l10, n_iter = self._hodens_thresholds(ctx, d_par, l10, target)
        coef = ctx.empty((hodens.coef_block_size(S, nz, nm),))
        d_thr, d_ngal, d_bg = self._hodens_occ(ctx, d_par, flag, l10, S, coef=coef)
        d_k = None if kindex is None else ctx.upload_int32(kindex)
        d_damp = ctx.upload(np.ascontiguousarray(damp, dtype=np.float64))
        out = ctx.empty((4, S, nz, n))
        P = ctx.empty((3, S, nz, n)) if parts else None
        ctx.call("hmg_hod_ensemble_power", S=S, nz=nz, nm=nm, nk=nk, n=n, d_us=d_us.ptr, d_um=d_um.ptr, d_coef=coef.ptr,
                 d_ngal=d_ngal.ptr, d_bg=d_bg.ptr, **self._model_block("hmg_hod_ensemble_power"), d_kindex=nat.ptr(d_k),
                 d_damp=d_damp.ptr, d_out=out.ptr, d_parts=nat.ptr(P))
        self._sync_point()
        return hodens.HodEnsembleResult(out, d_ngal, d_bg, d_thr, P, n_iter)

    def get_power_hod_ensemble(self, sets, mthresh=None, ngal=None, corr="max", satellite_profile_name="nfw",
                               matter_name=None, kindex=None, damping=True, parts=False):
        """hod_ensemble_device on the host: a dict of gg_1h, gg_2h, gg, gm_1h, gm_2h, gm, each (S, nz, n), and ngal, bg,
        log10mthresh (S, nz); with parts=True also G, X, I (S, nz, n)."""
        r = self.hod_ensemble_device(sets, mthresh=mthresh, ngal=ngal, corr=corr,
                                     satellite_profile_name=satellite_profile_name, matter_name=matter_name, kindex=kindex,
                                     damping=damping, parts=parts)
        power = r.power.numpy()
        out = dict(zip(hodens.POWER_KEYS, power))
        out["gg"], out["gm"] = power[0] + power[1], power[2] + power[3]
        out["ngal"], out["bg"], out["log10mthresh"] = r.ngal.numpy(), r.bg.numpy(), r.log10mthresh.numpy()
        if parts:
            out.update(zip(("G", "X", "I"), r.parts.numpy()))
        return out

    def hod_ensemble_occupations(self, sets, mthresh=None, ngal=None, corr="max"):
        """{Nc, Ns, NsNsm1, NcNs (S, nz, nm), ngal, bg (S, nz)}: the occupation numbers and sums of every set, each the
        bits add_hod gives for that set alone."""
        sets, flag, l10, target = self._hodens_request(sets, mthresh, ngal, corr)
        S = sets.shape[0]
        ctx = self._main(needs_aux=True)
        d_par = ctx.upload(sets)
        l10, _ = self._hodens_thresholds(ctx, d_par, l10, target)
        occ = ctx.empty((4, S, self._nz, self._nm))
        _, d_ngal, d_bg = self._hodens_occ(ctx, d_par, flag, l10, S, occ=occ)
        self._sync_point()
        out = dict(zip(("Nc", "Ns", "NsNsm1", "NcNs"), occ.numpy()))
        out["ngal"], out["bg"] = d_ngal.numpy(), d_bg.numpy()
        return out


_X_H = 0.76      # hydrogen mass fraction of the Battaglia profiles (hmvec/hmvec.py:922)


def _battaglia_fit(m200c, z, A0, alpham, alphaz):
    """A0 (M200c / 1e14)^alpha_m (1+z)^alpha_z on the host (hmvec/hmvec.py:800-802)."""
    return A0 * (m200c / 1.0e14) ** alpham * (1.0 + z) ** alphaz


def _mdelta_host(M1, c1, drho1, drho2):
    """Mass in the definition Delta rho = drho2 of NFW halos of mass M1 and concentration c1 in the definition drho1
    (hmvec/hmvec.py:770-798) on the host: equal r_s and rho_s give M2 / F(c2) = M1 / F(c1) with
    c2 = c1 (M2 drho1 / (M1 drho2))^(1/3), F(c) = ln(1+c) - c/(1+c); Newton in ln(M2/M1) to machine precision."""
    def F(c):
        return np.log1p(c) - c / (1.0 + c)
    lnF1 = np.log(F(c1))
    lq = np.zeros_like(M1)
    for _ in range(60):
        c2 = c1 * (np.exp(lq) * drho1 / drho2) ** (1.0 / 3.0)
        F2 = F(c2)
        resid = lq - np.log(F2) + lnF1
        dlnF = c2 * c2 / (1.0 + c2) ** 2 / F2           # d ln F / d ln c
        step = resid / (1.0 - dlnF / 3.0)
        lq = lq - step
        if np.all(np.abs(step) < 1e-15):
            break
    return M1 * np.exp(lq)


class _HostBlock:
    """The spectra of one batched launch on the host: fetched in one copy on first use.  Every array handed out is the
    caller's own, as in the reference (a fresh array per call): a slice of the fetched block the first time a spectrum
    is asked for, a new copy from the device after that (the first caller may have written into its slice)."""

    def __init__(self, dev):
        self.dev, self.host, self.given = dev, None, set()

    def take(self, i):
        if i in self.given:
            n = self.dev.shape[1] * self.dev.shape[2]
            return self.dev.view(i * n, self.dev.shape[1:]).numpy()
        if self.host is None:
            self.host = self.dev.numpy()
        self.given.add(i)
        return self.host[i]


class SpectraBlock:
    """See HaloModel.spectra_block.  With ``nbuf=2`` the block is double-buffered for streams of passes (parameter
    sweeps): ``compute(slot)`` enqueues pass i into device block i % 2, ``fetch_async(slot)`` sends it to its pinned
    twin on the context's copy lane behind an event, and pass i+1's kernels run while that copy is in flight;
    ``wait(slot)`` blocks the host on that one copy only and returns the views.  The next ``compute(slot)`` of the
    same slot is ordered behind the copy on the device, so no result is overwritten before it has left."""

    _COPY_LANE = 2
    _EV_READY, _EV_DONE = 10, 12       # event slots 10-11, 12-13 (HaloModel: 0-3, ShardedSpectra: 8-9, bench.py: 40+)

    def __init__(self, model, pairs, nbuf=1):
        self.model = model
        self.pairs = [(a, a if b is None else b) for a, b in pairs]
        ctx = model._ctx()
        nz, nk = model.zs.size, model.ks.size
        n = 2 * len(self.pairs)
        self.nbuf = int(nbuf)
        self._devs = [ctx.empty((n, nz, nk)) for _ in range(self.nbuf)]
        self._views = [[d.view(i * nz * nk, (nz, nk)) for i in range(n)] for d in self._devs]
        self._hosts = [nat.PinnedArray(ctx, (n, nz, nk)) for _ in range(self.nbuf)]
        self._inflight = [False] * self.nbuf
        self.dev, self.views, self.host = self._devs[0], self._views[0], self._hosts[0]
        self.nbytes = self.dev.nbytes

    def compute(self, slot=0):
        """Launch-only: the spectra of all pairs into device block `slot` (behind the copy that last read it)."""
        if self._inflight[slot]:
            self.model._ctx().wait(self._EV_DONE + slot)
        self.model.power_device_batch(self.pairs, self._views[slot][0::2], self._views[slot][1::2])

    def _as_dict(self, slot):
        a = self._hosts[slot].array
        return {p: (a[2 * i], a[2 * i + 1]) for i, p in enumerate(self.pairs)}

    def fetch(self, slot=0):
        """{(name, name2): (P_1h, P_2h)} as views of the pinned host block; blocks until the copy lands."""
        ctx = self.model._ctx()
        ctx.copy_to_pinned(self._hosts[slot], self._devs[slot])
        ctx.sync()
        self._inflight[slot] = False
        return self._as_dict(slot)

    def fetch_async(self, slot=0):
        """Start the copy of block `slot` on the copy lane, behind the launches enqueued so far; returns at once."""
        ctx = self.model._ctx()
        ctx.record(self._EV_READY + slot)
        ctx.lane(self._COPY_LANE)
        ctx.wait(self._EV_READY + slot)
        ctx.copy_to_pinned(self._hosts[slot], self._devs[slot])
        ctx.record(self._EV_DONE + slot)
        ctx.lane(0)
        self._inflight[slot] = True

    def wait(self, slot=0):
        """Views of block `slot` once its copy has landed (the device may already be busy with later passes)."""
        if self._inflight[slot]:
            self.model._ctx().event_synchronize(self._EV_DONE + slot)
        return self._as_dict(slot)


class _LazyArray:
    """Return value of add_nfw_profile's second element: behaves as the ndarray when used."""

    def __init__(self, mapping, name):
        self._m, self._n = mapping, name

    def __array__(self, dtype=None, copy=None):
        a = self._m[self._n]
        return a if dtype is None else a.astype(dtype)

    def __getattr__(self, k):
        return getattr(self._m[self._n], k)

    def __getitem__(self, idx):
        return self._m[self._n][idx]
