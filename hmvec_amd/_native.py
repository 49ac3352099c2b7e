"""ctypes binding of libhmgrid.so (C ABI in include/hmgrid.h).

Nothing of the ABI is written down here a second time: at import, _abi.py reads the header and this module publishes
what it finds - SIGNATURES (name -> argtypes), PARAMS (name -> parameter names), DEFINES (HMG_<NAME> -> integer), the
Structure classes (Tracer, HodPart, ...) and the constants under their short names (HOD_ALL, GNFW_SIGMA, ...).  A
pointer named d_* is bound as a device address, one named h_* as typed host memory; a header the reader does not
understand fails the import.  Context.call takes keywords by the header's parameter names (arguments()).

There is NO CPU fallback: if the shared library is missing or a call fails, this
module raises.  Build the library with ``python -c "import __graft_entry__ as g; g.build()"``
or ``make -C hmvec_amd/csrc``.
"""
import ctypes as C
import math
import os

import numpy as np

from . import _abi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("HMG_LIB_PATH") or os.path.join(_HERE, "libhmgrid.so")   # override: tuning experiments only

c_double_p = C.c_void_p  # device or host pointers travel as plain addresses


class NativeError(RuntimeError):
    pass


HEADER_PATH = os.path.normpath(os.path.join(_HERE, "..", "include", "hmgrid.h"))   # the tree travels whole: no installed layout
_STRUCTS = {"hmg_halo_stage_args": "HaloStageArgs", "hmg_massfn_params": "MassFnParams", "hmg_hod_params": "HodParams",
            "hmg_tracer": "Tracer", "hmg_massfn_part": "MassFnPart", "hmg_hod_part": "HodPart",
            "hmg_rows_part": "RowsPart", "hmg_nfw_part": "NfwPart", "hmg_profile_fft_part": "ProfileFftPart",
            "hmg_power_batch_desc": "PowerBatchDesc"}
# DEFINES: HMG_<NAME> -> integer; SIGNATURES: name -> argtypes (restype is int for all but hmg_last_error); PARAMS: name ->
# parameter names.  Read once, here, without the library: a header the reader does not understand fails the import.
try:
    with open(HEADER_PATH) as _f:
        DEFINES, _structs, SIGNATURES, PARAMS = _abi.read(_f.read(), _STRUCTS)
except OSError as e:
    raise ImportError(f"{HEADER_PATH}: the C ABI's header cannot be read ({e}); the binding is derived from it") from e
globals().update({_STRUCTS[c]: s for c, s in _structs.items()})      # nat.Tracer, nat.HodPart, ...
ABI_VERSION = DEFINES["HMG_ABI_VERSION"]
globals().update({n: DEFINES["HMG_" + n] for n in (
    "PB_PREPARED", "HOD_ALL", "HOD_OCCUPATIONS", "HOD_SUMS", "MF_SHETH_TORMEN", "MF_TINKER10", "PROF_BATTAGLIA_GAS",
    "PROF_BATTAGLIA_PRES", "TRACER_MATTER", "TRACER_HOD", "TRACER_PRESSURE", "KERNEL_POWER", "KERNEL_NFW",
    "KERNEL_PROFILE_FFT", "EVENT_SLOTS", "NFW_SERIES_STRIDE", "ROWSC_STRIDE", "GNFW_SIGMA", "GNFW_MEAN", "GNFW_EXCESS",
    "GNFW_GENERAL", "GNFW_TABLE_DOUBLES", "COMM_ID_BYTES")})
_I, _D, _P, _Z = C.c_int, C.c_double, C.c_void_p, C.c_size_t


def arguments(name, args, kw):
    """The arguments of entry point `name` behind its context handle as one positional tuple: `args`, then the keywords
    `kw` placed by the header's parameter names.  Raises NativeError on an unknown, duplicate or missing name."""
    ctx, *names = PARAMS.get(name) or (None,)
    if ctx != "ctx":
        raise NativeError(f"{name}: not an entry point that takes a context")
    given, rest = names[:len(args)], names[len(args):]
    bad = ([f"unknown {k}" for k in kw if k not in names] + [f"duplicate {k}" for k in kw if k in given]
           + [f"missing {n}" for n in rest if n not in kw])
    if bad or len(args) > len(names):
        raise NativeError(f"{name}: {', '.join(bad) or f'{len(args)} arguments for {len(names)} parameters'}")
    return (*args, *(kw[n] for n in rest))


_lib = None


def kernel_source_sha16():
    """First 16 hex digits of the SHA-256 over the kernel sources and their build recipe: what a stored
    profile (profiles/rNN/*.json) records and bench.py compares, so that counters measured on one build are
    never quoted for another."""
    import hashlib
    h = hashlib.sha256()
    csrc = os.path.join(_HERE, "csrc")
    names = ["hmgrid.hip", "longgrid.hip", "longgrid.hpp", "rowdev.hpp", "sici.hpp", "ldsfft.hpp", "fastmath.hpp", "Makefile",
             "lensing.hip", "j0.hpp", "j1.hpp", "ksz.hip", "realspace.hip", "j01.hpp", "trispectrum.hip", "bispectrum.hip",
             "response.hip", "gasproj.hip", "i0e.hpp", "rsd.hip", "gauss_moments.hpp", "onepoint.hip",
             "hodens.hip", "hankel.hip", "angcov.hip", "clusters.hip", "cib.hip", "curvedsky.hip", "nonlimber.hip", "sphbessel.hpp"]
    names += sorted(os.path.join("kernels", n) for n in os.listdir(os.path.join(csrc, "kernels")) if n.endswith(".hpp"))
    for name in names:          # (runtime.hip / comm.hip / hmctx.hpp hold no device code: not part of the kernel identity)
        with open(os.path.join(csrc, name), "rb") as f:
            h.update(f.read())
    return h.hexdigest()[:16]


def load():
    """Load libhmgrid.so once; raise loudly if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: the HIP extension is not built and there is no CPU "
            "fallback. Run `make -C hmvec_amd/csrc` (needs hipcc, --offload-arch=gfx950).")
    lib = C.CDLL(LIB_PATH)
    for name, argtypes in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the ABI drifted
        fn.argtypes = argtypes
        fn.restype = C.c_int
    lib.hmg_last_error.argtypes = []
    lib.hmg_last_error.restype = C.c_char_p
    if lib.hmg_abi_version() != ABI_VERSION:
        raise ImportError(f"libhmgrid ABI {lib.hmg_abi_version()} != binding {ABI_VERSION}")
    _lib = lib
    return lib


def check(rc):
    if rc != 0:
        raise NativeError(load().hmg_last_error().decode("utf-8", "replace"))


class DeviceArray:
    """A C-contiguous fp64 array living in HBM, owned by a Context."""

    __slots__ = ("ctx", "ptr", "shape", "_owner", "__weakref__")

    def __init__(self, ctx, ptr, shape, owner=True):
        self.ctx, self.ptr, self.shape, self._owner = ctx, ptr, tuple(int(s) for s in shape), owner

    @property
    def size(self):
        n = 1
        for s in self.shape:
            n *= s
        return n

    @property
    def nbytes(self):
        return self.size * 8

    def numpy(self):
        self.ctx.flush()
        out = np.empty(self.shape, dtype=np.float64)
        check(self.ctx.lib.hmg_memcpy_d2h(self.ctx.handle, out.ctypes.data, self.ptr, self.nbytes))
        return out

    def view(self, offset_elems, shape):
        """Non-owning window into this buffer (e.g. a z-slab)."""
        v = DeviceArray(self.ctx, self.ptr + 8 * int(offset_elems), shape, owner=False)
        v._owner = self  # keep parent alive
        return v

    def free(self):
        """Hand the block back to the context's free list (no device synchronisation).  The free list's
        invariant - whatever still touches a freed block was enqueued earlier on the same stream - only holds
        for work that HAS been enqueued.  Deferred stages hold raw addresses, so their owner must keep every
        array they refer to alive until the queue is issued: HaloModel keeps them in its buffer pool and input
        cache and issues the queue before it releases or replaces an entry of either (HaloModel._buf,
        HaloModel._release_inputs).  Flushing here instead would issue the queue whenever any unrelated temporary
        goes out of scope and split the grouped launches."""
        if self._owner is True and self.ptr and self.ctx is not None and self.ctx.handle:
            self.ctx.lib.hmg_free(self.ctx.handle, self.ptr)
        self.ptr = 0

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class PinnedArray:
    """Page-locked host block viewed as a numpy array: the destination of asynchronous D2H copies
    (hmg_memcpy_d2h_async).  Owns the block; numpy views into it keep this object alive through
    ``.base``."""

    def __init__(self, ctx, shape):
        self.ctx = ctx
        shape = (shape,) if np.isscalar(shape) else tuple(int(s) for s in shape)
        n = int(np.prod(shape)) if shape else 1
        p = C.c_void_p()
        check(ctx.lib.hmg_host_alloc(ctx.handle, n * 8, C.byref(p)))
        self.ptr = p.value
        buf = (C.c_double * n).from_address(self.ptr)
        buf._hmg_owner = self                     # the ctypes buffer is numpy's base object
        self.array = np.frombuffer(buf, dtype=np.float64).reshape(shape)

    def __del__(self):
        try:
            if self.ptr and self.ctx.handle:
                self.ctx.lib.hmg_host_free(self.ctx.handle, self.ptr)
            self.ptr = 0
        except Exception:
            pass


class Context:
    """One per GPU / process: stream, scratch, rocFFT plans, RCCL communicator."""

    def __init__(self, device=0):
        self.lib = load()
        h = C.c_void_p()
        check(self.lib.hmg_ctx_create(int(device), C.byref(h)))
        self.handle = h.value
        self.device = int(device)
        self.capture_serial = 0       # changes at every capture begin/end: events recorded before are off limits
        self._deferred = []           # objects with stages queued for a grouped launch (HaloModel), in order
        self._trace = None            # list of (name, args) while Context.trace records a launch-only sequence
        self.shared = {}              # id(read-only host array) -> (array, device copies ...): inputs several models share

    # deferred stages: a HaloModel queues the launch-only stages of a pass so that independent ones can
    # share a launch (hmg_group_*); ANY other native call of this context issues them first, so program
    # order is what every consumer sees
    def defer(self, owner):
        if owner not in self._deferred:
            self._deferred.append(owner)

    def flush(self):
        while self._deferred:
            self._deferred.pop(0)._flush()

    def call_now(self, name, *args):
        """A native call that does not flush the deferred stages (used while they are being issued).  Every
        stream-affecting native call of this class goes through here, so that a recorded call list
        (Context.trace) keeps lane switches, event records/waits and copies exactly as a capture does."""
        if self._trace is not None:
            self._trace.append((name, args))
        check(getattr(self.lib, name)(self.handle, *args))

    # call lists: the native calls of a launch-only sequence (a pass), recorded once and re-issued without the
    # Python facade in between - what a step that cannot be a HIP graph (event records with timestamps) uses so
    # that the host stays ahead of a 0.1 ms pass.  Same restrictions as a capture: same buffers, no allocation.
    def trace(self, fn):
        self.flush()
        self._trace = []
        try:
            fn()
            self.flush()
            return self._trace
        finally:
            self._trace = None

    def run_trace(self, calls):
        self.flush()
        lib, h = self.lib, self.handle
        for name, args in calls:
            check(getattr(lib, name)(h, *args))

    def close(self):
        self.shared = {}
        if getattr(self, "handle", None):
            self.lib.hmg_ctx_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # memory
    def empty(self, shape):
        shape = (int(shape),) if isinstance(shape, (int, np.integer)) else tuple(int(v) for v in shape)
        n = math.prod(shape)                     # (np.prod costs 3 us per call; a model makes ~60 of these)
        p = C.c_void_p()
        check(self.lib.hmg_malloc(self.handle, n * 8, C.byref(p)))
        return DeviceArray(self, p.value, shape)

    def upload(self, arr):
        a = np.ascontiguousarray(arr, dtype=np.float64)
        d = self.empty(a.shape)          # (a recycled block: its last owner released it, and owners of queued
                                         # stages issue the queue before they release anything - DeviceArray.free)
        check(self.lib.hmg_memcpy_h2d(self.handle, d.ptr, a.ctypes.data, a.nbytes))
        return d

    def upload_int32(self, arr):
        """A host integer array as 32-bit ints on the device: a DeviceArray whose block holds them packed (two per fp64
        slot; its shape counts slots, not ints)."""
        a = np.ascontiguousarray(arr, dtype=np.int32)
        d = self.empty(((a.size + 1) // 2,))
        check(self.lib.hmg_memcpy_h2d(self.handle, d.ptr, a.ctypes.data, a.nbytes))
        return d

    def write(self, dst, arr):
        """Overwrite DeviceArray ``dst`` with a host array (stream-ordered behind everything queued so far)."""
        self.flush()
        a = np.ascontiguousarray(arr, dtype=np.float64)
        if self._trace is not None:
            raise NativeError("Context.write inside Context.trace: a recorded call list cannot own host data")
        check(self.lib.hmg_memcpy_h2d(self.handle, dst.ptr, a.ctypes.data, a.nbytes))

    def copy(self, src):
        self.flush()
        d = self.empty(src.shape)
        self.call_now("hmg_memcpy_d2d", d.ptr, src.ptr, src.nbytes)
        return d

    def sync(self):
        self.flush()
        check(self.lib.hmg_sync(self.handle))

    def record(self, slot):
        self.call("hmg_event_record", slot)

    def lane(self, i):
        """Route subsequent launches to lane i (0 = main stream)."""
        self.call("hmg_lane_set", i)

    def wait(self, slot):
        """Current lane waits for the event last recorded in `slot`."""
        self.call("hmg_event_wait", slot)

    def elapsed_ms(self, s0, s1):
        ms = C.c_double()
        check(self.lib.hmg_elapsed_ms(self.handle, s0, s1, C.byref(ms)))
        return ms.value

    _NO_FLUSH = frozenset(["hmg_bracket_next", "hmg_profile_support_epoch", "hmg_prefix_deferral"])      # calls that enqueue nothing and read nothing

    def call(self, name, *args, **kw):
        """A native call behind the deferred stages.  Keywords are placed by the header's parameter names (arguments)."""
        if kw:
            args = arguments(name, args, kw)
        if name not in self._NO_FLUSH:
            self.flush()
        if self._trace is not None:
            self._trace.append((name, args))
        check(getattr(self.lib, name)(self.handle, *args))

    # captured steps
    def capture(self, fn):
        """Run ``fn()`` (launch-only: no allocation, upload, download or synchronisation) inside a
        HIP-graph capture and return the graph id for ``replay``."""
        self.flush()                      # stages queued before the capture are not part of it
        check(self.lib.hmg_graph_begin(self.handle))
        self.capture_serial += 1
        try:
            fn()
            self.flush()                  # ... and those queued inside it are
        except BaseException:
            for o in self._deferred:       # whatever was queued inside the failed capture is dropped with it
                o._drop_queue()
            self._deferred.clear()
            self.lib.hmg_graph_abort(self.handle)
            self.capture_serial += 1
            raise
        gid = C.c_int()
        try:
            check(self.lib.hmg_graph_end(self.handle, C.byref(gid)))
        finally:
            self.capture_serial += 1
        return gid.value

    def graph_kernel_nodes(self, gid):
        """Kernel launches the captured step `gid` holds."""
        n = C.c_int()
        check(self.lib.hmg_graph_kernel_nodes(self.handle, gid, C.byref(n)))
        return n.value

    def replay(self, gid):
        self.call("hmg_graph_launch", gid)

    def copy_to_pinned(self, pinned, src):
        """Asynchronous D2H of DeviceArray ``src`` into PinnedArray ``pinned`` on the current lane."""
        self.call("hmg_memcpy_d2h_async", pinned.ptr, src.ptr, src.nbytes)

    def copy_from_pinned(self, dst, pinned):
        """Asynchronous H2D of PinnedArray ``pinned`` into DeviceArray ``dst`` on the current lane."""
        self.call("hmg_memcpy_h2d_async", dst.ptr, pinned.ptr, dst.nbytes)

    def event_synchronize(self, slot):
        """Block the host until the event last recorded in ``slot`` has happened (other work keeps running)."""
        check(self.lib.hmg_event_synchronize(self.handle, slot))


_default_ctx = {}


def default_context(device=0):
    """Process-wide shared Context per device (streams, scratch, FFT tables are reused by
    every HaloModel that is not given its own)."""
    c = _default_ctx.get(device)
    if c is None or not c.handle:
        c = _default_ctx[device] = Context(device)
    return c


def context_or_default(ctx):
    return default_context(0) if ctx is None else ctx


def as_device(ctx, a):
    """A DeviceArray as it is (resident model data), anything else uploaded."""
    return a if isinstance(a, DeviceArray) else ctx.upload(np.ascontiguousarray(a, dtype=np.float64))


def ptr(x):
    """Device pointer of a DeviceArray or NULL."""
    return None if x is None else x.ptr
