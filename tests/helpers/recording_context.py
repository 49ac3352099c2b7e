"""A stand-in for the native library that records calls instead of making them, so that the Python facade can be
run - and its native call sequence read - without a GPU.

``recording_context()`` is a real ``_native.Context`` (made with ``__new__``: no library is loaded) whose ``lib`` is a
``RecordingLib``: every attribute is a function that logs (entry name, arguments) and returns 0.  Four entries also
do something, since the facade reads their output: hmg_malloc / hmg_host_alloc hand out addresses from a counter,
hmg_sigma2_layout_size writes a size, hmg_prefix_pending writes 0, hmg_memcpy_d2h zero-fills."""
import ctypes as C

import numpy as np

ZS = np.array([0.1, 0.5, 1.0])
KS = np.geomspace(1e-3, 10, 96)
MS = np.geomspace(1e11, 1e15, 48)
PAIRS = [("nfw", "nfw"), ("g", "electron"), ("y", "y")]


class RecordingLib:
    def __init__(self, render=None):
        self.calls = []                 # (entry name, arguments as passed, the context handle included) in call order
        self._next = 0x10000
        self._render = render or (lambda name, args: args)      # what to keep of the arguments, decided at call time

    def __getattr__(self, name):
        def entry(*args):
            if name in ("hmg_malloc", "hmg_host_alloc"):
                args[2]._obj.value = self._next
                self._next += (args[1] + 255) // 256 * 256 + 256
            elif name == "hmg_sigma2_layout_size":
                args[2]._obj.value = args[0] * args[1] * 2
            elif name == "hmg_prefix_pending":
                args[2]._obj.value = 0
            elif name == "hmg_memcpy_d2h":
                C.memset(args[1], 0, args[3])
            self.calls.append((name, self._render(name, args)))
            return 0
        return entry

    def names(self, start=0):
        return [name for name, _ in self.calls[start:]]


def recording_context(render=None):
    from hmvec_amd import _native as nat
    ctx = nat.Context.__new__(nat.Context)
    ctx.lib, ctx.handle, ctx.device = RecordingLib(render), 1, 0
    ctx.capture_serial, ctx._deferred, ctx._trace, ctx.shared = 0, [], None, {}
    return ctx


def build_model(ctx, zs=ZS, ks=KS, ms=MS, **kw):
    """The model of the facade checks: constructor (mass function + NFW), gas, pressure, HOD, one batch of spectra."""
    import hmvec_amd as hm
    h = hm.HaloModel(zs, ks, ms=ms, accuracy="low", engine="analytic", ctx=ctx, **kw)
    h.add_battaglia_profile("electron")
    h.add_battaglia_pres_profile("y")
    h.add_hod("g", mthresh=np.full(zs.size, 10 ** 10.5))
    h.power_device_batch(PAIRS)
    return h


def second_pass(h, ms=MS, numeric=False):
    """The steady state: every stage again on a model that exists, launch-only, then the spectra."""
    h.init_mass_function(ms)
    h.add_nfw_profile("nfw", numeric=numeric, ignore_existing=True)
    h.add_battaglia_profile("electron", ignore_existing=True)
    h.add_battaglia_pres_profile("y", ignore_existing=True)
    h.add_hod("g", mthresh=np.full(h.zs.size, 10 ** 10.5), ignore_existing=True)
    return h.power_device_batch(PAIRS)
