#!/usr/bin/env python3
"""Device time of the 1-halo trispectrum (hmg_trispectrum_1h) on GPU 0: T of ("g", "nfw") with itself
on the Config-3 grid (nz 32 x nm 512 x nk 4096) at n = 256 log-spaced nodes of ks, next to one pass of the one-pair mass
integrals (hmg_power) over the same two tensors.  The model is built once and the tables are uploaded once; each call is
repeated --warmup times, then timed --reps times between event records on the context's stream.  A window holds ONE
call of the trispectrum: the entry point waits on the host for its table check, so that wait (a few tens of
microseconds) is inside the window, as it is for every caller.  Prints one JSON line (median and minimum milliseconds,
the bytes the loader asks for) and, with --resources, the resource table of the unit (tools/kernel_resources.py).

Usage:  python tools/trispectrum_timing.py [--reps 20] [--warmup 3] [--n 256] [--resources]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)

import hmvec_amd as hm  # noqa: E402
from hmvec_amd import _native as nat  # noqa: E402

SLOT0 = 100       # event slots clear of HaloModel's (0-3) and bench.py's (40 and up)


def timed(ctx, reps, warmup, fn):
    for _ in range(warmup):
        fn()
    ctx.sync()
    ms = []
    for _ in range(reps):
        ctx.record(SLOT0)
        fn()
        ctx.record(SLOT0 + 1)
        ctx.sync()
        ms.append(ctx.elapsed_ms(SLOT0, SLOT0 + 1))
    return dict(median_ms=float(np.median(ms)), min_ms=float(np.min(ms)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--resources", action="store_true")
    a = ap.parse_args()
    nz, nm, nk, n = 32, 512, 4096, a.n
    zs, ms, ks = np.linspace(0.01, 3.0, nz), np.geomspace(2e10, 1e17, nm), np.geomspace(1e-4, 100, nk)
    h = hm.HaloModel(zs, ks, ms=ms, accuracy="low", engine="analytic")
    h.add_hod("g", mthresh=10 ** 10.5 + zs * 0.0)
    ctx = h._main(needs_aux=True)
    kindex = np.linspace(0, nk - 1, n).round().astype(int)            # ks is a geomspace: log-spaced nodes
    idx, frac, scale = h._trispectrum_tables(kindex, None, None, None, True)
    tg, tm_ = (h._tracer(r, 1) for r in h._resolve("g", "nfw"))
    d_idx, d_frac, d_scale = ctx.upload_int32(idx), ctx.upload(frac), ctx.upload(scale)
    T, p1 = ctx.empty((nz, n, n)), ctx.empty((nz, nk))
    common = (h._d_nzm.ptr, h._d_ms().ptr, h._d_wm().ptr, h._rho_m0())

    def tri():
        ctx.call("hmg_trispectrum_1h", nz, nm, nk, n, C.byref(tg), C.byref(tm_), C.byref(tg), C.byref(tm_), *common,
                 d_idx.ptr, d_frac.ptr, d_scale.ptr, None, T.ptr, None)

    def power():
        ctx.call("hmg_power", nz, nm, nk, C.byref(tg), C.byref(tm_), h._d_nzm.ptr, h._d_bh.ptr, h._d_ms().ptr,
                 h._d_wm().ptr, h._d_ks().ptr, h._d_Pzk().ptr, h._rho_m0(), float(h.p["kstar_damping"]), p1.ptr, None)

    tiles = (n - 1) // 64 + 1
    res = {"grid": [nz, nm, nk], "n": n,
           "trispectrum_g_nfw": timed(ctx, a.reps, a.warmup, tri),
           "power_1h_g_nfw": timed(ctx, a.reps, a.warmup, power),
           # one tensor (g's satellite profile is nfw itself), one node per sample, both sides of every tile
           "loader_requested_bytes": nz * tiles * tiles * nm * 2 * 64 * 8,
           "tensor_bytes": nz * nm * nk * 8}
    got = T.numpy()
    assert np.all(np.isfinite(got)) and np.all(got >= 0) and np.array_equal(got, got.transpose(0, 2, 1))
    res["kernel_source_sha16"] = nat.kernel_source_sha16()
    print(json.dumps(res))
    if a.resources:
        sys.stdout.flush()
        subprocess.run([sys.executable, os.path.join(HERE, "tools", "kernel_resources.py")], check=True)


if __name__ == "__main__":
    main()
