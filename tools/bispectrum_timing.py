#!/usr/bin/env python3
"""Device time of the halo-model bispectrum (hmg_bispectrum) on GPU 0: B1h, B2h, B3h of
("nfw", "nfw", "nfw") on the Config-3 grid (nz 32 x nm 512 x nk 4096) at n = 64 log-spaced nodes of ks and all closing
i <= j <= l triangles of them, next to one pass of the one-pair mass integrals (hmg_power) over the same tensor.  The
model is built once and the tables are uploaded once; each call is repeated --warmup times, then timed --reps times
between event records on the context's stream.  A window holds ONE call of the bispectrum: the entry point waits on the
host for its table check, so that wait (a few tens of microseconds) is inside the window, as it is for every caller.
Prints one JSON line (median and minimum milliseconds, the number of triangles, the words the loader asks for) and,
with --resources, the resource table of the unit (tools/kernel_resources.py).

Usage:  python tools/bispectrum_timing.py [--reps 20] [--warmup 3] [--n 64] [--resources]"""
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
from hmvec_amd import bispectrum as bs  # noqa: E402

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
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--resources", action="store_true")
    a = ap.parse_args()
    nz, nm, nk, n = 32, 512, 4096, a.n
    zs, ms, ks = np.linspace(0.01, 3.0, nz), np.geomspace(2e10, 1e17, nm), np.geomspace(1e-4, 100, nk)
    h = hm.HaloModel(zs, ks, ms=ms, accuracy="low", engine="analytic")
    ctx = h._main(needs_aux=True)
    kindex = np.linspace(0, nk - 1, n).round().astype(int)            # ks is a geomspace: log-spaced nodes
    idx, frac, scale = h._trispectrum_tables(kindex, None, None, None, False)
    tri = bs.check_triangles(None, bs.sample_wavenumbers(h.ks, idx, frac), zs)
    nt = tri.shape[0]
    t = h._tracer(h._resolve("nfw")[0], 1)
    d_idx, d_frac, d_scale, d_tri = ctx.upload_int32(idx), ctx.upload(frac), ctx.upload(scale), ctx.upload_int32(tri)
    B, p1 = ctx.empty((3, nz, nt)), ctx.empty((nz, nk))

    def bis():
        ctx.call("hmg_bispectrum", nz, nm, nk, n, nt, C.byref(t), C.byref(t), C.byref(t), h._d_nzm.ptr, h._d_bh.ptr,
                 h._d_ms().ptr, h._d_wm().ptr, h._d_ks().ptr, h._d_Pzk().ptr, h._rho_m0(), float(h.p["kstar_damping"]),
                 d_idx.ptr, d_frac.ptr, d_scale.ptr, d_tri.ptr, None, B.ptr, None, None)

    def power():
        ctx.call("hmg_power", nz, nm, nk, C.byref(t), C.byref(t), h._d_nzm.ptr, h._d_bh.ptr, h._d_ms().ptr,
                 h._d_wm().ptr, h._d_ks().ptr, h._d_Pzk().ptr, h._rho_m0(), float(h.p["kstar_damping"]), p1.ptr, None)

    blocks = (nt - 1) // 1024 + 1
    res = {"grid": [nz, nm, nk], "n": n, "triangles": int(nt), "blocks_per_z": blocks,
           "bispectrum_nfw_nfw_nfw": timed(ctx, a.reps, a.warmup, bis),
           "power_1h_nfw_nfw": timed(ctx, a.reps, a.warmup, power),
           # one distinct leg, one node per sample: every workgroup stages n words per mass bin, and so does the one prepass
           "loader_requested_bytes": nz * (blocks + 1) * nm * n * 8,
           "tensor_bytes": nz * nm * nk * 8}
    got = B.numpy()
    assert np.all(np.isfinite(got)) and np.all(got[0] > 0)
    res["kernel_source_sha16"] = nat.kernel_source_sha16()
    print(json.dumps(res))
    if a.resources:
        sys.stdout.flush()
        subprocess.run([sys.executable, os.path.join(HERE, "tools", "kernel_resources.py")], check=True)


if __name__ == "__main__":
    main()
