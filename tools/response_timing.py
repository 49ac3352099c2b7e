#!/usr/bin/env python3
"""Device time of the response and the super-sample contraction (hmg_response, hmg_ssc) on GPU 0:
R of the six pairs of ("nfw", "g", "y") on the Config-3 grid (nz 32 x nm 512 x nk 4096) at n = 256 log-spaced nodes of
ks, the contraction of those responses into the (6 * 256)^2 matrix, and - the yardstick - one pass of the one-pair mass
integrals (hmg_power) over the same tensor in the same run.  The model is built once and the tables are uploaded once;
each call is repeated --warmup times, then timed --reps times between event records on the context's stream.  A window
holds ONE call: hmg_response waits on the host for its table check, so that wait (a few tens of microseconds) is inside
its window, as it is for every caller.  Prints one JSON line (median and minimum milliseconds) and, with --resources,
the resource table of the units (tools/kernel_resources.py).

Usage:  python tools/response_timing.py [--reps 20] [--warmup 3] [--n 256] [--resources]"""
import argparse
import ctypes as C
import itertools
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)

import hmvec_amd as hm  # noqa: E402
from hmvec_amd import _native as nat  # noqa: E402
from hmvec_amd import cov  # noqa: E402

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
    h.add_battaglia_pres_profile("y", family="pres", xmax=5, nxs=512)
    h.add_hod("g", mthresh=10 ** 10.5 + zs * 0.0)
    ctx = h._main(needs_aux=True)
    pairs = list(itertools.combinations_with_replacement(("nfw", "g", "y"), 2))
    npairs = len(pairs)
    kindex = np.linspace(0, nk - 1, n).round().astype(int)            # ks is a geomspace: log-spaced nodes
    _, recs, (idx, frac, scale) = h._response_request(pairs, kindex, None, None, None)
    tr = (nat.Tracer * len(recs))(*[h._tracer(r, 1) for r in recs])
    d_idx, d_frac, d_scale = ctx.upload_int32(idx), ctx.upload(frac), ctx.upload(scale)
    d_dlnP, d_g = ctx.upload(cov.dlnp_table(h.ks, h.Pzk)), ctx.upload(np.full(nz, 1.0 / nz))
    R, covm, p1 = ctx.empty((npairs, nz, n)), ctx.empty((npairs, n, npairs, n)), ctx.empty((nz, nk))
    tm_ = h._tracer(h._resolve("nfw")[0], 1)

    def response():
        ctx.call("hmg_response", nz, nm, nk, n, npairs, tr, h._d_nzm.ptr, h._d_bh.ptr, h._d_ms().ptr, h._d_wm().ptr,
                 h._d_ks().ptr, h._d_Pzk().ptr, d_dlnP.ptr, h._rho_m0(), float(h.p["kstar_damping"]), d_idx.ptr,
                 d_frac.ptr, d_scale.ptr, R.ptr, None)

    def ssc():
        ctx.call("hmg_ssc", nz, n, npairs, R.ptr, None, d_g.ptr, covm.ptr)

    def power():
        ctx.call("hmg_power", nz, nm, nk, C.byref(tm_), C.byref(tm_), h._d_nzm.ptr, h._d_bh.ptr, h._d_ms().ptr,
                 h._d_wm().ptr, h._d_ks().ptr, h._d_Pzk().ptr, h._rho_m0(), float(h.p["kstar_damping"]), p1.ptr, None)

    res = {"grid": [nz, nm, nk], "n": n, "pairs": ["-".join(p) for p in pairs],
           "response_6_pairs": timed(ctx, a.reps, a.warmup, response),
           "ssc_6_pairs": timed(ctx, a.reps, a.warmup, ssc),
           "power_1h_nfw_nfw": timed(ctx, a.reps, a.warmup, power),
           "tensor_bytes": nz * nm * nk * 8}
    got, c = R.numpy(), covm.numpy()
    assert np.all(np.isfinite(got)) and np.all(np.isfinite(c)) and np.array_equal(c, c.transpose(2, 3, 0, 1))
    res["kernel_source_sha16"] = nat.kernel_source_sha16()
    print(json.dumps(res))
    if a.resources:
        sys.stdout.flush()
        subprocess.run([sys.executable, os.path.join(HERE, "tools", "kernel_resources.py")], check=True)


if __name__ == "__main__":
    main()
