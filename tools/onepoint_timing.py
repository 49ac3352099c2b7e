#!/usr/bin/env python3
"""Device time of the one-point contractions (hmg_onepoint_exponent, hmg_onepoint_moments) on GPU 0:
the Compton-y rings of every halo of the Config-3 grid (nz 32 x nm 512) with --ntheta rings each (default 64), contracted
at nlambda = 513 and 2049 (PDFs of 1024 and 4096 bins), and - the yardstick - one pass of the one-pair mass integrals
(hmg_power) over the Config-3 tensor in the same run.  The model is built once and the rings are evaluated once on the
device; each call is repeated --warmup times, then timed --reps times between event records on the context's stream.
get_y_pdf is timed end to end on the host's clock, the profiles' evaluation, the uploads, the fetch and the transform
included.  Prints one JSON line (median, minimum and maximum milliseconds; sine/cosine pairs per second).

Usage:  python tools/onepoint_timing.py [--reps 20] [--warmup 3] [--ntheta 64]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)

import hmvec_amd as hm  # noqa: E402
from hmvec_amd import _native as nat  # noqa: E402
from hmvec_amd import onepoint  # noqa: E402
from hmvec_amd.gasprofiles import projected_gnfw_device  # noqa: E402

SLOT0 = 100       # event slots clear of HaloModel's (0-3) and bench.py's (40 and up)


def spread(ms):
    return dict(median_ms=float(np.median(ms)), min_ms=float(np.min(ms)), max_ms=float(np.max(ms)))


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
    return spread(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ntheta", type=int, default=64)
    a = ap.parse_args()
    nz, nm, nk, nt = 32, 512, 4096, a.ntheta
    zs, ms, ks = np.linspace(0.01, 3.0, nz), np.geomspace(2e10, 1e17, nm), np.geomspace(1e-4, 100, nk)
    h = hm.HaloModel(zs, ks, ms=ms, accuracy="low", engine="analytic")
    ctx = h._main(needs_aux=True)
    req = h._y_request(1.0, None, None, None, nt, None, None, None)
    d_y = projected_gnfw_device(*req["proj"], ctx=ctx)
    d_area, d_amp, d_zw = ctx.upload(req["area"]), ctx.upload(req["amp"]), ctx.upload(req["zw"])
    k = h.get_y_cumulants(ntheta=nt)
    res = {"grid": [nz, nm, nt], "cumulants": [float(v) for v in k]}
    inputs = (nz, nm, nt, d_y.ptr, d_area.ptr, d_amp.ptr, h._d_nzm.ptr, h._d_wm().ptr, d_zw.ptr, 0, nm)
    for nbins in (1024, 4096):
        dy = np.sqrt(k[1]) / 10.0
        nl, dl = onepoint.lambda_grid(nbins, dy)
        rows, total = ctx.empty((nz, 2, nl)), ctx.empty((2, nl))
        r = timed(ctx, a.reps, a.warmup, lambda: ctx.call("hmg_onepoint_exponent", *inputs, nl, dl, rows.ptr, total.ptr))
        r["pairs_per_s"] = nz * nm * nt * (nl - 1) / (r["median_ms"] * 1e-3)
        assert np.all(np.isfinite(total.numpy()))
        res[f"exponent_nlambda_{nl}"] = r
    K, Ks = ctx.empty((nz, 4)), ctx.empty((4,))
    res["moments"] = timed(ctx, a.reps, a.warmup, lambda: ctx.call("hmg_onepoint_moments", *inputs, K.ptr, Ks.ptr))
    tm_ = h._tracer(h._resolve("nfw")[0], 1)
    p1 = ctx.empty((nz, nk))
    res["power_1h_nfw_nfw"] = timed(ctx, a.reps, a.warmup, lambda: ctx.call(
        "hmg_power", nz, nm, nk, C.byref(tm_), C.byref(tm_), h._d_nzm.ptr, h._d_bh.ptr, h._d_ms().ptr, h._d_wm().ptr,
        h._d_ks().ptr, h._d_Pzk().ptr, h._rho_m0(), float(h.p["kstar_damping"]), p1.ptr, None))
    for nbins in (1024, 4096):
        dy = np.sqrt(k[1]) / 10.0
        wall = []
        for i in range(a.warmup + a.reps):
            ctx.sync()
            t0 = time.perf_counter()
            ys, p = h.get_y_pdf(nbins, dy, ymin=k[0] - 100 * dy, noise_sigma=3 * dy, ntheta=nt)
            if i >= a.warmup:
                wall.append(1e3 * (time.perf_counter() - t0))
        res[f"get_y_pdf_{nbins}_bins_wall"] = spread(wall)
        res[f"get_y_pdf_{nbins}_bins_sum"] = float(p.sum())
    res["kernel_source_sha16"] = nat.kernel_source_sha16()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
