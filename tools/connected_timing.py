#!/usr/bin/env python3
"""Device time of the 2-, 3- and 4-halo terms of the trispectrum (hmg_trispectrum_connected) on GPU 0:
the five terms of ("nfw", "nfw" | "nfw", "nfw") and of ("g", "nfw" | "g", "nfw") on the Config-3 grid (nz 32 x nm 512 x
nk 4096) at n = 256 log-spaced nodes of ks with a 32-node rule, next to the PT averages alone (hmg_pt_averages), one pass
of the one-pair mass integrals (hmg_power) over the same tensors, and the numpy restatement of the contract
(tests/helpers/connected_model.py, wall time of one call on the host, at --n-host samples and --nz-host redshifts: it is
not written for speed).  The model is built once and the tables are uploaded once; each call is repeated --warmup times,
then timed --reps times between event records on the context's stream.  A window holds ONE call: the entry point waits
on the host for its table checks (its own and the 1-halo entry point's), so those waits are inside the window, as they
are for every caller.  Prints one JSON line and, with --resources, the resource table (tools/kernel_resources.py).

Usage:  python tools/connected_timing.py [--reps 10] [--warmup 2] [--n 256] [--nr 32] [--resources]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "tests", "helpers"))

import hmvec_amd as hm  # noqa: E402
from hmvec_amd import _native as nat  # noqa: E402
from hmvec_amd import connected as cn  # noqa: E402

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
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--nr", type=int, default=32)
    ap.add_argument("--n-host", type=int, default=32)
    ap.add_argument("--nz-host", type=int, default=1)
    ap.add_argument("--resources", action="store_true")
    a = ap.parse_args()
    nz, nm, nk, n = 32, 512, 4096, a.n
    zs, ms, ks = np.linspace(0.01, 3.0, nz), np.geomspace(2e10, 1e17, nm), np.geomspace(1e-4, 100, nk)
    h = hm.HaloModel(zs, ks, ms=ms, accuracy="low", engine="analytic")
    h.add_hod("g", mthresh=10 ** 10.5 + zs * 0.0)
    ctx = h._main(needs_aux=True)
    rule = cn.angle_rule(a.nr, "2d")
    kindex = np.linspace(0, nk - 1, n).round().astype(int)            # ks is a geomspace: log-spaced nodes
    idx, frac, scale = h._sample_tables(kindex, None, None, None, False, 256, "the connected trispectrum")
    scale1h = h._sample_tables(kindex, None, None, None, True, 256, "the connected trispectrum")[2]
    tg, tm_ = (h._tracer(r, 1) for r in h._resolve("g", "nfw"))
    d_idx, d_frac, d_scale, d_s1 = ctx.upload_int32(idx), ctx.upload(frac), ctx.upload(scale), ctx.upload(scale1h)
    d_rule = [ctx.upload(v) for v in (rule.mu, rule.one_minus_mu, rule.one_plus_mu, rule.weights)]
    T, pt, p1 = ctx.empty((5, nz, n, n)), ctx.empty((3, nz, n, n)), ctx.empty((nz, nk))
    block = h._model_block("hmg_trispectrum_connected")
    kstar = float(h.p["kstar_damping"])

    def connected(ta, tb):
        def call():
            ctx.call("hmg_trispectrum_connected", nz=nz, nm=nm, nk=nk, n=n, nr=rule.nr, h_a=C.byref(ta), h_b=C.byref(tb),
                     h_c=C.byref(ta), h_d=C.byref(tb), **block, kstar=kstar, d_idx=d_idx.ptr, d_frac=d_frac.ptr,
                     d_scale=d_scale.ptr, d_scale1h=d_s1.ptr, d_mu=d_rule[0].ptr, d_omm=d_rule[1].ptr, d_opm=d_rule[2].ptr,
                     d_w=d_rule[3].ptr, d_zweights=None, d_T=T.ptr, d_Tz=None)
        return call

    def averages():
        plane = 8 * nz * n * n
        ctx.call("hmg_pt_averages", nz, nk, n, rule.nr, h._d_ks().ptr, h._d_Pzk().ptr, d_idx.ptr, d_frac.ptr,
                 *(v.ptr for v in d_rule), pt.ptr, pt.ptr + plane, pt.ptr + 2 * plane)

    def power():
        ctx.call("hmg_power", nz, nm, nk, C.byref(tg), C.byref(tm_), h._d_nzm.ptr, h._d_bh.ptr, h._d_ms().ptr,
                 h._d_wm().ptr, h._d_ks().ptr, h._d_Pzk().ptr, h._rho_m0(), kstar, p1.ptr, None)

    res = {"grid": [nz, nm, nk], "n": n, "nr": rule.nr,
           "connected_nfw_nfw_nfw_nfw": timed(ctx, a.reps, a.warmup, connected(tm_, tm_))}
    got = T.numpy()
    assert np.all(np.isfinite(got))
    res["connected_g_nfw_g_nfw"] = timed(ctx, a.reps, a.warmup, connected(tg, tm_))
    got = T.numpy()
    assert np.all(np.isfinite(got))
    res["pt_averages"] = timed(ctx, a.reps, a.warmup, averages)
    res["power_1h_g_nfw"] = timed(ctx, a.reps, a.warmup, power)
    got = pt.numpy()
    assert np.all(np.isfinite(got)) and np.array_equal(got, got.transpose(0, 1, 3, 2))
    # the numpy restatement, on a part of the request
    import connected_model as cm
    sub, zsub = kindex[np.linspace(0, n - 1, a.n_host).round().astype(int)], slice(0, a.nz_host)
    view = cm.view(h, 0, a.nz_host, nm)
    t0 = time.perf_counter()
    cm.connected(view, ("g", "nfw", "g", "nfw"), rule, kindex=sub)
    res["restatement_host"] = dict(wall_s=time.perf_counter() - t0, n=int(sub.size), nz=int(a.nz_host))
    del zsub
    res["kernel_source_sha16"] = nat.kernel_source_sha16()
    print(json.dumps(res))
    if a.resources:
        sys.stdout.flush()
        subprocess.run([sys.executable, os.path.join(HERE, "tools", "kernel_resources.py")], check=True)


if __name__ == "__main__":
    main()
