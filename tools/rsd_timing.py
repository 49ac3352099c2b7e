#!/usr/bin/env python3
"""Device time of the redshift-space wedges and multipoles (hmg_rsd_wedges, hmg_rsd_multipoles) on
GPU 0: the pair ("g", "g") on the Config-3 grid (nz 32 x nm 512 x nk 4096) at all 4096 nodes of ks, the wedges at the 16
nodes of rsd.mu_rule(16), the multipoles with that rule, and - the yardstick - one pass of the one-pair mass integrals
(hmg_power) over the same tensor in the same run.  The model is built once and the tables are uploaded once; each call is
repeated --warmup times, then timed --reps times between event records on the context's stream.  A window holds ONE
call: both entry points wait on the host for their table check, so that wait (a few tens of microseconds) is inside the
window, as it is for every caller.  Prints one JSON line (median and minimum milliseconds) and, with --resources, the
resource table of the units (tools/kernel_resources.py).

Usage:  python tools/rsd_timing.py [--reps 20] [--warmup 3] [--nmu 16] [--pair g g] [--resources]"""
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
from hmvec_amd import rsd  # noqa: E402

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
    ap.add_argument("--nmu", type=int, default=16)
    ap.add_argument("--pair", nargs=2, default=["g", "g"])
    ap.add_argument("--resources", action="store_true")
    a = ap.parse_args()
    nz, nm, nk, nmu = 32, 512, 4096, a.nmu
    zs, ms, ks = np.linspace(0.01, 3.0, nz), np.geomspace(2e10, 1e17, nm), np.geomspace(1e-4, 100, nk)
    h = hm.HaloModel(zs, ks, ms=ms, accuracy="low", engine="analytic")
    h.add_hod("g", mthresh=10 ** 10.5 + zs * 0.0)
    ctx = h._main(needs_aux=True)
    recs, (kindex, damp, sigma_s, f), alphas = h._rsd_request(a.pair[0], a.pair[1], None, None, None, (1, 0, 1), True)
    n = kindex.size
    ta, tb = (h._tracer(r, 1) for r in recs)
    mus, _ = rsd.mu_rule(nmu)
    d_k, d_damp, d_sig, d_f = ctx.upload_int32(kindex), ctx.upload(damp), ctx.upload(sigma_s), ctx.upload(f)
    d_mus, d_wl = ctx.upload(np.ascontiguousarray(mus)), ctx.upload(rsd.legendre_weights(nmu))
    W, M, p1 = ctx.empty((2, nz, n, nmu)), ctx.empty((2, nz, n, 3)), ctx.empty((nz, nk))
    tm_ = h._tracer(h._resolve("nfw")[0], 1)
    common = (h._d_nzm.ptr, h._d_bh.ptr, h._d_ms().ptr, h._d_wm().ptr, h._d_ks().ptr, h._d_Pzk().ptr, h._rho_m0(), d_k.ptr,
              d_damp.ptr, d_mus.ptr)

    def wedges():
        ctx.call("hmg_rsd_wedges", nz, nm, nk, n, nmu, C.byref(ta), C.byref(tb), *common, d_sig.ptr, d_f.ptr, *alphas, W.ptr,
                 None)

    def multipoles():
        ctx.call("hmg_rsd_multipoles", nz, nm, nk, n, nmu, C.byref(ta), C.byref(tb), *common, d_wl.ptr, d_sig.ptr, d_f.ptr,
                 *alphas, M.ptr, None)

    def power():
        ctx.call("hmg_power", nz, nm, nk, C.byref(tm_), C.byref(tm_), h._d_nzm.ptr, h._d_bh.ptr, h._d_ms().ptr,
                 h._d_wm().ptr, h._d_ks().ptr, h._d_Pzk().ptr, h._rho_m0(), float(h.p["kstar_damping"]), p1.ptr, None)

    res = {"grid": [nz, nm, nk], "n": n, "nmu": nmu, "pair": "-".join(a.pair),
           "rsd_wedges": timed(ctx, a.reps, a.warmup, wedges),
           "rsd_multipoles": timed(ctx, a.reps, a.warmup, multipoles),
           "power_1h_nfw_nfw": timed(ctx, a.reps, a.warmup, power),
           "tensor_bytes": nz * nm * nk * 8}
    w, m = W.numpy(), M.numpy()
    assert np.all(np.isfinite(w)) and np.all(np.isfinite(m))
    # the rule's sum of the 2-halo wedge is the 2-halo multipole the device formed from the same nodes
    quad = np.einsum("lq,zsq->zsl", rsd.legendre_weights(nmu), w[1])
    scale = np.einsum("lq,zsq->zsl", np.abs(rsd.legendre_weights(nmu)), np.abs(w[1]))
    res["max_2h_rule_mismatch_eps"] = float(np.max(np.abs(quad - m[1]) / scale) / 2.0 ** -52)
    res["kx_max"] = float(ks.max() * sigma_s.max())
    res["kernel_source_sha16"] = nat.kernel_source_sha16()
    print(json.dumps(res))
    if a.resources:
        sys.stdout.flush()
        subprocess.run([sys.executable, os.path.join(HERE, "tools", "kernel_resources.py")], check=True)


if __name__ == "__main__":
    main()
