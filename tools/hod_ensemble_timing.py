#!/usr/bin/env python3
"""Device time of the HOD parameter ensemble (hmg_hod_ensemble, hmg_hod_ensemble_power) on GPU 0
against the loop it replaces, on the Config-3 grid (nz 32 x nm 512 x nk 4096) with "nfw" as both tensors.

For S in --sets (default 16 64 256), on the whole grid and on 64 log-spaced nodes:

  ensemble   HaloModel.hod_ensemble_device(sets, mthresh) - uploads, allocations and, with a kindex, the host's wait for
             the check of the node list included, as every caller pays them;
  loop       per set one add_hod(..., param_override=set, ignore_existing=True) - one hmg_hod - and one batched pass over
             the pairs (g, g) and (g, "nfw") (power_device_batch): the existing methods, unchanged;
  kernel     hmg_hod_ensemble_power alone on a coefficient block that exists (whole grid only: launch-only).

Method: each figure is the time between two event records on the context's stream around a window of repeated calls that
lasts at least --window seconds (default 0.5), after --warmup calls of the same shape; ensemble and loop windows alternate,
--reps times (default 5); median, and spread = (max - min) / median over the repeats.  The kernel's time is put against
its issue bound, 5 S nz nm n FMA at the fp64 vector peak (78.6 TFLOP/s = 39.3e12 FMA/s), and its byte bound, the tensor
once per set tile of 8 at 8 TB/s (HBM peak; tiles that find the tensor in L2 make it beat this bound).  Prints one JSON line.

Usage:  python tools/hod_ensemble_timing.py [--sets 16 64 256] [--reps 5] [--warmup 2] [--window 0.5] [--resources]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)

import hmvec_amd as hm  # noqa: E402
from hmvec_amd import _native as nat  # noqa: E402
from hmvec_amd import hod_ensemble as he  # noqa: E402

SLOT0 = 100       # event slots clear of HaloModel's (0-3) and bench.py's (40 and up)
FMA_PEAK = 39.3e12
HBM_PEAK = 8.0e12


def window_ms(ctx, fn, calls):
    ctx.sync()
    ctx.record(SLOT0)
    for _ in range(calls):
        fn()
    ctx.record(SLOT0 + 1)
    ctx.sync()
    return ctx.elapsed_ms(SLOT0, SLOT0 + 1) / calls


def calls_for(ctx, fn, warmup, window):
    for _ in range(warmup):
        fn()
    once = max(window_ms(ctx, fn, 1), 1e-3)
    return max(1, int(np.ceil(1e3 * window / once)))


def alternate(ctx, fns, reps, warmup, window):
    """{name: (median ms, spread)} of the functions, their windows alternating."""
    calls = {k: calls_for(ctx, f, warmup, window) for k, f in fns.items()}
    ms = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            ms[k].append(window_ms(ctx, f, calls[k]))
    return {k: dict(median_ms=float(np.median(v)), spread=float((np.max(v) - np.min(v)) / np.median(v)), calls=calls[k])
            for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", type=int, nargs="+", default=[16, 64, 256])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--grid", type=int, nargs=3, default=[32, 512, 4096])
    ap.add_argument("--resources", action="store_true")
    a = ap.parse_args()
    nz, nm, nk = a.grid
    zs, ms, ks = np.linspace(0.01, 3.0, nz), np.geomspace(2e10, 1e17, nm), np.geomspace(1e-4, 100, nk)
    h = hm.HaloModel(zs, ks, ms=ms, accuracy="low", engine="analytic")
    mthresh = 10 ** 10.5 + zs * 0.0
    nodes = np.round(np.geomspace(1, nk - 1, 64)).astype(np.int64)          # 64 log-spaced nodes, kept distinct
    for i in range(1, nodes.size):
        nodes[i] = max(nodes[i], nodes[i - 1] + 1)
    assert nodes[-1] <= nk - 1 and np.unique(nodes).size == 64
    ctx = h._main(needs_aux=True)
    res = {"grid": [nz, nm, nk], "tensor_bytes": nz * nm * nk * 8, "nodes": int(nodes.size), "cases": []}
    for S in a.sets:
        t = np.linspace(0.0, 1.0, S)
        sets = hm.hod_sets(sig=0.15 + 0.1 * t, alphasat=0.8 + 0.4 * t, Bsat=7.0 + 5.0 * t, betasat=0.6 + 0.3 * t,
                           Bcut=0.5 + 2.0 * t, betacut=0.4 + 0.4 * t)
        overrides = [{"hod_" + c: float(v) for c, v in zip(sets.columns, row)} for row in sets]

        def loop():
            for ov in overrides:
                h.add_hod("g_loop", mthresh=mthresh, param_override=ov, ignore_existing=True)
                h.power_device_batch([("g_loop", "g_loop"), ("g_loop", "nfw")])

        for what, kidx in (("grid", None), ("nodes", nodes)):
            def ensemble():
                h.hod_ensemble_device(sets, mthresh=mthresh, kindex=kidx)

            case = {"S": S, "columns": what}
            fns = {"ensemble": ensemble}
            if what == "grid":
                fns["loop"] = loop
            case.update(alternate(ctx, fns, a.reps, a.warmup, a.window))
            if what == "grid":
                case["loop_over_ensemble"] = case["loop"]["median_ms"] / case["ensemble"]["median_ms"]
                case["faster_by_more_than_the_spread"] = bool(
                    case["loop"]["median_ms"] * (1 - case["loop"]["spread"])
                    > case["ensemble"]["median_ms"] * (1 + case["ensemble"]["spread"]))
                # the contraction alone
                d_par, d_thr = ctx.upload(np.asarray(sets)), ctx.upload(np.log10(np.broadcast_to(mthresh, (S, nz))))
                d_ngal, d_bg = ctx.empty((S, nz)), ctx.empty((S, nz))
                coef = ctx.empty((he.coef_block_size(S, nz, nm),))
                d_u = h.uk_profiles.dev("nfw")
                d_damp, out = ctx.upload(np.ones(nk)), ctx.empty((4, S, nz, nk))

                def occupations():
                    ctx.call("hmg_hod_ensemble", S, nz, nm, 0, d_par.ptr, d_thr.ptr, h._d_zs().ptr, h._d_ms().ptr,
                             h._d_nzm.ptr, h._d_bh.ptr, h._d_wm().ptr, d_ngal.ptr, d_bg.ptr, None, coef.ptr)

                def kernel():
                    ctx.call("hmg_hod_ensemble_power", S, nz, nm, nk, nk, d_u.ptr, d_u.ptr, coef.ptr, d_ngal.ptr, d_bg.ptr,
                             **h._model_block("hmg_hod_ensemble_power"), d_kindex=None, d_damp=d_damp.ptr, d_out=out.ptr,
                             d_parts=None)

                occupations()
                k = alternate(ctx, {"occupations": occupations, "kernel": kernel}, a.reps, a.warmup, a.window)
                case.update(k)
                issue_ms = 1e3 * 5.0 * S * nz * nm * nk / FMA_PEAK
                bytes_ms = 1e3 * ((S + 7) // 8) * nz * nm * nk * 8 / HBM_PEAK
                case["issue_bound_ms"], case["byte_bound_ms"] = issue_ms, bytes_ms
                case["bound"] = "issue" if issue_ms >= bytes_ms else "bytes"
                case["share_of_issue_bound"] = issue_ms / k["kernel"]["median_ms"]
                case["share_of_byte_bound"] = bytes_ms / k["kernel"]["median_ms"]
                assert np.all(np.isfinite(out.numpy()))
            res["cases"].append(case)
    res["kernel_source_sha16"] = nat.kernel_source_sha16()
    print(json.dumps(res))
    if a.resources:
        sys.stdout.flush()
        subprocess.run([sys.executable, os.path.join(HERE, "tools", "kernel_resources.py")], check=True)


if __name__ == "__main__":
    main()
