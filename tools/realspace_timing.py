#!/usr/bin/env python3
"""Device time of the correlation-function transform (hmg_xi_transform), of the Hankel
transforms (hmg_hankel_transform: W_0 alone, W_2 alone and both from one launch; section 14) and of the angular
transforms (hmg_angular_transform: W_0, W_2, W_4 alone, W_0 with W_4 - xi+ and xi- - and all three, with every distance
1 so that the radii are the same; hmg_angular_zsum with ten rows of weights; section 22) on GPU 0, one launch of
  * 6 spectra x nz 32 rows of nk 4096 at 64 radii (the Config-3 grid), and
  * 6 spectra x nz 20 rows of nk 1001 at 64 radii (the README grid).
Rows are a matter-like spectrum with per-row amplitudes, radii geomspace(0.1, 200, 64).  Inputs are uploaded once; the
launch is repeated --warmup times, then timed --reps times between event records on the context's stream; each timed
window holds --batch launches (a single launch is shorter than the event resolution allows to trust).  Prints one JSON
line with the median and minimum milliseconds per launch.

Usage:  python tools/realspace_timing.py [--reps 20] [--warmup 3] [--batch 10]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from hmvec_amd import _native as nat  # noqa: E402

SLOT0 = 100       # event slots clear of HaloModel's (0-3) and bench.py's (40 and up)


def timed(ctx, reps, warmup, batch, entry, *args):
    for _ in range(warmup):
        ctx.call(entry, *args)
    ctx.sync()
    ms = []
    for _ in range(reps):
        ctx.record(SLOT0)
        for _ in range(batch):
            ctx.call(entry, *args)
        ctx.record(SLOT0 + 1)
        ctx.sync()
        ms.append(ctx.elapsed_ms(SLOT0, SLOT0 + 1) / batch)
    return dict(median_ms=float(np.median(ms)), min_ms=float(np.min(ms)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=10)
    a = ap.parse_args()
    ctx = nat.Context(0)
    rng = np.random.default_rng(0)
    rs = np.geomspace(0.1, 200, 64)
    d_rs = ctx.upload(rs)
    res = {}
    for shape, rows, nk in (("6x32_rows_nk4096_nr64", 6 * 32, 4096), ("6x20_rows_nk1001_nr64", 6 * 20, 1001)):
        ks = np.geomspace(1e-4, 100, nk)
        P = rng.uniform(0.5, 2.0, (rows, 1)) * (2e4 * (ks / 0.02) / (1 + (ks / 0.02) ** 2) ** 1.9)[None, :]
        d_ks, d_P, out, out2 = ctx.upload(ks), ctx.upload(P), ctx.empty((rows, rs.size)), ctx.empty((rows, rs.size))
        common = (rows, nk, rs.size, d_ks.ptr, d_P.ptr, d_rs.ptr)
        for label, entry, outs in (("xi", "hmg_xi_transform", (out.ptr,)), ("w0", "hmg_hankel_transform", (out.ptr, None)),
                                   ("w2", "hmg_hankel_transform", (None, out2.ptr)),
                                   ("w0_w2", "hmg_hankel_transform", (out.ptr, out2.ptr))):
            label = f"{label}_{shape}"
            res[label] = timed(ctx, a.reps, a.warmup, a.batch, entry, *common, *outs)
            res[label]["panel_radius_pairs"] = rows * (nk - 1) * rs.size
            got = out.numpy()
            assert np.all(np.isfinite(got)) and np.all(got[:, 0] > 0) and np.all(np.isfinite(out2.numpy()))
        w0 = out.numpy()                 # (W_0 of the last Hankel launch: the angular launch must give its bits)
        n, nz, nw = 6, rows // 6, 10
        d_chi, d_zw = ctx.upload(np.ones(nz)), ctx.upload(rng.uniform(-1.0, 1.0, (nw, nz)))
        a0, a2, a4 = (ctx.empty((rows, rs.size)) for _ in range(3))
        zs = ctx.empty((n, nw, rs.size))
        ang = (n, nz, nk, rs.size, d_ks.ptr, d_P.ptr, d_chi.ptr, d_rs.ptr)
        for label, outs in (("ang_w0", (a0.ptr, None, None)), ("ang_w2", (None, a2.ptr, None)),
                            ("ang_w4", (None, None, a4.ptr)), ("ang_w0_w4", (a0.ptr, None, a4.ptr)),
                            ("ang_w0_w2_w4", (a0.ptr, a2.ptr, a4.ptr))):
            label = f"{label}_{shape}"
            res[label] = timed(ctx, a.reps, a.warmup, a.batch, "hmg_angular_transform", *ang, *outs)
            res[label]["panel_radius_pairs"] = rows * (nk - 1) * rs.size
        assert np.array_equal(a0.numpy(), w0) and np.all(np.isfinite(a4.numpy()))
        res[f"ang_zsum_nw{nw}_{shape}"] = timed(ctx, a.reps, a.warmup, a.batch, "hmg_angular_zsum", n, nz, rs.size, nw,
                                                d_zw.ptr, a4.ptr, zs.ptr)
        assert np.all(np.isfinite(zs.numpy()))
    res["kernel_source_sha16"] = nat.kernel_source_sha16()
    print(json.dumps(res))
    ctx.close()


if __name__ == "__main__":
    main()
