#!/usr/bin/env python3
"""Device time of the correlation-function transform (hmg_xi_transform) on GPU 0, one launch of
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


def timed(ctx, reps, warmup, batch, *args):
    for _ in range(warmup):
        ctx.call("hmg_xi_transform", *args)
    ctx.sync()
    ms = []
    for _ in range(reps):
        ctx.record(SLOT0)
        for _ in range(batch):
            ctx.call("hmg_xi_transform", *args)
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
    for label, rows, nk in (("xi_6x32_rows_nk4096_nr64", 6 * 32, 4096), ("xi_6x20_rows_nk1001_nr64", 6 * 20, 1001)):
        ks = np.geomspace(1e-4, 100, nk)
        P = rng.uniform(0.5, 2.0, (rows, 1)) * (2e4 * (ks / 0.02) / (1 + (ks / 0.02) ** 2) ** 1.9)[None, :]
        d_ks, d_P, out = ctx.upload(ks), ctx.upload(P), ctx.empty((rows, rs.size))
        res[label] = timed(ctx, a.reps, a.warmup, a.batch, rows, nk, rs.size, d_ks.ptr, d_P.ptr, d_rs.ptr, out.ptr)
        xi = out.numpy()
        assert np.all(np.isfinite(xi)) and np.all(xi[:, 0] > 0)
        res[label]["panel_radius_pairs"] = rows * (nk - 1) * rs.size
    res["kernel_source_sha16"] = nat.kernel_source_sha16()
    print(json.dumps(res))
    ctx.close()


if __name__ == "__main__":
    main()
