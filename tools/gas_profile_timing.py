#!/usr/bin/env python3
"""Device time of the projected gas / pressure profile kernels on GPU 0: 10 000 profiles x 32 radii
through hmg_gnfw_projected for each kind ("sigma", "mean", "excess"), for general rows (alpha != 1: the gas profile) and
alpha == 1 rows (the pressure profile), and through hmg_gnfw_projected_smooth.  Inputs are uploaded once; each kernel is
launched --warmup times, then timed --reps times between event records on the context's stream.  Prints one JSON line with
the median and minimum milliseconds per kernel and its integrand evaluations per second (from the median): an output
costs 64 evaluations of the family for "sigma" (the line of sight), 128 for "mean" and "excess" (line of sight + inner
sphere), 64 x 64 for the smoothed projection (64 outer nodes, a line of sight each).

Usage:  python tools/gas_profile_timing.py [--reps 20] [--warmup 3]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from hmvec_amd import _native as nat  # noqa: E402

SLOT0 = 100       # event slots clear of HaloModel's (0-3) and bench.py's (40 and up)
EVALS = {"sigma": 64, "mean": 128, "excess": 128, "smooth": 64 * 64}
KINDS = {"sigma": nat.GNFW_SIGMA, "mean": nat.GNFW_MEAN, "excess": nat.GNFW_EXCESS}


def timed(ctx, reps, warmup, name, *args):
    for _ in range(warmup):
        ctx.call(name, *args)
    ctx.sync()
    ms = []
    for _ in range(reps):
        ctx.record(SLOT0)
        ctx.call(name, *args)
        ctx.record(SLOT0 + 1)
        ms.append(ctx.elapsed_ms(SLOT0, SLOT0 + 1))
    return dict(median_ms=float(np.median(ms)), min_ms=float(np.min(ms)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    ctx = nat.Context(0)
    rng = np.random.default_rng(0)

    n, nr = 10000, 32
    xcut = rng.uniform(2.0, 4.0, n)                                   # r_vir / (R200c / 2), r_vir / (xc R200c)
    x = xcut[:, None] * np.geomspace(0.01, 1.5, nr)[None, :]          # the last radii lie beyond the cut
    eta = rng.uniform(3.5, 6.0, n)
    sig = rng.uniform(0.05, 1.0, n)
    d_xc, d_x, d_eta, d_sig = (ctx.upload(v) for v in (xcut, x, eta, sig))
    out = ctx.empty((n, nr))
    res = {}
    for label, alpha, gamma in (("general", rng.uniform(0.7, 0.95, n), -0.2), ("alpha1", np.ones(n), -0.3)):
        d_al = ctx.upload(alpha)
        for kind, code in KINDS.items():
            r = timed(ctx, a.reps, a.warmup, "hmg_gnfw_projected", n, nr, 1, code, d_al.ptr, d_eta.ptr, d_xc.ptr, gamma,
                      d_x.ptr, out.ptr)
            r["evals_per_s"] = n * nr * EVALS[kind] / (r["median_ms"] * 1e-3)
            res[f"{kind}_{label}_10000x32"] = r
            assert np.all(np.isfinite(out.numpy()))
        r = timed(ctx, a.reps, a.warmup, "hmg_gnfw_projected_smooth", n, nr, 1, nat.GNFW_SIGMA, d_al.ptr, d_eta.ptr,
                  d_xc.ptr, gamma, d_x.ptr, d_sig.ptr, out.ptr)
        r["evals_per_s"] = n * nr * EVALS["smooth"] / (r["median_ms"] * 1e-3)
        res[f"smooth_{label}_10000x32"] = r
        assert np.all(np.isfinite(out.numpy()))
    res["kernel_source_sha16"] = nat.kernel_source_sha16()
    print(json.dumps(res))
    ctx.close()


if __name__ == "__main__":
    main()
