#!/usr/bin/env python3
"""Device time of the cluster-lensing kernels (DESIGN.md sections 10 and 12) on GPU 0:
  * Sigma of 10 000 halos x 32 radii, centred (hmg_lensing_sigma_nfw) and miscentred (hmg_lensing_sigma_nfw_off);
  * Delta Sigma of the same halos and radii, centred (hmg_lensing_delta_sigma_nfw) and miscentred
    (hmg_lensing_delta_sigma_nfw_off);
  * kappa_2h and gamma_t_2h at nz = 32, ntheta = 64, nk = 4096 (hmg_lensing_kappa_2h, hmg_lensing_gamma_t_2h, nM = 16).
Inputs are uploaded once; each kernel is launched --warmup times, then timed --reps times between event records on
the context's stream.  Prints one JSON line with the median and minimum milliseconds per kernel.

Usage:  python tools/lensing_timing.py [--reps 20] [--warmup 3]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from hmvec_amd import _native as nat  # noqa: E402

SLOT0 = 100       # event slots clear of HaloModel's (0-3) and bench.py's (40 and up)


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
    rs = rng.uniform(0.05, 0.6, n)
    dc = 10 ** rng.uniform(3, 5, n)
    rhoc = np.full(n, 1.3e11)
    da = rng.uniform(500, 1700, n)                              # D_A [Mpc]
    rbins = da[:, None] * (np.geomspace(0.5, 30, nr) * np.pi / 180 / 60)[None, :]
    off = da * (0.5 * np.pi / 180 / 60)
    d = [ctx.upload(x) for x in (rs, dc, rhoc, rbins, off)]
    out = ctx.empty((n, nr))
    res = {"sigma_centred_10000x32": timed(ctx, a.reps, a.warmup, "hmg_lensing_sigma_nfw", n, nr, 1,
                                           d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr, out.ptr)}
    res["sigma_miscentred_10000x32"] = timed(ctx, a.reps, a.warmup, "hmg_lensing_sigma_nfw_off", n, nr, 1, d[0].ptr,
                                             d[1].ptr, d[2].ptr, d[3].ptr, d[4].ptr, out.ptr)
    assert np.all(np.isfinite(out.numpy()))
    res["delta_sigma_centred_10000x32"] = timed(ctx, a.reps, a.warmup, "hmg_lensing_delta_sigma_nfw", n, nr, 1,
                                                d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr, out.ptr)
    res["delta_sigma_miscentred_10000x32"] = timed(ctx, a.reps, a.warmup, "hmg_lensing_delta_sigma_nfw_off", n, nr, 1,
                                                   d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr, d[4].ptr, out.ptr)
    assert np.all(np.isfinite(out.numpy()))

    nz, nt, nk, nm, nM = 32, 64, 4096, 64, 16
    ks = np.geomspace(1e-4, 100, nk)
    zs = np.linspace(0.1, 1.5, nz)
    chi = 3000.0 * zs / (1 + 0.3 * zs)
    pre = np.full(nz, 1e-3)
    Pzk = 1e4 * (ks / 0.02) / (1 + (ks / 0.02) ** 2.5)[None, :] * np.ones((nz, 1))
    ms = np.geomspace(1e11, 1e16, nm)
    bh = 1 + (ms / 1e14)[None, :] ** 0.5 * np.ones((nz, 1))
    th = np.geomspace(0.5, 30, nt) * np.pi / 180 / 60
    Ms = np.geomspace(1e13, 1e15, nM)
    e = [ctx.upload(x) for x in (ks, chi, pre, Pzk, th, ms, bh, Ms)]
    out2 = ctx.empty((nz, nt, nM))
    res["kappa_2h_nz32_nt64_nk4096"] = timed(ctx, a.reps, a.warmup, "hmg_lensing_kappa_2h", nz, nk, nt, nm, nM,
                                             e[0].ptr, e[1].ptr, e[2].ptr, e[3].ptr, e[4].ptr, 100.0, 1e4, e[5].ptr,
                                             e[6].ptr, e[7].ptr, out2.ptr)
    assert np.all(np.isfinite(out2.numpy()))
    res["gamma_t_2h_nz32_nt64_nk4096"] = timed(ctx, a.reps, a.warmup, "hmg_lensing_gamma_t_2h", nz, nk, nt, nm, nM,
                                               e[0].ptr, e[1].ptr, e[2].ptr, e[3].ptr, e[4].ptr, 100.0, 1e4, e[5].ptr,
                                               e[6].ptr, e[7].ptr, out2.ptr)
    assert np.all(np.isfinite(out2.numpy()))
    res["kernel_source_sha16"] = nat.kernel_source_sha16()
    print(json.dumps(res))
    ctx.close()


if __name__ == "__main__":
    main()
