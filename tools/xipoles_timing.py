#!/usr/bin/env python3
"""Device time of the correlation-multipole transform (hmg_xi_multipoles) on GPU 0: one launch of
192 rows of nk 4096 at 64 separations for xi_0 alone, xi_2 with xi_4, and all three, from contiguous rows and - all
three - from the (rows, nk, 3) layout of multipoles_device; hmg_xi_transform at the same shape in the same run, for
scale.  Rows are a matter-like spectrum with per-row amplitudes, separations geomspace(0.1, 200, 64).  Section 13's
protocol (tools/realspace_timing.py): inputs uploaded once, --warmup launches, then --reps windows of --batch
back-to-back launches between two event records on the context's stream, no profiler.  Prints one JSON line with the
median and minimum milliseconds per launch.

Usage:  python tools/xipoles_timing.py [--reps 20] [--warmup 3] [--batch 10]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from hmvec_amd import _native as nat  # noqa: E402
from tools.realspace_timing import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=10)
    a = ap.parse_args()
    ctx = nat.Context(0)
    rng = np.random.default_rng(0)
    rows, nk = 192, 4096
    ss = np.geomspace(0.1, 200, 64)
    ks = np.geomspace(1e-4, 100, nk)
    base = rng.uniform(0.5, 2.0, (rows, 1)) * (2e4 * (ks / 0.02) / (1 + (ks / 0.02) ** 2) ** 1.9)[None, :]
    P = np.stack([base, 0.6 * base, 0.1 * base])                                        # (3, rows, nk)
    d_ks, d_ss, d_P = ctx.upload(ks), ctx.upload(ss), ctx.upload(P)
    d_S = ctx.upload(np.ascontiguousarray(np.moveaxis(P, 0, -1)))                       # (rows, nk, 3)
    o = [ctx.empty((rows, ss.size)) for _ in range(3)]
    ref = ctx.empty((rows, ss.size))
    p = [d_P.ptr + 8 * i * rows * nk for i in range(3)]
    q = [d_S.ptr + 8 * i for i in range(3)]
    head = (rows, nk, ss.size, d_ks.ptr)
    res = {}
    for label, ins, strides, outs in (
            ("xi0", (p[0], None, None), (nk, 1), (o[0].ptr, None, None)),
            ("xi2_xi4", (None, p[1], p[2]), (nk, 1), (None, o[1].ptr, o[2].ptr)),
            ("xi0_xi2_xi4", tuple(p), (nk, 1), tuple(x.ptr for x in o)),
            ("xi0_xi2_xi4_strided", tuple(q), (3 * nk, 3), tuple(x.ptr for x in o))):
        got = [x.numpy() for x in o] if label.endswith("strided") else None
        res[label] = timed(ctx, a.reps, a.warmup, a.batch, "hmg_xi_multipoles", *head, *ins, *strides, d_ss.ptr, *outs)
        res[label]["panel_separation_pairs"] = rows * (nk - 1) * ss.size
        if got is not None:
            assert all(np.array_equal(x.numpy(), g) for x, g in zip(o, got))           # strided = contiguous, bit for bit
    res["xi_transform"] = timed(ctx, a.reps, a.warmup, a.batch, "hmg_xi_transform", *head, p[0], d_ss.ptr, ref.ptr)
    assert np.array_equal(o[0].numpy(), ref.numpy()) and all(np.all(np.isfinite(x.numpy())) for x in o)
    res["kernel_source_sha16"] = nat.kernel_source_sha16()
    print(json.dumps(res))
    ctx.close()


if __name__ == "__main__":
    main()
