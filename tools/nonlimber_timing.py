#!/usr/bin/env python3
"""Device time of the non-Limber two-halo projection on GPU 0 for F = 8 fields, ngz = 4096 nodes of
chi on [1140, 1860] Mpc, nkq = 4096 nodes of k linear to 0.6 / Mpc and lmax = 256: the transfer functions
(hmg_nonlimber_transfer: 4096 workgroups, 16 chunks of 256 chi nodes each, 17 tiles of orders), the k sum of all 36 pairs
(hmg_nonlimber_cl) and the probe (hmg_sph_bessel at 65536 arguments), timed between event records on the context's stream,
next to the numpy restatement of the transfers (tests/helpers/nonlimber_model.py) on --numpy-nodes of the k nodes, scaled
to all of them.  Inputs are uploaded once; each timed window holds --batch launches.  Prints one JSON line.

Usage:  python tools/nonlimber_timing.py [--reps 5] [--warmup 1] [--batch 1] [--numpy-nodes 8]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

from hmvec_amd import _native as nat  # noqa: E402
from realspace_timing import timed  # noqa: E402
import nonlimber_model as nlm  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--numpy-nodes", type=int, default=8)
    ap.add_argument("--fields", type=int, default=8)
    ap.add_argument("--ngz", type=int, default=4096)
    ap.add_argument("--nkq", type=int, default=4096)
    ap.add_argument("--lmax", type=int, default=256)
    a = ap.parse_args()
    F, ngz, nkq, lmax = a.fields, a.ngz, a.nkq, a.lmax
    ctx = nat.Context(0)
    rng = np.random.default_rng(0)
    chis, kq = np.linspace(1140.0, 1860.0, ngz), np.linspace(1e-4, 0.6, nkq)
    window = np.exp(-0.5 * ((chis - 1500.0) / 60.0) ** 2)
    src = rng.uniform(0.5, 1.5, (F, 1, nkq)) * window[None, :, None] * np.ones((1, 1, nkq))
    d_kq, d_chis, d_src = ctx.upload(kq), ctx.upload(chis), ctx.upload(src)
    T = ctx.empty((F, lmax + 1, nkq))
    res = dict(fields=F, ngz=ngz, nkq=nkq, lmax=lmax)
    res["transfer"] = timed(ctx, a.reps, a.warmup, a.batch, "hmg_nonlimber_transfer", F, ngz, nkq, lmax, d_kq.ptr, d_chis.ptr,
                            d_src.ptr, T.ptr)
    res["transfer"]["fma_per_launch"] = F * ngz * nkq * (lmax + 1)
    res["transfer"]["tflops"] = 2e-9 * res["transfer"]["fma_per_launch"] / res["transfer"]["median_ms"]
    pairs = np.ascontiguousarray([(f, g) for f in range(F) for g in range(f, F)], dtype=np.int32)
    out = ctx.empty((pairs.shape[0], lmax + 1))
    d_wk = ctx.upload(nlm.trapz_weights(kq))
    res["cl"] = timed(ctx, a.reps, a.warmup, a.batch, "hmg_nonlimber_cl", F, nkq, lmax, pairs.shape[0],
                      pairs.ctypes.data_as(C.POINTER(C.c_int)), ctx.upload_int32(pairs).ptr, d_kq.ptr, d_wk.ptr, T.ptr, out.ptr)
    res["cl"]["pairs"] = int(pairs.shape[0])
    xs = rng.uniform(1.0, 1000.0, 65536)
    J = ctx.empty((lmax + 1, xs.size))
    res["sph_bessel_65536"] = timed(ctx, a.reps, a.warmup, a.batch, "hmg_sph_bessel", lmax, xs.size, ctx.upload(xs).ptr, J.ptr)
    got, cl = T.numpy(), out.numpy()
    assert np.all(np.isfinite(got)) and np.all(np.isfinite(cl)) and np.all(cl[[0, -1]] > 0)
    # the restatement on a few k nodes, spread over the range, and its time scaled to all of them
    pick = np.linspace(0, nkq - 1, max(1, a.numpy_nodes)).astype(int)
    t0 = time.perf_counter()
    ref, gate = nlm.transfer(kq[pick], chis, src[:, :, pick], lmax, with_gate=True, cj=101.0)
    dt = time.perf_counter() - t0
    res["numpy_restatement_ms_scaled"] = 1e3 * dt / 2.0 * nkq / pick.size          # (the gate doubles the work)
    res["worst_error_over_gate"] = float(np.max(np.abs(got[:, :, pick] - ref) / np.maximum(gate, 1e-300)))
    res["kernel_source_sha16"] = nat.kernel_source_sha16()
    print(json.dumps(res))
    ctx.close()


if __name__ == "__main__":
    main()
