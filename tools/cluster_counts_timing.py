#!/usr/bin/env python3
"""Device time of the cluster counts (hmg_cluster_selection) on GPU 0: one
cluster_abundance_device of the Config-3 halo grid (nz 32 x nm 512) against a survey of T = 256 noise tiles with the
default 64-node scatter rule in nq = 8 bins of significance - 2.4e9 fp64 erfc - and, the yardstick, one pass of the
one-pair mass integrals (hmg_power) over the Config-3 tensor in the same run.  The model and the survey are built and
uploaded once; each call is repeated --warmup times, then timed --reps times between event records on the context's
stream.  cluster_abundance_device is also timed end to end on the host's clock (uploads included), and the numpy
restatement of the same sum (tests/helpers/cluster_counts_model.py) once on this host (--numpy-z redshifts of the 32,
scaled up).  Prints one JSON line: median, minimum and maximum milliseconds, erfc per second, and that rate against the
kernel's instruction-issue bound (--valu-per-erfc vector instructions per erfc, counted in `make asm`'s clusters.s).

Usage:  python tools/cluster_counts_timing.py [--reps 10] [--warmup 2] [--numpy-z 1]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "tests", "helpers"))

import hmvec_amd as hm  # noqa: E402
from hmvec_amd import _native as nat  # noqa: E402
from onepoint_timing import spread, timed  # noqa: E402

CUS, SIMDS, CLOCK_HZ = 256, 4, 2.4e9      # MI355X: a wave64 vector instruction occupies its SIMD for 4 cycles


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--numpy-z", type=int, default=1, help="redshifts the numpy restatement runs (0: skip it)")
    ap.add_argument("--valu-per-erfc", type=float, default=160.0,
                    help="vector instructions per erfc: 142 of the edge loop + 20 nq / (nq + 1) of a bin (hmvec_amd/csrc/clusters.s)")
    a = ap.parse_args()
    nz, nm, nk, T, G, nq = 32, 512, 4096, 256, 64, 8
    zs, ms, ks = np.linspace(0.01, 3.0, nz), np.geomspace(2e10, 1e17, nm), np.geomspace(1e-4, 100, nk)
    h = hm.HaloModel(zs, ks, ms=ms, accuracy="low", engine="analytic")
    ctx = h._main(needs_aux=True)
    rng = np.random.default_rng(0)
    noise, area = np.geomspace(0.5, 4.0, T), rng.uniform(0.5, 1.5, T) * (4.0 * np.pi * 0.3 / T)
    sel = hm.cluster_selection([5.0, 5.5, 6.0, 7.0, 8.0, 10.0, 14.0, 20.0, np.inf], noise, area, sigma_ln=0.2)
    lnobs = hm.powerlaw_lnobs(h, np.log(6.0), 1.6, C=0.7, mpivot=3e14)
    d_ln, d_sig = ctx.upload(lnobs), ctx.upload(np.full((nz, nm), 0.2))
    d_lnn, d_area, d_t, d_w, d_e = (ctx.upload(v) for v in (sel.lnnoise, sel.area, sel.t, sel.w, sel.edges))
    n, bn = ctx.empty((nz, nq)), ctx.empty((nz, nq))
    erfcs = nz * nm * T * G * (nq + 1)
    res = {"grid": [nz, nm], "tiles": T, "nodes": G, "bins": nq, "erfc": erfcs}

    def call(S=None):
        ctx.call("hmg_cluster_selection", nz=nz, nm=nm, T=T, G=G, nq=nq, kind=0, d_lnobs=d_ln.ptr, d_sigln=d_sig.ptr,
                 d_lnnoise=d_lnn.ptr, d_area=d_area.ptr, d_t=d_t.ptr, d_w=d_w.ptr, d_edges=d_e.ptr, m_lo=0, m_hi=nm,
                 **h._model_block("hmg_cluster_selection"), d_n=n.ptr, d_bn=bn.ptr, d_S=nat.ptr(S))

    r = timed(ctx, a.reps, a.warmup, call)
    r["erfc_per_s"] = erfcs / (r["median_ms"] * 1e-3)
    bound = CUS * SIMDS * 64 * CLOCK_HZ / (4.0 * a.valu_per_erfc)
    r["issue_bound_erfc_per_s"], r["fraction_of_issue_bound"] = bound, r["erfc_per_s"] / bound
    res["selection"] = r
    S = ctx.empty((nz, nm, nq))
    res["selection_with_S"] = timed(ctx, a.reps, a.warmup, lambda: call(S))
    got_n, got_bn = n.numpy(), bn.numpy()
    assert np.all(np.isfinite(got_n)) and np.all(got_n > 0) and np.all(np.isfinite(got_bn))
    wall = []
    for i in range(a.warmup + a.reps):
        ctx.sync()
        t0 = time.perf_counter()
        dn, _ = hm.cluster_abundance_device(h, lnobs, sel)
        ctx.sync()
        if i >= a.warmup:
            wall.append(1e3 * (time.perf_counter() - t0))
    res["cluster_abundance_device_wall"] = spread(wall)
    assert np.array_equal(dn.numpy(), got_n)
    tm_ = h._tracer(h._resolve("nfw")[0], 1)
    p1 = ctx.empty((nz, nk))
    res["power_1h_nfw_nfw"] = timed(ctx, a.reps, a.warmup, lambda: ctx.call(
        "hmg_power", nz, nm, nk, C.byref(tm_), C.byref(tm_), h._d_nzm.ptr, h._d_bh.ptr, h._d_ms().ptr, h._d_wm().ptr,
        h._d_ks().ptr, h._d_Pzk().ptr, h._rho_m0(), float(h.p["kstar_damping"]), p1.ptr, None))
    if a.numpy_z > 0:
        import cluster_counts_model as cm
        from hmvec_amd.quadrature import trapz_weights
        k = min(a.numpy_z, nz)
        t0 = time.perf_counter()
        Sref = cm.selection(lnobs[:k], np.full((k, nm), 0.2), sel.lnnoise, sel.area, sel.t, sel.w, sel.edges, 0)
        nref, _ = cm.mass_sums(Sref, trapz_weights(ms), np.array(h.nzm)[:k], np.array(h.bh)[:k])
        dt = time.perf_counter() - t0
        res["numpy_restatement_s"] = dt * nz / k
        res["numpy_restatement_redshifts_run"] = k
        res["max_rel_diff_to_numpy"] = float(np.max(np.abs(got_n[:k] - nref) / nref))
    res["kernel_source_sha16"] = nat.kernel_source_sha16()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
