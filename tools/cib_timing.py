#!/usr/bin/env python3
"""Device time of the CIB halo model (hmg_cib_luminosity, hmg_emission_power) on GPU 0, on the
Config-3 grid (nz 32 x nm 512 x nk 4096) with F = 9 frequencies, "nfw" as the satellite tensor and as the one partner:

  luminosity   hmg_cib_luminosity alone on buffers that exist, for nsub in --nsub (default 64 256);
  grid, nodes  hmg_emission_power alone on the whole k grid and on 64 log-spaced nodes (with a node list the call waits on
               the host for the check of the list: that wait is part of the figure, as every caller pays it);
  end_to_end   get_power_cib(model, nus): luminosities, their sums, the contraction, the partner's two-halo terms, the
               copies to the host and the assembly;
  power        one hmg_power pass (P_1h and P_2h of "nfw" x "nfw") over the same tensor, the yardstick.

Method: each figure is the time between two event records on the context's stream around a window of repeated calls that
lasts at least --window seconds (default 0.5), after --warmup calls of the same shape; the windows alternate, --reps times
(default 5); median, and spread = (max - min) / median over the repeats.  The contraction is put against its issue bound at
the fp64 vector peak (78.6 TFLOP/s = 39.3e12 FMA/s), twice: with the operations the definition needs per (z, m, k) -
2 per pair, 3 per frequency for t, a and w t, 1 per leg and 1 per cross - and with those the tiled kernel issues (a tile
recomputes t, a, w t of its two blocks, and F is padded to a multiple of 4); and against its byte bound, the tensor once
at 8 TB/s.  Prints one JSON line.

Usage:  python tools/cib_timing.py [--nsub 64 256] [--reps 5] [--warmup 2] [--window 0.5] [--grid 32 512 4096]"""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "tools"))

import hmvec_amd as hm  # noqa: E402
from hmvec_amd import _native as nat  # noqa: E402
from hmvec_amd import cib  # noqa: E402
from hod_ensemble_timing import FMA_PEAK, HBM_PEAK, alternate  # noqa: E402

NUS = np.array([100.0, 143.0, 217.0, 353.0, 545.0, 857.0, 1200.0, 2000.0, 3000.0])


def issued_ops(F, NP):
    """fp64 operations per (z, m, k) the tiled kernel issues: per diagonal tile 3 T for t, a, w t, T (T + 1) pair FMAs,
    T legs, NP (T + 1) for the crosses; per off-diagonal tile 5 T and 2 T^2."""
    T = cib.FREQ_TILE
    nb = (F + T - 1) // T
    return nb * (3 * T + T * (T + 1) + T + NP * (T + 1)) + nb * (nb - 1) // 2 * (5 * T + 2 * T * T)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nsub", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--grid", type=int, nargs=3, default=[32, 512, 4096])
    a = ap.parse_args()
    nz, nm, nk = a.grid
    zs, ms, ks = np.linspace(0.01, 3.0, nz), np.geomspace(2e10, 1e17, nm), np.geomspace(1e-4, 100, nk)
    h = hm.HaloModel(zs, ks, ms=ms, accuracy="low", engine="analytic")
    nodes = np.round(np.geomspace(1, nk - 1, 64)).astype(np.int64)          # 64 log-spaced nodes, kept distinct
    for i in range(1, nodes.size):
        nodes[i] = max(nodes[i], nodes[i - 1] + 1)
    assert nodes[-1] <= nk - 1 and np.unique(nodes).size == 64
    ctx = h._main(needs_aux=True)
    F, NP = NUS.size, 1
    p, x0 = dict(cib.cib_defaults), hm.sed_break(cib.cib_defaults["beta"], cib.cib_defaults["gamma"])
    res = {"grid": [nz, nm, nk], "F": F, "partners": NP, "tensor_bytes": nz * nm * nk * 8, "nodes": int(nodes.size)}
    run = dict(reps=a.reps, warmup=a.warmup, window=a.window)

    # the luminosities alone
    chis = np.asarray(h.comoving_radial_distance(zs), dtype=np.float64).reshape(-1)
    d_nus, d_chis = ctx.upload(NUS), ctx.upload(chis)
    d_Lc, d_Ls = ctx.empty((F, nz, nm)), ctx.empty((F, nz, nm))
    par = (nat.C.c_double * nat.DEFINES["HMG_CIB_NPAR"])(*[p[k] for k in cib.PARAMETERS], x0)
    fns, keep = {}, []
    for nsub in a.nsub:
        t, w = hm.sub_rule(nsub)
        d_t, d_w = ctx.upload(t), ctx.upload(w)
        keep += [d_t, d_w]

        def lum(nsub=nsub, d_t=d_t, d_w=d_w):
            ctx.call("hmg_cib_luminosity", F, nz, nm, nsub, d_nus.ptr, h._d_zs().ptr, h._d_ms().ptr, d_chis.ptr, None, d_t.ptr,
                     d_w.ptr, par, d_Lc.ptr, d_Ls.ptr)

        fns[f"luminosity_nsub{nsub}"] = lum
    res["luminosity"] = alternate(ctx, fns, **run)

    # the contraction alone, against one hmg_power pass over the same tensor
    tables = hm.cib_luminosities(h, NUS, nsub=64)
    d_u = h.uk_profiles.dev("nfw")
    tr = (nat.Tracer * 1)(nat.Tracer(nat.TRACER_MATTER, d_u.ptr))
    npair = F * (F + 1) // 2
    block = h._model_block("hmg_emission_power")
    out = {}
    fns = {}
    for what, kidx in (("grid", None), ("nodes", nodes)):
        n = nk if kidx is None else kidx.size
        d_k = None if kidx is None else ctx.upload_int32(kidx)
        d_damp = ctx.upload(np.ones(n))
        P1h, I, X = ctx.empty((npair, nz, n)), ctx.empty((F, nz, n)), ctx.empty((NP, F, nz, n))
        out[what] = (P1h, I, X, d_k, d_damp)

        def contraction(n=n, bufs=out[what]):
            P1h, I, X, d_k, d_damp = bufs
            ctx.call("hmg_emission_power", F=F, nz=nz, nm=nm, nk=nk, n=n, d_us=d_u.ptr, d_Lc=tables.Lc.ptr, d_Ls=tables.Ls.ptr,
                     NP=NP, h_partners=tr, **block, d_kindex=nat.ptr(d_k), d_damp=d_damp.ptr, d_P1h=P1h.ptr, d_I=I.ptr,
                     d_X1h=X.ptr)

        fns[what] = contraction
    o1, o2 = ctx.empty((nz, nk)), ctx.empty((nz, nk))
    fns["power"] = lambda: h.power_device("nfw", "nfw", out1=o1, out2=o2)
    fns["end_to_end"] = lambda: hm.get_power_cib(h, NUS, partners=("nfw",), nsub=64)
    res["contraction"] = c = alternate(ctx, fns, **run)
    assert np.all(np.isfinite(out["grid"][0].numpy())) and np.all(np.isfinite(out["nodes"][2].numpy()))
    needed = 2 * npair + (4 + NP) * F
    elements = nz * nm * nk
    res["ops_needed"], res["ops_issued"] = needed, issued_ops(F, NP)
    res["issue_bound_ms"] = 1e3 * needed * elements / FMA_PEAK
    res["issued_bound_ms"] = 1e3 * issued_ops(F, NP) * elements / FMA_PEAK
    res["byte_bound_ms"] = 1e3 * elements * 8 / HBM_PEAK
    res["share_of_issue_bound"] = res["issue_bound_ms"] / c["grid"]["median_ms"]
    res["share_of_issued_bound"] = res["issued_bound_ms"] / c["grid"]["median_ms"]
    res["grid_over_power"] = c["grid"]["median_ms"] / c["power"]["median_ms"]
    res["kernel_source_sha16"] = nat.kernel_source_sha16()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
