#!/usr/bin/env python3
"""Device time of the curved-sky Gaussian covariance on GPU 0 for the 3x2pt-like data vector of
tools/angcov_timing.py: 8 fields (3 lens bins of spin 0, 5 source bins of spin 2), 41 probes (w of the lens bins, gamma_t
of every lens about every source bin, xi+ of 12 and xi- of 11 of the 15 source pairs), 20 bins in theta from 5e-4 to 0.1
and 17 log-spaced nodes to l_max = 2e4.  Timed separately between event records on the context's stream: the weights
launch (hmg_curvedsky_weights, four kinds: the recurrence from l = 0 at 21 edges), the contraction with its ordered
combine (hmg_curvedsky_gaussian), and next to them the flat path's two launches on the same shape (hmg_angcov_weights,
hmg_angcov_gaussian).  Inputs are uploaded once; each timed window holds --batch launches.  Prints one JSON line.

Usage:  python tools/curvedsky_timing.py [--reps 10] [--warmup 2] [--batch 3]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from hmvec_amd import _native as nat  # noqa: E402
from hmvec_amd import angcov, curvedsky  # noqa: E402
from angcov_timing import data_vector, spectra  # noqa: E402
from realspace_timing import timed  # noqa: E402

KIND_OF_ORDER = {0: "w", 2: "gammat", 4: "xim"}


def curved_probes():
    """angcov_timing's data vector with its orders as kinds: order 0 of two source bins is xi+."""
    return [(f, g, "xip" if mu == 0 and f >= 3 else KIND_OF_ORDER[mu]) for f, g, mu in data_vector()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=3)
    a = ap.parse_args()
    ctx = nat.Context(0)
    nodes = np.geomspace(2.0, 2e4, 17)
    edges, fsky, spins = np.geomspace(5e-4, 0.1, 21), 0.12, [0, 0, 0, 2, 2, 2, 2, 2]
    Cn, noise = spectra(nodes)
    _, l0, nl = angcov.check_nodes(nodes)
    probes = curved_probes()
    pr = curvedsky.check_probes(probes, noise.size, spins)
    nt, np_, nf = edges.size - 1, len(probes), noise.size
    d_edges, d_cd = ctx.upload(edges), ctx.upload(curvedsky.cos_differences(edges))
    K = [ctx.empty((nl, nt)) for _ in range(4)]
    res = dict(fields=nf, probes=np_, bins=nt, multipoles=nl, nodes=int(nodes.size))
    res["weights"] = timed(ctx, a.reps, a.warmup, a.batch, "hmg_curvedsky_weights", l0, nl, nt, d_edges.ptr, d_cd.ptr,
                           *(k.ptr for k in K))
    words = np_ * (np_ + 1) // 2 * ((nl - 1) // angcov.chunk() + 1) * nt * nt
    work, cov = ctx.empty((words,)), ctx.empty((np_, nt, np_, nt))
    d_nodes, d_C, d_noise, d_pr = ctx.upload(nodes), ctx.upload(Cn), ctx.upload(noise), ctx.upload_int32(pr)
    res["gaussian"] = timed(ctx, a.reps, a.warmup, a.batch, "hmg_curvedsky_gaussian", nf, nodes.size, d_nodes.ptr, d_C.ptr,
                            d_noise.ptr, l0, nl, nt, d_cd.ptr, np_, pr.ctypes.data_as(C.POINTER(C.c_int)), d_pr.ptr,
                            4.0 * np.pi * fsky, *(k.ptr for k in K), words, work.ptr, cov.ptr)
    res["total_median_ms"] = res["weights"]["median_ms"] + res["gaussian"]["median_ms"]
    got = cov.numpy()
    assert np.all(np.isfinite(got)) and np.array_equal(got, got.transpose(2, 3, 0, 1))
    assert np.array_equal(got, curvedsky.curved_cov_gaussian(nodes, Cn, noise, edges, probes, fsky, spins=spins, ctx=ctx))
    # the flat path on the same shape
    fpr = angcov.check_probes(data_vector(), nf)
    d_ells, d_fpr = ctx.upload(np.arange(l0, l0 + nl, dtype=np.float64)), ctx.upload_int32(fpr)
    res["flat_weights"] = timed(ctx, a.reps, a.warmup, a.batch, "hmg_angcov_weights", nl, nt, d_ells.ptr, d_edges.ptr,
                                *(k.ptr for k in K[:3]))
    res["flat_gaussian"] = timed(ctx, a.reps, a.warmup, a.batch, "hmg_angcov_gaussian", nf, nodes.size, d_nodes.ptr,
                                 d_C.ptr, d_noise.ptr, l0, nl, nt, d_edges.ptr, np_, fpr.ctypes.data_as(C.POINTER(C.c_int)),
                                 d_fpr.ptr, 4.0 * np.pi * fsky, *(k.ptr for k in K[:3]), words, work.ptr, cov.ptr)
    res["flat_total_median_ms"] = res["flat_weights"]["median_ms"] + res["flat_gaussian"]["median_ms"]
    flat = cov.numpy()
    res["max_rel_diff_curved_to_flat"] = float(np.max(np.abs(got - flat)) / np.max(np.abs(flat)))
    res["kernel_source_sha16"] = nat.kernel_source_sha16()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
