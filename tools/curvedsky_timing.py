#!/usr/bin/env python3
"""Device time of the curved-sky Gaussian covariance on GPU 0 for the 3x2pt-like data vector of
tools/angcov_timing.py: 8 fields (3 lens bins of spin 0, 5 source bins of spin 2), 41 probes (w of the lens bins, gamma_t
of every lens about every source bin, xi+ of 12 and xi- of 11 of the 15 source pairs), 20 bins in theta from 5e-4 to 0.1
and 17 log-spaced nodes to l_max = 2e4.  Timed separately between event records on the context's stream: the weights
launch (four kinds: the recurrence from l = 0 at 21 edges), the contraction with its ordered combine, and next to them
the flat path's two launches on the same shape, all four as angcov.sky_gaussian_launches builds them for the library.
Inputs are uploaded once; each timed window holds --batch launches.  Prints one JSON line.

Usage:  python tools/curvedsky_timing.py [--reps 10] [--warmup 2] [--batch 3]"""
import argparse
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
    res = dict(fields=nf, probes=np_, bins=nt, multipoles=nl, nodes=int(nodes.size))
    weights, gaussian, cov, _keepalive = angcov.sky_gaussian_launches(curvedsky.CURVED, ctx, nodes, l0, nl, Cn, noise, edges, pr, fsky)
    res["weights"] = timed(ctx, a.reps, a.warmup, a.batch, *weights)
    res["gaussian"] = timed(ctx, a.reps, a.warmup, a.batch, *gaussian)
    res["total_median_ms"] = res["weights"]["median_ms"] + res["gaussian"]["median_ms"]
    got = cov.numpy()
    assert np.all(np.isfinite(got)) and np.array_equal(got, got.transpose(2, 3, 0, 1))
    assert np.array_equal(got, curvedsky.curved_cov_gaussian(nodes, Cn, noise, edges, probes, fsky, spins=spins, ctx=ctx))
    # the flat path on the same shape
    weights, gaussian, fcov, _fkeepalive = angcov.sky_gaussian_launches(
        angcov.FLAT, ctx, nodes, l0, nl, Cn, noise, edges, angcov.check_probes(data_vector(), nf), fsky)
    res["flat_weights"] = timed(ctx, a.reps, a.warmup, a.batch, *weights)
    res["flat_gaussian"] = timed(ctx, a.reps, a.warmup, a.batch, *gaussian)
    res["flat_total_median_ms"] = res["flat_weights"]["median_ms"] + res["flat_gaussian"]["median_ms"]
    flat = fcov.numpy()
    res["max_rel_diff_curved_to_flat"] = float(np.max(np.abs(got - flat)) / np.max(np.abs(flat)))
    res["kernel_source_sha16"] = nat.kernel_source_sha16()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
