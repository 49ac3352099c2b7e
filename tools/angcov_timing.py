#!/usr/bin/env python3
"""Device time of the Gaussian covariance of angular correlation functions on GPU 0 for a
3x2pt-like data vector: 8 fields (3 lens bins, 5 source bins), 41 probes (w of the lens bins, gamma_t of every lens
about every source bin, xi+ of 12 and xi- of 11 of the 15 source pairs), 20 bins in theta and 17 log-spaced nodes to
l_max = 2e4.  Timed separately between event records on the context's stream: the weights launch (three orders) and
the contraction with its ordered combine, both as angcov.sky_gaussian_launches builds them for the library.  Inputs are
uploaded once; each timed window holds --batch launches.  Next to it, the wall time of the numpy einsum restatement
(tests/helpers/angcov_model.cov_numpy) on the same host, once.  Prints one JSON line.

Usage:  python tools/angcov_timing.py [--reps 10] [--warmup 2] [--batch 3]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

from hmvec_amd import _native as nat  # noqa: E402
from hmvec_amd import angcov  # noqa: E402
from realspace_timing import timed  # noqa: E402


def data_vector():
    lens, src = [0, 1, 2], [3, 4, 5, 6, 7]
    probes = [(f, f, 0) for f in lens] + [(f, g, 2) for f in lens for g in src]
    pairs = [(f, g) for i, f in enumerate(src) for g in src[i:]]
    probes += [(f, g, 0) for f, g in pairs[:12]] + [(f, g, 4) for f, g in pairs[:11]]
    return probes


def spectra(nodes, nf=8):
    amp = np.geomspace(3e-7, 2e-9, nf)
    auto = amp[:, None] / (1.0 + nodes[None, :] / np.linspace(40, 400, nf)[:, None]) ** 1.2
    C_ = 0.5 * np.sqrt(auto[:, None, :] * auto[None, :, :])
    C_[np.arange(nf), np.arange(nf)] = auto
    return C_, np.geomspace(2e-9, 1e-10, nf)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=3)
    ap.add_argument("--no-numpy", action="store_true")
    a = ap.parse_args()
    ctx = nat.Context(0)
    nodes = np.geomspace(2.0, 2e4, 17)
    probes, edges, fsky = data_vector(), np.geomspace(5e-4, 0.1, 21), 0.12
    Cn, noise = spectra(nodes)
    _, l0, nl = angcov.check_nodes(nodes)
    nt, np_, nf = edges.size - 1, len(probes), noise.size
    res = dict(fields=nf, probes=np_, bins=nt, multipoles=nl, nodes=int(nodes.size))
    weights, gaussian, cov, _keepalive = angcov.sky_gaussian_launches(
        angcov.FLAT, ctx, nodes, l0, nl, Cn, noise, edges, angcov.check_probes(probes, nf), fsky)
    res["weights"] = timed(ctx, a.reps, a.warmup, a.batch, *weights)
    res["gaussian"] = timed(ctx, a.reps, a.warmup, a.batch, *gaussian)
    res["gaussian"]["fma"] = np_ * (np_ + 1) // 2 * nl * nt * nt
    got = cov.numpy()
    assert np.all(np.isfinite(got)) and np.array_equal(got, got.transpose(2, 3, 0, 1))
    assert np.array_equal(got, angcov.real_cov_gaussian(nodes, Cn, noise, edges, probes, fsky, ctx=ctx))
    if not a.no_numpy:
        import angcov_model as acm
        t0 = time.perf_counter()
        ref = acm.cov_numpy(nodes, Cn, noise, edges, probes, fsky)
        res["numpy_einsum_s"] = time.perf_counter() - t0
        res["max_rel_diff_to_numpy"] = float(np.max(np.abs(got - ref)) / np.max(np.abs(ref)))
    res["kernel_source_sha16"] = nat.kernel_source_sha16()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
