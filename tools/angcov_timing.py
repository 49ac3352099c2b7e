#!/usr/bin/env python3
"""Device time of the Gaussian covariance of angular correlation functions on GPU 0 for a
3x2pt-like data vector: 8 fields (3 lens bins, 5 source bins), 41 probes (w of the lens bins, gamma_t of every lens
about every source bin, xi+ of 12 and xi- of 11 of the 15 source pairs), 20 bins in theta and 17 log-spaced nodes to
l_max = 2e4.  Timed separately between event records on the context's stream: the weights launch
(hmg_angcov_weights, three orders) and the contraction with its ordered combine (hmg_angcov_gaussian).  Inputs are
uploaded once; each timed window holds --batch launches.  Next to it, the wall time of the numpy einsum restatement
(tests/helpers/angcov_model.cov_numpy) on the same host, once.  Prints one JSON line.

Usage:  python tools/angcov_timing.py [--reps 10] [--warmup 2] [--batch 3]"""
import argparse
import ctypes as C
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
    d_ells, d_edges = ctx.upload(np.arange(l0, l0 + nl, dtype=np.float64)), ctx.upload(edges)
    K = [ctx.empty((nl, nt)) for _ in range(3)]
    res = dict(fields=nf, probes=np_, bins=nt, multipoles=nl, nodes=int(nodes.size))
    res["weights"] = timed(ctx, a.reps, a.warmup, a.batch, "hmg_angcov_weights", nl, nt, d_ells.ptr, d_edges.ptr,
                           *(k.ptr for k in K))
    pr = angcov.check_probes(probes, nf)
    words = np_ * (np_ + 1) // 2 * ((nl - 1) // angcov.chunk() + 1) * nt * nt
    work, cov = ctx.empty((words,)), ctx.empty((np_, nt, np_, nt))
    d_nodes, d_C, d_noise, d_pr = ctx.upload(nodes), ctx.upload(Cn), ctx.upload(noise), ctx.upload_int32(pr)
    res["gaussian"] = timed(ctx, a.reps, a.warmup, a.batch, "hmg_angcov_gaussian", nf, nodes.size, d_nodes.ptr, d_C.ptr,
                            d_noise.ptr, l0, nl, nt, d_edges.ptr, np_, pr.ctypes.data_as(C.POINTER(C.c_int)), d_pr.ptr,
                            4.0 * np.pi * fsky, *(k.ptr for k in K), words, work.ptr, cov.ptr)
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
