#!/usr/bin/env python3
"""CPU prototype of the quadrature rules of the projected gas / pressure profile kernels: the
same nodes, maps and formulas as hmvec_amd/csrc/kernels/gasproj.hpp in numpy (libm in place of the short device
functions), compared with the adaptive-quadrature model of tests/helpers/gas_profile_model.py over the grids of
tests/test_gpu_gas_profiles.py.  Its worst relative errors are what the gates of those tests are derived from.  No GPU.

Usage:  python tools/gas_profile_prototype.py [--nodes 64] [--smooth-nodes 32]"""
import argparse
import os
import sys

import numpy as np
from scipy.special import i0e

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(HERE, "tests", "helpers"))
import gas_profile_model as gm  # noqa: E402


def gl01(n):
    x, w = np.polynomial.legendre.leggauss(n)
    return 0.5 * (x + 1.0), 0.5 * w


def family(lr, alpha, eta, g):
    return np.exp(g * lr - eta * np.log1p(np.exp(alpha * lr)))


def core(s, alpha, gamma, eta, xcut, n=64):
    """(F, G) at s by the kernel's rule: gnfw_los and gnfw_inner."""
    u, w = gl01(n)
    F = outer = 0.0
    if s < xcut:
        um1 = (xcut - s) / s
        T = np.log1p(um1 + np.sqrt(um1 * (um1 + 2.0)))
        t = T * u
        e1 = np.exp(-t)
        e2 = e1 * e1
        lr = np.log(s) - np.log(2.0) + t + np.log1p(e2)
        r = 0.5 * s * (1.0 + e2) / e1
        fr = w * family(lr, alpha, eta, gamma + 1.0)
        F = 2.0 * (T * np.sum(fr))
        outer = T * s * np.sum(fr * r * (e1 * (1.0 - e2) / (1.0 + e2)))
    b = min(s, xcut)
    inner = b * np.sum(2.0 * u * w * family(np.log(b) + 2.0 * np.log(u), alpha, eta, gamma + 2.0))
    return F, 4.0 * (inner + outer) / (s * s)


def smooth(s, sig, alpha, gamma, eta, xcut, nseg=32, n=64):
    """F_sigma(s) by the kernel's rule: two segments of nseg nodes, s' = lo + (hi - lo) sin^2(pi u / 2)."""
    a, b = max(0.0, s - 10.0 * sig), min(xcut, s + 10.0 * sig)
    if not b > a:
        return 0.0
    c = s if s < b else 0.5 * (a + b)
    u, w = gl01(nseg)
    sg, cg = np.sin(0.5 * np.pi * u) ** 2, np.cos(0.5 * np.pi * u) ** 2
    wj = w * 0.5 * np.pi * np.sin(np.pi * u)
    total = 0.0
    for lo, hi in ((a, c), (c, b)):
        sp = np.where(np.arange(nseg) < nseg // 2, lo + (hi - lo) * sg, hi - (hi - lo) * cg)
        F = np.array([core(x, alpha, gamma, eta, xcut, n)[0] for x in sp])
        d = s - sp
        total += np.sum(wj * (hi - lo) * sp / sig ** 2 * np.exp(-0.5 * d * d / sig ** 2) * i0e(s * sp / sig ** 2) * F)
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=64)
    ap.add_argument("--smooth-nodes", type=int, default=32)
    a = ap.parse_args()
    worst = dict(sigma=0.0, mean=0.0, excess=0.0)
    for alpha, eta, gamma in ((0.88, 4.125, -0.2), (0.70, 6.04, -0.2), (1.0, 4.35, -0.3), (1.0, 6.0, -0.3)):
        for xcut in (2.0, 4.0, 20.0, 200.0):
            for s in (1e-3, 1e-2, 0.1, 0.5, 1.0, 1.9, 0.999 * xcut, xcut, 1.5 * xcut):
                F, G = core(s, alpha, gamma, eta, xcut, a.nodes)
                Fr, Gr = gm.F_proj(s, alpha, gamma, eta, xcut), gm.G_mean(s, alpha, gamma, eta, xcut)
                worst["sigma"] = max(worst["sigma"], abs(F - Fr) / Fr if Fr else abs(F))
                worst["mean"] = max(worst["mean"], abs(G - Gr) / Gr)
                worst["excess"] = max(worst["excess"], abs((G - F) - (Gr - Fr)) / abs(Gr - Fr))
    print(f"core, {a.nodes} nodes: worst relative error  sigma {worst['sigma']:.2e}  mean {worst['mean']:.2e}  "
          f"excess {worst['excess']:.2e}")
    w = 0.0
    for alpha, eta, gamma, xcut in ((0.88, 4.125, -0.2, 4.0), (1.0, 4.35, -0.3, 2.0)):
        for sig in (0.05, 0.5, 5.0):
            for s in (0.01, 0.3, 1.0, 0.95 * xcut, 1.3 * xcut):
                ref = gm.F_smooth(s, sig, alpha, gamma, eta, xcut)
                v = smooth(s, sig, alpha, gamma, eta, xcut, a.smooth_nodes, a.nodes)
                w = max(w, abs(v - ref) / abs(ref) if ref else abs(v))
    print(f"smoothing, 2 x {a.smooth_nodes} outer nodes: worst relative error {w:.2e}")


if __name__ == "__main__":
    main()
