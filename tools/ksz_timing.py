#!/usr/bin/env python3
"""Device time of the kSZ kernels on GPU 0, at the reference's default grids:
  * P_q_perp (hmg_ksz_pqperp): nk = 200, nmu = 102, at nz = 1 and 32;
  * N_vv (hmg_ksz_nvv): nmu = 102, nkL = 100, nkS = 101, lmax = 8000, at nz = 1 and 32, without and with photo-z;
  * C_ell (hmg_ksz_limber_cl): 2000 ells x 100 chi nodes on a (200 k x 32 z) table.
Inputs are uploaded once; each kernel is launched --warmup times, then timed --reps times between event records on
the context's stream.  Prints one JSON line with the median and minimum milliseconds per kernel.
With --reference, prints instead the CPU seconds of the reference's own loops for the same sizes (hmvec/ksz.py's
P_q_perp loop, Nvv_core_integral and the C_ell loop, restated as it runs them; needs no GPU).

Usage:  python tools/ksz_timing.py [--reps 20] [--warmup 3] [--reference]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SLOT0 = 100       # event slots clear of HaloModel's (0-3) and bench.py's (40 and up)
NK, NMU, NKL, NKS, NELL, LMAX = 200, 102, 100, 101, 2000, 8000


def inputs(nz):
    ks = np.geomspace(2e-3, 100.0, NK)
    mus = np.linspace(-1.0, 1.0, NMU)
    x = ks / 0.05
    Pee = np.array([1e3 * x / (1 + x ** 2.2) * (1 + 0.01 * i) for i in range(nz)])
    Pmm = np.array([2e4 * x / (1 + x ** 2.9) * (1 - 0.01 * i) for i in range(nz)])
    adotf = np.linspace(40.0, 60.0, nz)
    return ks, mus, Pee, Pmm, adotf


def nvv_inputs(nz):
    mus = np.linspace(-1.0, 1.0, NMU)
    kLs = np.geomspace(3e-3, 0.1, NKL)
    kSs = np.geomspace(0.1, 10.0, NKS)
    ls = np.arange(LMAX + 1.0)
    cls = 2e3 / (ls + 10) ** 2 + 1e-5
    chi = np.linspace(1000.0, 4000.0, nz)
    F = np.full(nz, 1e-3)
    ngg = np.full(nz, 1e4)
    Pge = np.array([1e3 / (1 + kSs ** 1.5)] * nz)
    Pgg = np.array([3e3 / (1 + kSs ** 1.8)] * nz)
    sig = 0.02 * (1 + np.linspace(0.2, 1.5, nz))
    H = np.full(nz, 3e-4)
    return mus, kLs, kSs, cls, chi, F, ngg, Pge, Pgg, sig, H


def gpu(a):
    from hmvec_amd import _native as nat
    ctx = nat.Context(0)

    def timed(name, *args):
        for _ in range(a.warmup):
            ctx.call(name, *args)
        ctx.sync()
        ms = []
        for _ in range(a.reps):
            ctx.record(SLOT0)
            ctx.call(name, *args)
            ctx.record(SLOT0 + 1)
            ms.append(ctx.elapsed_ms(SLOT0, SLOT0 + 1))
        return dict(median_ms=float(np.median(ms)), min_ms=float(np.min(ms)))

    res = {}
    for nz in (1, 32):
        ks, mus, Pee, Pmm, adotf = inputs(nz)
        d = [ctx.upload(v) for v in (ks, mus, Pee, Pmm, adotf)]
        out = ctx.empty((NK, nz))
        res[f"pqperp_nz{nz}_nk200_nmu102"] = timed("hmg_ksz_pqperp", nz, NK, NMU, *[x.ptr for x in d], out.ptr)
        assert np.all(np.isfinite(out.numpy()))
        v = nvv_inputs(nz)
        e = [ctx.upload(x) for x in v]
        o = ctx.empty((nz, NMU, NKL))
        flag = ctx.empty((1,))
        base = [nz, NMU, NKL, NKS, LMAX + 1, 0, e[0].ptr, e[1].ptr, e[2].ptr, e[3].ptr, e[4].ptr, e[5].ptr]
        tail = [e[6].ptr, e[7].ptr, e[8].ptr, None, o.ptr, flag.ptr]
        res[f"nvv_nz{nz}"] = timed("hmg_ksz_nvv", *base, None, None, *tail)
        res[f"nvv_photoz_nz{nz}"] = timed("hmg_ksz_nvv", *base, e[9].ptr, e[10].ptr, *tail)
        assert np.all(np.isfinite(o.numpy()))
    ks, _, _, _, _ = inputs(32)
    zs = np.linspace(0.1, 2.0, 32)
    P = np.abs(np.sin(ks[:, None] * 3 + zs[None, :])) + 0.1
    ells = np.linspace(100.0, 10000.0, NELL)
    chi = np.geomspace(ells / 30.0, 5000.0, 100, axis=-1)
    zn = chi / 3500.0
    f = [ctx.upload(x) for x in (ells, chi, zn, zs, ks, P)]
    cl = ctx.empty((NELL,))
    res["limber_cl_2000ells"] = timed("hmg_ksz_limber_cl", NELL, 100, 32, NK, *[x.ptr for x in f], 0, 1e-20, 7.4e12,
                                      cl.ptr)
    assert np.all(np.isfinite(cl.numpy()))
    res["kernel_source_sha16"] = nat.kernel_source_sha16()
    print(json.dumps(res))
    ctx.close()


def reference(a):
    """The reference's loops as hmvec/ksz.py runs them (Python over (z, k) / ell, numpy inside)."""
    from scipy.interpolate import RectBivariateSpline, interp1d
    trapz = getattr(np, "trapezoid", None) or np.trapz
    res = {}
    for nz in (1, 32):
        ks, mus, Pee, Pmm, adotf = inputs(nz)
        t = time.perf_counter()
        mu_mesh, k_mesh = np.meshgrid(mus, ks)
        for iz in range(nz):
            isPee = interp1d(ks, Pee[iz], bounds_error=False, fill_value=0.)
            iPmm = interp1d(ks, Pmm[iz], bounds_error=False, fill_value=0.)
            for k in ks:
                with np.errstate(invalid="ignore", divide="ignore"):
                    frac = k * (k - 2 * k_mesh * mu_mesh) * (1 - mu_mesh ** 2)
                    frac /= (k_mesh ** 2 * (k_mesh ** 2 + k ** 2 - 2 * k * k_mesh * mu_mesh))
                    kmkp = np.sqrt(k_mesh ** 2 + k ** 2 - 2 * k * k_mesh * mu_mesh)
                    igr = k_mesh ** 2 * frac
                    igr *= iPmm(k_mesh.flatten()).reshape(kmkp.shape) * isPee(kmkp.flatten()).reshape(kmkp.shape)
                trapz(trapz(np.nan_to_num(igr), ks, axis=0), mus)
        res[f"pqperp_nz{nz}_s"] = time.perf_counter() - t
        mus, kLs, kSs, cls, chi, F, ngg, Pge, Pgg, sig, H = nvv_inputs(nz)
        for photo in (False, True):
            t = time.perf_counter()
            for iz in range(nz):
                W = np.exp(-sig[iz] ** 2 * (mus[:, None] * kLs[None, :]) ** 2 / 2 / H[iz] ** 2)[..., None] \
                    if photo else 1.0
                ell = [chi[iz] * k for k in kSs]
                C = np.array([cls[int(x)] if x <= LMAX else np.inf for x in ell])
                y = kSs * ((W * Pge[iz]) ** 2 / ((W ** 2 * Pgg[iz] + ngg[iz]) * C))
                y = np.where(np.isfinite(y), y, 0)
                (np.resize(mus, (kLs.size, mus.size)).T ** -2.) * 2 * np.pi * chi[iz] ** 2 / F[iz] ** 2 / trapz(y, kSs)
            res[f"nvv{'_photoz' if photo else ''}_nz{nz}_s"] = time.perf_counter() - t
    ks, _, _, _, _ = inputs(32)
    zs = np.linspace(0.1, 2.0, 32)
    spl = RectBivariateSpline(zs, ks, (np.abs(np.sin(ks[:, None] * 3 + zs[None, :])) + 0.1).T, kx=1, ky=1, s=0)
    t = time.perf_counter()
    for ell in np.linspace(100.0, 10000.0, NELL):
        chi_int = np.geomspace(ell / 30.0, 5000.0, 100)
        z_int = chi_int / 3500.0
        integrand = np.zeros(100)
        for i, k in enumerate(ell / chi_int):
            integrand[i] = spl(z_int[i], k)[0, 0]
        trapz(integrand / chi_int ** 2 * (1 + z_int) ** 4, chi_int)
    res["limber_cl_2000ells_s"] = time.perf_counter() - t
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reference", action="store_true")
    a = ap.parse_args()
    reference(a) if a.reference else gpu(a)


if __name__ == "__main__":
    main()
