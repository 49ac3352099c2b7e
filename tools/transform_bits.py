#!/usr/bin/env python3
"""Bits of the four transforms of tabulated spectra (hmg_xi_transform, hmg_hankel_transform, hmg_angular_transform,
hmg_xi_multipoles; DESIGN.md sections 13, 14, 22, 24) of the working-tree library against those of the committed one
(hmvec_amd/libhmgrid_base.so, tools/ab_build.sh).  Two fresh child processes, each under its own time limit: the first
loads the base library (HMG_LIB_PATH) and writes every output to FILE, the second loads the working-tree library and
compares with np.array_equal; the tool stops at the first non-zero exit status.  Grids of nk = 2, 33, 258, 1030 reaching
k = 1e4, six radii (a full tile and a partial one) from 0.003 to 2e5, so that k R and the panels' theta fall on both sides
of every branch (0.5, 2, 3, 4, 5, 6, 2^30); every subset of the orders; contiguous rows and the (rows, nk, 3) layout.
A proof for one change of the kernels, not a test: recorded bits would pin the compiler.

Usage:  tools/ab_build.sh && python tools/transform_bits.py FILE"""
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT_S = 120


def outputs():
    sys.path.insert(0, HERE)
    from hmvec_amd import _native as nat
    ctx = nat.Context(0)
    rng = np.random.default_rng(0)
    n, nz = 2, 3
    rows = n * nz
    R, chi = np.array([0.003, 0.05, 0.4, 3.0, 40.0, 2e5]), np.array([0.5, 1.0, 3.0])
    d_R, d_chi = ctx.upload(R), ctx.upload(chi)
    o = [ctx.empty((rows, R.size)) for _ in range(3)]
    res = {}
    for nk in (2, 33, 258, 1030):
        ks = np.geomspace(1e-3, 1e4, nk)
        P = rng.uniform(0.5, 2.0, (3, rows, 1)) * (2e4 * (ks / 0.02) / (1 + (ks / 0.02) ** 2) ** 1.9)     # (3, rows, nk)
        d_ks, d_P = ctx.upload(ks), ctx.upload(P)
        d_S = ctx.upload(np.ascontiguousarray(np.moveaxis(P, 0, -1)))                                   # (rows, nk, 3)
        head = (rows, nk, R.size, d_ks.ptr)
        for mask in range(1, 8):                                      # bit i: the order 2 i is asked for
            outs = tuple(o[i].ptr if mask >> i & 1 else None for i in range(3))
            keep = lambda tag: res.update({f"{tag}_nk{nk}_orders{mask}_out{i}": o[i].numpy()      # noqa: E731
                                           for i in range(3) if mask >> i & 1})
            if mask == 1:
                ctx.call("hmg_xi_transform", *head, d_P.ptr, d_R.ptr, outs[0])
                keep("xi")
            if mask < 4:
                ctx.call("hmg_hankel_transform", *head, d_P.ptr, d_R.ptr, *outs[:2])
                keep("hankel")
            ctx.call("hmg_angular_transform", n, nz, nk, R.size, d_ks.ptr, d_P.ptr, d_chi.ptr, d_R.ptr, *outs)
            keep("angular")
            for tag, p0, step, strides in (("xipoles", d_P.ptr, 8 * rows * nk, (nk, 1)),
                                           ("xipoles_strided", d_S.ptr, 8, (3 * nk, 3))):
                ctx.call("hmg_xi_multipoles", *head, *(p0 + step * i for i in range(3)), *strides, d_R.ptr, *outs)
                keep(tag)
    ctx.close()
    return res


def main():
    if len(sys.argv) == 2:
        for mode, lib in (("write", os.path.join(HERE, "hmvec_amd", "libhmgrid_base.so")), ("compare", None)):
            env = {k: v for k, v in os.environ.items() if k != "HMG_LIB_PATH"}
            if lib:
                env["HMG_LIB_PATH"] = lib
            child = ["timeout", "-k", "10", str(LIMIT_S), sys.executable, os.path.abspath(__file__), sys.argv[1], mode]
            rc = subprocess.run(child, env=env).returncode
            if rc:
                sys.exit(f"{mode}: exit status {rc}")
        return
    path, mode = sys.argv[1:]
    res = outputs()
    if mode == "write":
        with open(path, "wb") as f:
            np.savez(f, **res)
        print(f"wrote {len(res)} arrays to {path}")
        return
    with np.load(path) as ref:
        bad = [k for k in res if not np.array_equal(res[k], ref[k])] + [k for k in ref.files if k not in res]
    print(f"{len(res) - len(bad)} of {len(res)} arrays match {path} bit for bit" + "".join(f"\n  differs: {k}" for k in bad))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
