"""Block order of the batched mass integrals, asked without a GPU.

For a grid of the benchmark's kind (default Config 3: 32 x 512 x 4096, nxs = 5000, xmax = 20) this takes the oracle's
NFW scale radius r_s and concentration c and the Battaglia rows' length scale r_200c / 2, applies the two skip rules of
power_batch_kernel with the kernel's own expressions -
    Battaglia tensor: nconst[row] = #{k < kt_1 / (r_g (1+z))}           a 128-k tile is loaded when nconst[row] < kend
    NFW tensor:       nser[row]   = #{(1+c) (k r_s (1+z)) <= 0.8}       a 128-k tile is loaded when nser[row]  < kend
- and prints: the bins loaded per tile (mean over z), the loaded (bin, tensor) tiles per class of id % 8 (blocks are dealt
round-robin over the 8 XCDs: observed, not a contract) for each order of hmvec_amd/csrc/kernels/pb_map.hpp, and the end
of a list-scheduling model of the launch: cost of a workgroup = alpha loads + beta nm + gamma series-evaluated bins, 64
slots per XCD, ids taken in order by the first free slot of their XCD.
What the GPU said to this model (profiles/r11/pb_order_ab.txt): a workgroup takes about 60 us whatever its tile - 512
bins at one dependent scalar round trip each - so the defaults below (beta from that, alpha from the 10 us that loading
workgroups lose when the whole chip loads) put the three orders at 136-138, 128 and 132 us.  With constants that
charge the loads (--alpha 0.1 --beta 0.12 --gamma 0.02) the model promises 65-90 us of 300 from the order; the launch
gave 10 of 139, and to the interleaved order, not to heavy-first.  That gain comes from what the model leaves out:
workgroups that load slow each other down, and in the interleaved order fewer of them are on the chip at a time.
For tools only: nothing under hmvec_amd/ imports oracle/.
Usage: python tools/pb_order_model.py [--nz 32 --nm 512 --nk 4096 --nxs 5000 --xmax 20 --alpha A --beta B --gamma G]"""
import argparse
import heapq
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)

TILE = 128


def pb_map(order, i, ntile, nz):
    """hmvec_amd/csrc/kernels/pb_map.hpp"""
    if order == 0:
        return i % ntile, i // ntile
    s, z = i // nz, i % nz
    if order == 1:
        return ntile - 1 - s, z
    return (s >> 1 if s & 1 else ntile - 1 - (s >> 1)), z


def skip_counts(nz, nm, nk, nxs, xmax):
    import hmvec_amd as hm
    from hmvec_amd.params import default_params
    from oracle import hmref
    p = dict(default_params)
    zs, ms, ks = np.linspace(0.01, 3.0, nz), np.geomspace(2e10, 1e17, nm), np.geomspace(1e-4, 100, nk)
    cos = hm.Cosmology(dict(p), accuracy="low", engine="analytic")
    ksig = np.geomspace(p["sigma2_kmin"], p["sigma2_kmax"], p["sigma2_numks"])
    ci = hmref.CosmoInputs(h=cos.h, omm0=cos.omm0, ombh2=p["ombh2"], rho_crit_0=float(cos.rho_critical_z(0.0)),
                           rho_crit_zs=cos.rho_critical_z(zs), Pzk=None, sPzk=None, ks_sigma2=ksig, h_of_z_zs=cos.h_of_z(zs))
    cs = hmref.concentration(ms, zs, ci.h, p, "vir")
    rss = hmref.rvir(ci, ms, zs, "vir") / cs
    d1 = hmref.delta_rho_of_mdef(ci, zs, "vir")
    m200c = hmref.mdelta_from_mdelta(ms, cs, d1, 200.0 * ci.rho_crit_zs)
    rgs = hmref.lagrangian_radius(m200c, ci.rho_crit_zs[:, None], 200.0) / 2.0
    z1 = 1.0 + zs[:, None]
    # NFW: the kernel's products in its order, opc * ((k * rs) * z1) <= 0.8; ks ascending, so the count is a prefix
    nser = np.empty((nz, nm), dtype=np.int64)
    for iz in range(nz):
        x = (1.0 + cs[iz])[:, None] * ((ks[None, :] * rss[iz][:, None]) * z1[iz])
        nser[iz] = np.sum(x <= 0.8, axis=1)
    # Battaglia: kt_1 of the sine transform (oracle.hmref.sine_transform), left fill below kt_1 / (r_g (1+z))
    step = (xmax - xmax / nxs) / nxs
    kt1 = 2 * np.pi / (nxs * step)
    klo = kt1 / rgs / z1
    nconst = np.stack([np.searchsorted(ks, klo[iz], side="left") for iz in range(nz)])
    return nconst, nser


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nz", type=int, default=32)
    ap.add_argument("--nm", type=int, default=512)
    ap.add_argument("--nk", type=int, default=4096)
    ap.add_argument("--nxs", type=int, default=5000)
    ap.add_argument("--xmax", type=float, default=20.0)
    ap.add_argument("--alpha", type=float, default=0.01, help="us per loaded (bin, tensor) tile")
    ap.add_argument("--beta", type=float, default=0.115, help="us per mass bin walked")
    ap.add_argument("--gamma", type=float, default=0.0, help="us per series-evaluated bin")
    a = ap.parse_args()
    nz, nm, nk = a.nz, a.nm, a.nk
    nconst, nser = skip_counts(nz, nm, nk, a.nxs, a.xmax)
    ntile = (nk + TILE - 1) // TILE
    kend = np.minimum(nk, (np.arange(ntile) + 1) * TILE)
    lb = nconst[:, :, None] < kend[None, None, :]            # [z][m][tile]: the Battaglia tile is loaded
    ln = nser[:, :, None] < kend[None, None, :]
    mono = bool(np.all(np.diff(lb.astype(int), axis=1) >= 0) and np.all(np.diff(ln.astype(int), axis=1) >= 0))
    print(f"grid {nz} x {nm} x {nk}, {ntile} tiles of {TILE} k; loaded is monotone in m: {mono}")
    print("bins loaded per tile, mean over z")
    print("Battaglia  " + " ".join(f"{v:.0f}" for v in lb.sum(1).mean(0)))
    print("NFW        " + " ".join(f"{v:.0f}" for v in ln.sum(1).mean(0)))
    loads = (lb.sum(1) + ln.sum(1)).astype(float)            # [z][tile]
    series = (~ln).sum(1).astype(float)
    cost = a.alpha * loads + a.beta * nm + a.gamma * series
    print(f"tiles that load nothing: {int(np.sum(loads.max(0) == 0))} of {ntile}; whole tensor bytes of the heaviest tile: "
          f"{2 * nm * TILE * 8 / 2 ** 20:.2f} MiB")
    print(f"model: alpha {a.alpha} beta {a.beta} gamma {a.gamma} ; sum of all work / 512 slots {cost.sum() / 512:.1f} us; "
          f"longest workgroup {cost.max():.1f} us")
    for order in (0, 1, 2):
        per = np.zeros(8)
        free = [[0.0] * 64 for _ in range(8)]
        for q in free:
            heapq.heapify(q)
        ends = np.zeros(8)
        for i in range(ntile * nz):
            t, z = pb_map(order, i, ntile, nz)
            x = i % 8
            per[x] += loads[z, t]
            e = heapq.heappop(free[x]) + cost[z, t]
            heapq.heappush(free[x], e)
            ends[x] = max(ends[x], e)
        print(f"O{order}: loaded tiles per class of id % 8: " + " ".join(f"{v:.0f}" for v in sorted(per)) +
              f"  (max / min {per.max() / max(per.min(), 1):.2f}); model end per class {ends.min():.0f}-{ends.max():.0f} us")


if __name__ == "__main__":
    main()
