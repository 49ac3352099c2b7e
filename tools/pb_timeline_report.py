"""Summary of one workgroup timeline of power_batch_kernel, as the instrumented build of profiles/r11/pb_timeline.patch
writes it: lines `id t_out xcc tile z`, exit times in ticks of the 100 MHz wall clock from the first exit.  The build
stamps exits only (an entry stamp changes the kernel's code and doubles its time: see the patch), so entries are
RECONSTRUCTED: blocks are dispatched in id order, block b goes to the XCD of b % 8 (checked below against the recorded
XCD ids) and takes the slot of that XCD that frees first; the first `slots` blocks enter at the origin.  The origin is
the last exit minus the duration of the launch, which the caller passes (the launch's average in a kernel trace of the
plain build).
Prints: end time per XCD, reconstructed durations of the workgroups of some tiles, the longest workgroup, from when on
fewer than half / a quarter of the slots are busy, and the mean number of busy workgroups over the last tenth.
Usage: python tools/pb_timeline_report.py timeline.txt launch_us [slots, default 512]"""
import heapq
import sys

import numpy as np


def main():
    path, launch_us = sys.argv[1], float(sys.argv[2])
    slots = int(sys.argv[3]) if len(sys.argv) > 3 else 512
    head = open(path).readline().strip()
    a = np.loadtxt(path, comments="#", dtype=np.int64).reshape(-1, 5)
    xcc, tile = a[:, 2], a[:, 3]
    t_out = a[:, 1] * 0.01                                   # us from the first exit
    t_out = t_out - t_out.max() + launch_us                  # us from the start of the launch
    n = len(a)
    same = float(np.mean(xcc[8:] == xcc[:-8])) if n > 8 else 1.0
    print(f"{head}\n{n} workgroups, {slots} slots, launch {launch_us:.1f} us (given); first exit at {t_out.min():.1f} us")
    print(f"blocks b and b+8 on one XCD: {100 * same:.1f} % of the pairs; XCD of the first 8 ids: {xcc[:8].tolist()}")
    # entries: per XCD, ids in order take the slot that frees first
    t_in = np.zeros(n)
    per = slots // 8
    free = {int(x): [0.0] * per for x in np.unique(xcc)}
    for i in range(n):
        q = free[int(xcc[i])]
        t_in[i] = heapq.heappop(q)
        heapq.heappush(q, t_out[i])
    dur = t_out - t_in
    print(f"sum of workgroup times / slots {dur.sum() / slots:.1f} us; longest workgroup {dur.max():.1f} us (tile {tile[dur.argmax()]}, "
          f"entry {t_in[dur.argmax()]:.1f} us)")
    print("XCD   workgroups   last exit us   sum of workgroup times / slots of the XCD us   mean tile")
    ends = []
    for x in np.unique(xcc):
        s = xcc == x
        ends.append(t_out[s].max())
        print(f"{x:3d}   {s.sum():10d}   {t_out[s].max():12.1f}   {dur[s].sum() / per:20.1f}   {tile[s].mean():26.1f}")
    print(f"XCD end times: {min(ends):.1f} - {max(ends):.1f} us (spread {max(ends) - min(ends):.1f})")
    print("tile   workgroups   duration us min / median / max   mean entry us   (entries reconstructed)")
    tmax = int(tile.max())
    for t in sorted(set([0, 1, tmax // 2, tmax - 1, tmax])):
        s = tile == t
        if s.any():
            print(f"{t:4d}   {s.sum():10d}   {dur[s].min():8.1f} {np.median(dur[s]):8.1f} {dur[s].max():8.1f}   {t_in[s].mean():12.1f}")
    ev = np.concatenate([np.stack([t_in, np.ones(n)], 1), np.stack([t_out, -np.ones(n)], 1)])
    ev = ev[np.lexsort((ev[:, 1], ev[:, 0]))]
    busy = np.cumsum(ev[:, 1])
    for frac in (0.5, 0.25):
        at = np.nonzero(busy >= frac * slots)[0]
        t_last = ev[at[-1] + 1, 0] if at.size and at[-1] + 1 < len(ev) else 0.0
        print(f"fewer than {frac:.2f} of the slots busy from {t_last:.1f} us to the end: {launch_us - t_last:.1f} us = "
              f"{100 * (launch_us - t_last) / launch_us:.0f} % of the launch")
    k90 = np.searchsorted(ev[:, 0], 0.9 * launch_us)
    w = np.diff(np.append(ev[k90:, 0], launch_us))
    prev = busy[k90 - 1] if k90 > 0 else 0
    mean_busy = float((np.sum(busy[k90:] * w) + prev * (ev[k90, 0] - 0.9 * launch_us if k90 < len(ev) else 0)) / (0.1 * launch_us))
    print(f"last 10 % of the launch ({0.9 * launch_us:.1f} - {launch_us:.1f} us): {mean_busy:.0f} workgroups busy on average")
    last_entry = t_in.max()
    print(f"last entry at {last_entry:.1f} us: the launch runs {launch_us - last_entry:.1f} us after its last dispatch")


if __name__ == "__main__":
    main()
