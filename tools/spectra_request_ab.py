"""Two trees of this repository side by side on the recording stand-in for the library (tests/helpers/recording_context.py):
do the public spectra doors of HaloModel make the same native calls, print the same lines and leave the same cache keys,
and what does a request cost on the host?  No GPU and no built library are needed.

    python tools/spectra_request_ab.py OTHER_TREE [--rounds N] [--repeats N] [--out FILE]

OTHER_TREE is a checkout of the commit to compare with (say `git worktree add ../parent HEAD~1`).  Every public call is
one case; the two sides are compared call by call after one normalisation: within one public call, an hmg_prefix_fill of
a pointer that the same call has filled before is dropped (the library makes it a no-op).  Host cost: the median wall
time of a cache-miss get_power("nfw") and of power_device_batch(PAIRS) on the helper's model, the whole measurement
repeated `rounds` times per tree in turn, each in a process of its own."""
import argparse
import contextlib
import ctypes as C
import gc
import hashlib
import io
import itertools
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------- worker side
def plain(x, nat):
    """A native argument as plain data: what it points at instead of where that lives on the host."""
    if type(x).__name__ == "CArgObject":
        return plain(x._obj, nat)
    if isinstance(x, nat.PowerBatchDesc):
        d = {name: plain(getattr(x, name), nat) for name, typ in x._fields_ if not name.startswith("h_")}
        d["h_tr"] = [plain(x.h_tr[i], nat) for i in range(x.ntr)]
        for name in ("h_pair_a", "h_pair_b", "h_P1h", "h_P2h"):
            d[name] = [getattr(x, name)[i] for i in range(x.npairs)]
        return d
    if isinstance(x, C.Structure):
        return {name: plain(getattr(x, name), nat) for name, _ in x._fields_}
    if isinstance(x, C._Pointer):
        return plain(x.contents, nat) if x else None
    if isinstance(x, C.Array):
        return [plain(v, nat) for v in x]
    if isinstance(x, C._SimpleCData):
        return x.value
    if isinstance(x, bytes):
        return x.hex()
    return x


def render(nat):
    def fn(name, args):
        args = list(args)
        if name == "hmg_memcpy_h2d":          # (handle, dst, host src, bytes): the data, not its address
            args[2] = hashlib.sha256(C.string_at(args[2], args[3])).hexdigest()[:16]
        elif name == "hmg_memcpy_d2h":        # (handle, host dst, src, bytes)
            args[1] = "host"
        return [plain(a, nat) for a in args]
    return fn


def record(tree):
    sys.path[:0] = [tree, os.path.join(tree, "tests", "helpers")]
    import numpy as np
    import recording_context as rc
    import hmvec_amd as hm
    from hmvec_amd import _native as nat
    from hmvec_amd import ksz
    gc.disable()          # (a collection would put hmg_free calls wherever it happens to run)
    nz = rc.ZS.size
    mth = np.full(nz, 10 ** 10.5)
    cases = []

    def variant(which, small, hints):
        os.environ.pop("HMG_NO_HINTS", None)
        if not hints:
            os.environ["HMG_NO_HINTS"] = "1"
        hm.HaloModel._SMALL_GRID_BYTES = (32 << 20) if small else 0
        ctx = rc.recording_context(render(nat))
        h = rc.build_model(ctx, nfw_numeric=(which == "numeric"))        # nfw, electron, y, g
        if which in ("second", "many"):
            h.add_hod("g2", mthresh=mth * 3, corr="min")
            h.add_battaglia_pres_profile("y2", param_override={"battaglia_pres_gamma": -0.2})
        if which in ("central", "many"):
            h.add_hod("gc", mthresh=mth * 2, central_profile_name="electron")
        if which == "both":
            h.add_hod("electron", mthresh=mth, ignore_existing=True)    # an HOD and a matter profile of one name
        if which == "hand":
            h.uk_profiles["good"] = np.full((nz, rc.MS.size, rc.KS.size), 0.5)
            h.uk_profiles["broken"] = np.ones((nz, rc.MS.size, rc.KS.size // 2))
            h.add_hod("gb", mthresh=mth, satellite_profile_name="broken")
        return ctx, h

    def door(tag, ctx, h, fn):
        n = len(ctx.lib.calls)
        out, err = io.StringIO(), None
        try:
            with contextlib.redirect_stdout(out):
                fn()
        except Exception as e:
            err = type(e).__name__
        cases.append({"case": tag, "calls": [[name, a] for name, a in ctx.lib.calls[n:]], "stdout": out.getvalue(),
                      "raised": err, "cache": sorted(k for k, v in h._pcache.items() if v[0] == h._version)})

    def requeue(h):
        """Every stage of a pass again: the next request finds them queued."""
        h.init_mass_function(rc.MS)
        h.add_nfw_profile("nfw", ignore_existing=True)
        h.add_battaglia_profile("electron", ignore_existing=True)
        h.add_hod("g", mthresh=mth, ignore_existing=True)

    b1, b2 = np.linspace(1, 2, nz), np.linspace(2, 3, nz)
    for which, small, hints in [(w, s, True) for w in ("readme", "second", "central", "both", "many", "hand", "numeric")
                                for s in (True, False)] + [("readme", True, False), ("numeric", True, False)]:
        ctx, h = variant(which, small, hints)
        tag = f"{which}/{'small' if small else 'large'}/{'hints' if hints else 'nohints'}"
        names = list(dict.fromkeys(itertools.chain(h.hods, h.uk_profiles, h.pk_profiles))) + ["nope"]
        pairs = [(a, b) for a in names for b in names if "nope" not in (a, b) or a == b]

        def D(what, fn):
            door(f"{tag}: {what}", ctx, h, fn)
        for a, b in pairs:          # each pair as the first request after a change of state, then from the cache
            h._bump()
            D(f"miss get_power_1halo({a},{b})", lambda: h.get_power_1halo(a, b))
            D(f"hit get_power_2halo({a},{b})", lambda: h.get_power_2halo(a, b))
            D(f"hit get_power({a},{b})", lambda: h.get_power(a, b))
        h._bump()
        for a, b in pairs:          # ... and with whatever the requests before it have left in the cache
            D(f"get_power({a},{b})", lambda: h.get_power(a, b))
            D(f"get_power_2halo({a},{b})", lambda: h.get_power_2halo(a, b))
        D("get_power(nfw) name2=None", lambda: h.get_power("nfw"))
        for a, b in pairs:
            for want in (("1h", "2h"), ("1h",), ("2h",)):
                D(f"power_device({a},{b},{want})", lambda: h.power_device(a, b, want=want))
            D(f"power_device({a},{b},b1,b2)", lambda: h.power_device(a, b, b1, b2))
            D(f"get_power_2halo({a},{b},b1)", lambda: h.get_power_2halo(a, b, b1_in=b1))
            D(f"get_power_2halo({a},{b},b1,b2,verbose)", lambda: h.get_power_2halo(a, b, verbose=True, b1_in=b1, b2_in=b2))
            D(f"get_power({a},{b},b1,b2)", lambda: h.get_power(a, b, b1=b1, b2=b2))
            D(f"get_power({a},{b},verbose)", lambda: h.get_power(a, b, verbose=True))
            D(f"two_halo_terms({a},{b})", lambda: h.two_halo_terms(a, b))
            D(f"ksz._power_on_device({a},{b})", lambda: ksz._power_on_device(h, a, b))
        real = [n for n in names if n not in ("nope", "broken", "gb")]
        batches = [rc.PAIRS, [("g", "nfw"), ("nfw", "g"), ("g", "g"), ("g", "nfw")], [("nfw", None), ("y", "nfw"), ("nfw", "y")],
                   [(a, b) for a in real[:3] for b in real[:3]], [(a, a) for a in real], [(real[-1], real[0]), (real[0], real[-1])],
                   [(a, b) for a in real[:2] for b in real[-2:]], [("nfw", "nope")], [("nfw", names[-2])]]
        for i, bt in enumerate(batches):
            D(f"power_device_batch #{i}", lambda: h.power_device_batch(bt))
            D(f"get_power_all #{i}", lambda: h.get_power_all(bt))
            D(f"spectra_block #{i}", lambda: h.spectra_block(bt).compute())
        for what, fn in [("get_power(nfw)", lambda: h.get_power("nfw")), ("get_power(g,electron)", lambda: h.get_power("g", "electron")),
                         ("get_power_1halo(y)", lambda: h.get_power_1halo("y")), ("get_power_all", lambda: h.get_power_all(rc.PAIRS)),
                         ("power_device_batch", lambda: h.power_device_batch(rc.PAIRS)),
                         ("power_device(g,nfw)", lambda: h.power_device("g", "nfw"))]:
            requeue(h)
            D(f"stages queued, {what}", fn)
        ctx.handle = None
    json.dump(cases, sys.stdout)


def cost(tree, repeats):
    sys.path[:0] = [tree, os.path.join(tree, "tests", "helpers")]
    import recording_context as rc
    ctx = rc.recording_context(lambda name, args: None)
    h = rc.build_model(ctx)
    out = {}
    for what, before, fn in [("get_power_miss", h._bump, lambda: h.get_power("nfw")),
                             ("power_device_batch", lambda: None, lambda: h.power_device_batch(rc.PAIRS))]:
        ts = []
        for _ in range(repeats + 20):
            before()
            del ctx.lib.calls[:]
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        out[what] = statistics.median(ts[20:]) * 1e6
    ctx.handle = None
    json.dump(out, sys.stdout)


# ---------------------------------------------------------------------------------------------------- comparing side
def worker(mode, tree, *more):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), mode, tree, *more], check=True, capture_output=True,
                       text=True, env={**os.environ, "PYTHONDONTWRITEBYTECODE": "1"})
    return json.loads(r.stdout)


def normalised(calls):
    filled, out = set(), []
    for name, args in calls:
        if name == "hmg_prefix_fill":
            if args[1] in filled:
                continue
            filled.add(args[1])
        out.append([name, args])
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("other")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--repeats", type=int, default=300)
    ap.add_argument("--out")
    a = ap.parse_args()
    other = os.path.abspath(a.other)
    theirs, ours = worker("--record", other), worker("--record", HERE)
    lines = [f"cases (public calls) compared: {len(ours)} (other tree: {len(theirs)})"]
    diffs = dropped = 0
    for t, o in itertools.zip_longest(theirs, ours, fillvalue={}):
        tn, on = normalised(t.get("calls", [])), normalised(o.get("calls", []))
        dropped += len(t.get("calls", [])) - len(tn)
        same = (tn == on and all(t.get(k) == o.get(k) for k in ("case", "stdout", "raised", "cache")))
        if not same:
            diffs += 1
            if diffs <= 20:
                lines.append(f"DIFFERENT {o.get('case')}: other {[n for n, _ in tn]} raised {t.get('raised')} / "
                             f"this {[n for n, _ in on]} raised {o.get('raised')}")
    ncalls = sum(len(o["calls"]) for o in ours)
    lines.append(f"native calls of this tree: {ncalls}; repeated hmg_prefix_fill dropped from the other tree: {dropped}; "
                 f"cases that raise: {sum(1 for o in ours if o['raised'])}")
    lines.append(f"differences after normalisation: {diffs}")
    runs = {"other": [], "this": []}
    for _ in range(a.rounds):
        runs["other"].append(worker("--cost", other, str(a.repeats)))
        runs["this"].append(worker("--cost", HERE, str(a.repeats)))
    lines.append(f"host cost on the recording stand-in, median of {a.repeats} calls, {a.rounds} rounds per tree in turn [us]:")
    for what in runs["this"][0]:
        for side in ("other", "this"):
            v = sorted(r[what] for r in runs[side])
            lines.append(f"  {what:20s} {side:5s} median {statistics.median(v):7.1f}  range {v[0]:7.1f} .. {v[-1]:7.1f}")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    return 1 if diffs else 0


if __name__ == "__main__":
    if sys.argv[1:2] == ["--record"]:
        record(sys.argv[2])
    elif sys.argv[1:2] == ["--cost"]:
        cost(sys.argv[2], int(sys.argv[3]))
    else:
        sys.exit(main())
