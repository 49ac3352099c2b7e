"""hmvec_amd/spectra.py and the facade's use of it, without a GPU: how a name resolves, the batch rule, the rider rule and
the pair bookkeeping as tables, the native calls of whole requests against a recording stand-in for the library
(tests/helpers/recording_context.py), and the failure path of a cached request.  The literal expectations of the rule
tables and the call sequences were recorded with the same helper on the facade as it was before these decisions moved
into spectra.py (the rider rule and the batch rule of halomodel.py)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import recording_context as rc  # noqa: E402

from hmvec_amd import _native as nat  # noqa: E402
from hmvec_amd import spectra  # noqa: E402


# What is registered, in the order the facade iterates it (hods, then uk_profiles, then pk_profiles).  hods: name ->
# (satellite profile, central profile); wrong: hand-assigned uk_profiles entries that are not in the model's shape.
REGISTRIES = {
    "readme": dict(hods={"g": ("nfw", None)}, uk=["nfw", "electron"], pk=["y"]),
    "numeric": dict(hods={"g": ("nfw", None)}, uk=["nfw", "electron"], pk=["y"], numeric=True),
    "many": dict(hods={"g": ("nfw", None), "g2": ("nfw", None), "gc": ("nfw", "electron")}, uk=["nfw", "electron"], pk=["y", "y2"]),
    "both": dict(hods={"g": ("nfw", None), "electron": ("nfw", None)}, uk=["nfw", "electron"], pk=["y"]),
    "hand": dict(hods={"g": ("nfw", None), "gb": ("broken", None)}, uk=["nfw", "electron", "good", "broken"], pk=["y"],
                 wrong=["broken"]),
}
MTH = 10 ** 10.5


def build(reg, ctx):
    """The model of a registry on a recording context."""
    import hmvec_amd as hm
    nz, nm, nk = rc.ZS.size, rc.MS.size, rc.KS.size
    h = hm.HaloModel(rc.ZS, rc.KS, ms=rc.MS, accuracy="low", engine="analytic", ctx=ctx, nfw_numeric=reg.get("numeric", False))
    for name in reg["uk"][1:]:
        if name == "electron":
            h.add_battaglia_profile(name)
        else:
            h.uk_profiles[name] = np.full((nz, nm, nk // 2 if name in reg.get("wrong", ()) else nk), 0.5)
    for name in reg["pk"]:
        h.add_battaglia_pres_profile(name)
    for name, (sat, cen) in reg["hods"].items():
        h.add_hod(name, mthresh=np.full(nz, MTH), satellite_profile_name=sat, central_profile_name=cen, ignore_existing=True)
    return h


KIND = "mhp"          # hmg_tracer kinds: TRACER_MATTER, TRACER_HOD, TRACER_PRESSURE


def render(name, args):
    """What the literal sequences keep of a call."""
    if name in ("hmg_power", "hmg_power_2halo_terms"):
        ta, tb = args[4]._obj, args[5]._obj
        what = KIND[ta.kind] + KIND[tb.kind]
        if name == "hmg_power":
            what += " " + "+".join(t for t, p in zip(("1h", "2h"), args[-2:]) if p)
        return f"{name} {what}" + (" bias" if ta.d_bias_override or tb.d_bias_override else "")
    if name == "hmg_power_batch_run":
        d = args[4]._obj
        return (f"{name} {''.join(KIND[d.h_tr[i].kind] for i in range(d.ntr))} "
                f"{','.join(f'{d.h_pair_a[i]}{d.h_pair_b[i]}' for i in range(d.npairs))}" + (" prepared" if args[5] else ""))
    if name == "hmg_prefix_fill":
        return (name, args[1])
    return name


def run(h, step):
    """One step of SEQUENCES on a model; returns its calls, with the tensor's name in place of a filled pointer and without
    the repeated fills of a pointer (no-ops in the library)."""
    ctx = h._ctx()
    n = len(ctx.lib.calls)
    if step == ("requeue",):
        h.init_mass_function(rc.MS)
        h.add_nfw_profile("nfw", ignore_existing=True)
        h.add_battaglia_profile("electron", ignore_existing=True)
        n = len(ctx.lib.calls)
    else:
        getattr(h, step[0])(*step[1:])
    tensor = {dd.dev(nm_, fill=False).ptr: nm_ for dd in (h.uk_profiles, h.pk_profiles) for nm_ in dd}
    out = []
    for _, c in ctx.lib.calls[n:]:
        c = c if isinstance(c, str) else f"{c[0]} {tensor[c[1]]}"
        if c != "hmg_free" and not (c.startswith("hmg_prefix_fill") and c in out):      # (when a block is released is the collector's business)
            out.append(c)
    return out


# (registry, small-grid rule, request) -> the pairs of its batch, '' where it takes the one-pair kernel
RIDERS = [
    ('readme', True, 'nfw', 'nfw', 'nfw:nfw nfw:g nfw:electron nfw:y g:g g:electron g:y electron:electron electron:y y:y'),
    ('readme', True, 'electron', 'electron', 'electron:electron electron:g electron:nfw electron:y g:g g:nfw g:y nfw:nfw nfw:y y:y'),
    ('readme', True, 'y', 'y', 'y:y y:g y:nfw y:electron g:g g:nfw g:electron nfw:nfw nfw:electron electron:electron'),
    ('readme', True, 'g', 'g', 'g:g g:nfw g:electron g:y nfw:nfw nfw:electron nfw:y electron:electron electron:y y:y'),
    ('readme', True, 'g', 'electron', 'g:g g:electron g:nfw g:y electron:electron electron:nfw electron:y nfw:nfw nfw:y y:y'),
    ('readme', True, 'electron', 'g', 'electron:electron electron:g electron:nfw electron:y g:g g:nfw g:y nfw:nfw nfw:y y:y'),
    ('readme', True, 'y', 'nfw', 'y:y y:nfw y:g y:electron nfw:nfw nfw:g nfw:electron g:g g:electron electron:electron'),
    ('readme', False, 'nfw', 'nfw', 'nfw:nfw nfw:g g:g'),
    ('readme', False, 'electron', 'electron', 'electron:electron'),
    ('readme', False, 'y', 'y', 'y:y'),
    ('readme', False, 'g', 'g', 'g:g g:nfw nfw:nfw'),
    ('readme', False, 'g', 'electron', 'g:g g:electron g:nfw electron:electron electron:nfw nfw:nfw'),
    ('readme', False, 'electron', 'g', 'electron:electron electron:g electron:nfw g:g g:nfw nfw:nfw'),
    ('readme', False, 'y', 'nfw', 'y:y y:nfw y:g nfw:nfw nfw:g g:g'),
    ('many', True, 'nfw', 'nfw', 'nfw:nfw nfw:g nfw:g2 nfw:gc g:g g2:g2 gc:gc'),
    ('many', True, 'electron', 'electron', 'electron:electron electron:g electron:g2 electron:gc g:g g2:g2 gc:gc'),
    ('many', True, 'y', 'y', 'y:y y:g y:g2 y:gc g:g g2:g2 gc:gc'),
    ('many', True, 'y2', 'y2', 'y2:y2 y2:g y2:g2 y2:gc g:g g2:g2 gc:gc'),
    ('many', True, 'g', 'g', 'g:g g:nfw g2:g2 g2:nfw gc:gc gc:nfw nfw:nfw'),
    ('many', True, 'g2', 'g2', 'g2:g2 g2:nfw g:g g:nfw gc:gc gc:nfw nfw:nfw'),
    ('many', True, 'gc', 'gc', 'gc:gc gc:nfw g:g g:nfw g2:g2 g2:nfw nfw:nfw'),
    ('many', True, 'g', 'g2', ''),
    ('many', True, 'y', 'y2', ''),
    ('many', True, 'g', 'electron', 'g:g g:electron electron:electron electron:g2 electron:gc g2:g2 gc:gc'),
    ('many', True, 'gc', 'y', 'gc:gc gc:y y:y y:g y:g2 g:g g2:g2'),
    ('many', True, 'y2', 'g2', 'y2:y2 y2:g2 y2:g y2:gc g2:g2 g:g gc:gc'),
    ('many', True, 'gc', 'g', ''),
    ('many', False, 'nfw', 'nfw', 'nfw:nfw nfw:g nfw:g2 g:g g2:g2'),
    ('many', False, 'electron', 'electron', 'electron:electron'),
    ('many', False, 'y', 'y', 'y:y'),
    ('many', False, 'y2', 'y2', 'y2:y2'),
    ('many', False, 'g', 'g', 'g:g g:nfw g2:g2 g2:nfw nfw:nfw'),
    ('many', False, 'g2', 'g2', 'g2:g2 g2:nfw g:g g:nfw nfw:nfw'),
    ('many', False, 'gc', 'gc', 'gc:gc gc:nfw g:g g:nfw g2:g2 g2:nfw nfw:nfw'),
    ('many', False, 'g', 'g2', ''),
    ('many', False, 'y', 'y2', ''),
    ('many', False, 'g', 'electron', 'g:g g:electron electron:electron electron:g2 electron:gc g2:g2 gc:gc'),
    ('many', False, 'gc', 'y', 'gc:gc gc:y y:y y:g y:g2 g:g g2:g2'),
    ('many', False, 'y2', 'g2', 'y2:y2 y2:g2 y2:g y2:nfw g2:g2 g2:nfw g:g g:nfw nfw:nfw'),
    ('many', False, 'gc', 'g', ''),
    ('both', True, 'electron', 'electron', ''),
    ('both', True, 'g', 'g', 'g:g g:nfw g:y nfw:nfw nfw:y y:y'),
    ('both', True, 'nfw', 'nfw', 'nfw:nfw nfw:g nfw:y g:g g:y y:y'),
    ('both', True, 'electron', 'nfw', ''),
    ('both', True, 'g', 'electron', ''),
    ('both', False, 'electron', 'electron', ''),
    ('both', False, 'g', 'g', 'g:g g:nfw nfw:nfw'),
    ('both', False, 'nfw', 'nfw', 'nfw:nfw nfw:g g:g'),
    ('both', False, 'electron', 'nfw', ''),
    ('both', False, 'g', 'electron', ''),
    ('hand', True, 'nfw', 'nfw', 'nfw:nfw nfw:g nfw:electron nfw:good g:g g:electron g:good electron:electron electron:good good:good'),
    ('hand', True, 'good', 'good', 'good:good good:g good:nfw good:electron g:g g:nfw g:electron nfw:nfw nfw:electron electron:electron'),
    ('hand', True, 'broken', 'broken', ''),
    ('hand', True, 'gb', 'gb', ''),
    ('hand', True, 'g', 'g', 'g:g g:nfw g:electron g:good nfw:nfw nfw:electron nfw:good electron:electron electron:good good:good'),
    ('hand', True, 'nfw', 'broken', ''),
    ('hand', True, 'good', 'g', 'good:good good:g good:nfw good:electron g:g g:nfw g:electron nfw:nfw nfw:electron electron:electron'),
    ('hand', False, 'nfw', 'nfw', 'nfw:nfw nfw:g g:g'),
    ('hand', False, 'good', 'good', 'good:good'),
    ('hand', False, 'broken', 'broken', ''),
    ('hand', False, 'gb', 'gb', ''),
    ('hand', False, 'g', 'g', 'g:g g:nfw nfw:nfw'),
    ('hand', False, 'nfw', 'broken', ''),
    ('hand', False, 'good', 'g', 'good:good good:g good:nfw g:g g:nfw nfw:nfw'),
]
RIDER_IDS = [f"{r[0]}-{'small' if r[1] else 'large'}-{r[2]}-{r[3]}" for r in RIDERS]

# (registry, pairs) -> does power_device_batch take the batched kernel
BATCHABLE = [
    ('readme', [('nfw', 'nfw'), ('g', 'electron'), ('y', 'y')], True),
    ('readme', [('g', 'nfw'), ('nfw', 'g'), ('g', 'g')], True),
    ('many', [('g', 'g2')], False),
    ('many', [('y', 'y2'), ('nfw', 'nfw')], False),
    ('many', [('g', 'y'), ('g2', 'y2')], True),
    ('many', [('g', 'g'), ('g2', 'g2')], True),
    ('many', [('gc', 'electron'), ('gc', 'gc')], True),
    ('many', [('nfw', 'nfw'), ('electron', 'electron'), ('y', 'y'), ('g', 'g')], True),
    ('many', [('nfw', 'nfw'), ('electron', 'electron'), ('y', 'y'), ('g', 'g'), ('gc', 'gc')], False),
    ('both', [('electron', 'electron')], False),
    ('both', [('nfw', 'g')], True),
]

# Whole requests through the facade: (registry, small-grid rule, [(method, arguments ...)], the calls of each step as
# render and run keep them); "requeue" leaves the stages of a pass queued for the request behind it.
SEQUENCES = [
    ('readme', True, [('get_power', 'nfw'), ('get_power_2halo', 'g', 'electron'), ('_bump',), ('get_power_1halo', 'electron', 'g')],
     ['hmg_malloc', 'hmg_malloc', 'hmg_memcpy_h2d', 'hmg_hod', 'hmg_group_rows', 'hmg_profile_support_epoch',
      'hmg_prefix_deferral', 'hmg_group_profile', 'hmg_prefix_deferral', 'hmg_profile_support_epoch',
      'hmg_power_batch_run mhmp 00,01,02,03,11,12,13,22,23,33 prepared', 'hmg_malloc', 'hmg_add', 'hmg_memcpy_d2h'],
     ['hmg_memcpy_d2h'],
     [],
     ['hmg_malloc', 'hmg_power_batch_run mhmp 00,01,02,03,11,12,13,22,23,33', 'hmg_memcpy_d2h'],
     ),
    ('readme', False, [('get_power', 'nfw'), ('get_power', 'y')],
     ['hmg_malloc', 'hmg_malloc', 'hmg_memcpy_h2d', 'hmg_hod', 'hmg_group_rows', 'hmg_profile_support_epoch',
      'hmg_prefix_deferral', 'hmg_group_profile', 'hmg_prefix_deferral', 'hmg_profile_support_epoch',
      'hmg_power_batch_run mh 00,01,11 prepared', 'hmg_malloc', 'hmg_add', 'hmg_memcpy_d2h'],
     ['hmg_malloc', 'hmg_power_batch_run p 00', 'hmg_malloc', 'hmg_add', 'hmg_memcpy_d2h'],
     ),
    ('readme', True, [('requeue',), ('get_power', 'nfw')],
     [],
     ['hmg_malloc', 'hmg_malloc', 'hmg_memcpy_h2d', 'hmg_sigma2_halo_front', 'hmg_profile_support_epoch',
      'hmg_prefix_deferral', 'hmg_group_tensors', 'hmg_prefix_deferral', 'hmg_profile_support_epoch',
      'hmg_power_batch_run mhmp 00,01,02,03,11,12,13,22,23,33 prepared', 'hmg_malloc', 'hmg_add', 'hmg_memcpy_d2h'],
     ),
    ('many', True, [('get_power', 'g', 'g2'), ('get_power_all', [('g', 'nfw'), ('nfw', 'g'), ('g', 'g'), ('g', 'nfw')])],
     ['hmg_malloc', 'hmg_malloc', 'hmg_malloc', 'hmg_memcpy_h2d', 'hmg_hod', 'hmg_power hh 1h+2h', 'hmg_malloc', 'hmg_add',
      'hmg_memcpy_d2h'],
     ['hmg_malloc', 'hmg_malloc', 'hmg_malloc', 'hmg_malloc', 'hmg_malloc', 'hmg_malloc', 'hmg_malloc', 'hmg_malloc',
      'hmg_power_batch_run hm 01,00', 'hmg_memcpy_d2d', 'hmg_memcpy_d2d', 'hmg_memcpy_d2d', 'hmg_memcpy_d2d', 'hmg_malloc',
      'hmg_add', 'hmg_memcpy_d2h', 'hmg_malloc', 'hmg_add', 'hmg_memcpy_d2h', 'hmg_malloc', 'hmg_add', 'hmg_memcpy_d2h',
      'hmg_malloc', 'hmg_add', 'hmg_memcpy_d2h'],
     ),
    ('both', True, [('get_power', 'electron'), ('power_device', 'electron', 'nfw')],
     ['hmg_hod', 'hmg_prefix_fill electron', 'hmg_malloc', 'hmg_malloc', 'hmg_memcpy_h2d', 'hmg_power hh 1h', 'hmg_malloc',
      'hmg_power mm 2h', 'hmg_malloc', 'hmg_add', 'hmg_memcpy_d2h'],
     ['hmg_prefix_fill electron', 'hmg_malloc', 'hmg_power hm 1h', 'hmg_malloc', 'hmg_power mm 2h'],
     ),
    ('hand', True, [('get_power', 'nfw'), ('get_power_1halo', 'good', 'nfw')],
     ['hmg_malloc', 'hmg_malloc', 'hmg_memcpy_h2d', 'hmg_hod', 'hmg_power_batch_run mhmm 00,01,02,03,11,12,13,22,23,33',
      'hmg_malloc', 'hmg_add', 'hmg_memcpy_d2h'],
     ['hmg_memcpy_d2h'],
     ),
    ('numeric', True, [('power_device', 'g', 'nfw'), ('two_halo_terms', 'nfw', 'electron'), ('get_power', 'g', 'electron')],
     ['hmg_hod', 'hmg_group_rows', 'hmg_profile_support_epoch', 'hmg_prefix_deferral', 'hmg_group_profile',
      'hmg_prefix_deferral', 'hmg_profile_support_epoch', 'hmg_prefix_fill nfw', 'hmg_malloc', 'hmg_malloc', 'hmg_malloc',
      'hmg_memcpy_h2d', 'hmg_power hm 1h+2h'],
     ['hmg_prefix_fill nfw', 'hmg_prefix_fill electron', 'hmg_malloc', 'hmg_malloc', 'hmg_malloc',
      'hmg_power_2halo_terms mm', 'hmg_memcpy_d2h', 'hmg_memcpy_d2h', 'hmg_memcpy_d2h'],
     ['hmg_malloc', 'hmg_power_batch_run hmmp 00,01,02,03,11,12,13,22,23,33', 'hmg_malloc', 'hmg_add', 'hmg_memcpy_d2h'],
     ),
]


# ---------------------------------------------------------------------------------------------------- the pure module
def plain(reg):
    """A registry as spectra.py takes it: the HOD mapping, the two key lists, the validity predicate."""
    hods = {n: {"satellite_profile": s, "central_profile": c} for n, (s, c) in reg["hods"].items()}
    return hods, reg["uk"], reg["pk"], lambda tag, name: name not in reg.get("wrong", ())


def resolve_all(reg, names):
    hods, uk, pk, _ = plain(reg)
    return [spectra.resolve(n, hods, uk, pk) for n in names]


def test_resolve():
    hods = {"g": {"satellite_profile": "nfw", "central_profile": None},
            "gc": {"satellite_profile": "nfw", "central_profile": "electron"},
            "electron": {"satellite_profile": "nfw", "central_profile": None}}
    R = spectra.Resolved
    # each dict alone
    assert spectra.resolve("g", hods, [], []) == R("g", "h", "h", (("uk", "nfw"),), (("uk", "nfw"),))
    assert spectra.resolve("nfw", {}, ["nfw"], []) == R("nfw", "m", "m", (("uk", "nfw"),), (("uk", "nfw"),))
    assert spectra.resolve("y", {}, [], ["y"]) == R("y", "p", "p", (("pk", "y"),), (("pk", "y"),))
    # an HOD with a central profile streams two tensors
    assert spectra.resolve("gc", hods, ["nfw", "electron"], ["y"]).tensors1 == (("uk", "nfw"), ("uk", "electron"))
    # a name in two dicts: the 1-halo lookup tries hods, uk, pk, the 2-halo lookup uk, pk, hods
    both = spectra.resolve("electron", hods, ["nfw", "electron"], ["y"])
    assert both == R("electron", "h", "m", (("uk", "nfw"),), (("uk", "electron"),)) and not both.same
    assert both.found(1) == ("h", (("uk", "nfw"),)) and both.found(2) == ("m", (("uk", "electron"),))
    assert spectra.resolve("x", {}, ["x"], ["x"])[1:3] == ("m", "m")
    assert spectra.resolve("x", {"x": hods["g"]}, [], ["x"])[1:3] == ("h", "p")
    assert spectra.resolve("g", hods, [], []).same
    with pytest.raises(ValueError, match="'nope'"):
        spectra.resolve("nope", hods, ["nfw"], ["y"])


@pytest.mark.parametrize("regname,small,a,b,want", RIDERS, ids=RIDER_IDS)
def test_rider_rule(regname, small, a, b, want):
    reg = REGISTRIES[regname]
    hods, uk, pk, valid = plain(reg)
    ra, rb = resolve_all(reg, [a, b])
    got = spectra.with_riders(ra, rb, resolve_all(reg, [*hods, *uk, *pk]), valid, small)
    assert " ".join(f"{x.name}:{y.name}" for x, y in got) == want
    assert all(isinstance(t, spectra.Resolved) for pair in got for t in pair)


def test_rider_rule_reads_the_registered_tracers_only_while_the_batch_has_room():
    reg = REGISTRIES["many"]
    hods, uk, pk, valid = plain(reg)
    seen = []

    def registered():
        for r in resolve_all(reg, [*hods, *uk, *pk]):
            seen.append(r.name)
            yield r
    ra, rb = resolve_all(reg, ["nfw", "electron"])
    got = spectra.with_riders(ra, rb, registered(), valid, True)
    assert seen == ["g", "g2"] and len({t.name for pair in got for t in pair}) == spectra.BATCH_NAMES == 4


@pytest.mark.parametrize("regname,pairs,want", BATCHABLE)
def test_batch_rule(regname, pairs, want):
    names = list(dict.fromkeys(n for pair in pairs for n in pair))
    rec = dict(zip(names, resolve_all(REGISTRIES[regname], names)))
    assert spectra.batchable(list(rec.values()), [(rec[a], rec[b]) for a, b in pairs]) is want


def test_pair_bookkeeping():
    names, unique, alias, first = spectra.pair_plan([("a", "b"), ("b", "a"), ("a", "a"), ("a", "b")])
    assert (names, unique, alias, first) == (["a", "b"], [(0, 1), (0, 0)], [0, 0, 1, 0], [0, 2])
    names, unique, alias, first = spectra.pair_plan([("y", "y"), ("x", "y"), ("z", "x"), ("y", "x")])
    assert (names, unique, alias, first) == (["y", "x", "z"], [(0, 0), (0, 1), (1, 2)], [0, 1, 2, 1], [0, 1, 2])
    assert spectra.pair_plan([]) == ([], [], [], [])


# ---------------------------------------------------------------------------------------------------- the facade on it
@pytest.fixture
def no_switches(monkeypatch):
    for sw in ("HMG_LANES", "HMG_NO_GROUPS", "HMG_NO_PREFIX_DEFERRAL", "HMG_NO_HINTS", "HMG_NO_ROWSC", "HMG_X"):
        monkeypatch.delenv(sw, raising=False)
    return monkeypatch


def model(regname, small, monkeypatch, ctx):
    import hmvec_amd as hm
    monkeypatch.setattr(hm.HaloModel, "_SMALL_GRID_BYTES", (32 << 20) if small else 0)
    return build(REGISTRIES[regname], ctx)


@pytest.mark.parametrize("regname,small,steps,want", [(*s[:3], list(s[3:])) for s in SEQUENCES],
                         ids=[f"{s[0]}-{'small' if s[1] else 'large'}-{s[2][-1][0]}" for s in SEQUENCES])
def test_requests_through_the_facade_make_the_recorded_calls(no_switches, capsys, regname, small, steps, want):
    ctx = rc.recording_context(render)
    h = model(regname, small, no_switches, ctx)
    assert [run(h, step) for step in steps] == want
    ctx.handle = None


@pytest.mark.parametrize("regname,small,a,b,want", RIDERS, ids=RIDER_IDS)
def test_the_cache_holds_both_orders_of_every_pair_of_the_batch(no_switches, regname, small, a, b, want):
    ctx = rc.recording_context()
    h = model(regname, small, no_switches, ctx)
    valid = plain(REGISTRIES[regname])[3]
    if not all(valid(*t) for r in resolve_all(REGISTRIES[regname], [a, b]) for t in r.tensors1 + r.tensors2):
        with pytest.raises(ValueError, match="has shape"):
            h.get_power_1halo(a, b)
        assert h._pcache == {}
    else:
        h.get_power_1halo(a, b)
        pairs = [tuple(p.split(":")) for p in want.split()]          # (none: the one-pair kernel, its own entry only)
        assert set(h._pcache) == ({k for p in pairs for k in (p, p[::-1])} or {(a, b)})
        assert all(e.version == h._version and (e.host is not None) == bool(pairs) for e in h._pcache.values())
        assert all(h._pcache[p] is h._pcache[p[::-1]] for p in pairs)
    ctx.handle = None


class FailingLib(rc.RecordingLib):
    """The recording stand-in with entries that report a native error."""

    def __init__(self):
        rc.RecordingLib.__init__(self)
        self.failing = set()

    def __getattr__(self, name):
        entry = rc.RecordingLib.__getattr__(self, name)
        return (lambda *args: entry(*args) + 1) if name in self.failing else entry


@pytest.mark.parametrize("failing", ["hmg_group_tensors", "hmg_power_batch_run"])
def test_a_native_error_in_a_cached_request_reaches_the_caller_and_nothing_is_cached(no_switches, failing):
    """The pass whose launch fails is gone (the queue is popped before it is issued): a second attempt would integrate
    over tensors, n and b that were never recomputed, and cache the result."""
    class Lib:
        @staticmethod
        def hmg_last_error():
            return b"stand-in failure"
    no_switches.setattr(nat, "load", lambda: Lib)
    ctx = rc.recording_context()
    ctx.lib = FailingLib()
    h = model("readme", True, no_switches, ctx)
    h.get_power("g")
    run(h, ("requeue",))                  # the stages of a new pass are queued: the request issues them with its batch
    before, n = dict(h._pcache), len(ctx.lib.calls)
    assert h._stages and all(ent.version != h._version for ent in before.values())
    ctx.lib.failing.add(failing)
    with pytest.raises(nat.NativeError, match="stand-in failure"):
        h.get_power("nfw")                # (on this small grid electron, y and g ride along)
    assert h._pcache == before
    assert ctx.lib.names(n).count("hmg_power_batch_run") == (failing == "hmg_power_batch_run")
    assert ctx.lib.names(n).count("hmg_group_tensors") == 1 and "hmg_power" not in ctx.lib.names(n)
    ctx.handle = None
