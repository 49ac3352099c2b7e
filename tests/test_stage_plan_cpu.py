"""hmvec_amd/stages.py and the facade's use of it, without a GPU: the stand-alone form of every part, the plan a queue
becomes, the flush-before-queue rule, and the native call sequence of a whole pass against a recording stand-in for
the library (tests/helpers/recording_context.py).  The literal sequences were recorded with the same helper on the
facade as it was before the grouping decision moved into stages.py."""
import ctypes as C
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import recording_context as rc  # noqa: E402

from hmvec_amd import _native as nat  # noqa: E402
from hmvec_amd import stages  # noqa: E402

SWITCHES = ("HMG_LANES", "HMG_NO_GROUPS", "HMG_NO_PREFIX_DEFERRAL", "HMG_NO_HINTS", "HMG_NO_ROWSC", "HMG_X")
DIMS = (3, 48, 96, 77)


@pytest.fixture
def no_switches(monkeypatch):
    for sw in SWITCHES:
        monkeypatch.delenv(sw, raising=False)
    return monkeypatch


def sentinel_part(cls):
    """An instance whose every field holds a value of its own, and those values in field order."""
    vals = []
    for i, (_, typ) in enumerate(cls._fields_):
        if typ is C.c_int:
            vals.append(100 + i)
        elif typ is C.c_double:
            vals.append(0.5 + i)
        elif typ is C.c_void_p:
            vals.append(0x1000 * (i + 1))
        elif issubclass(typ, C.Array):
            vals.append(typ(*[i + j / 16 for j in range(typ._length_)]))
        else:
            vals.append(C.pointer(typ._type_()))
    return cls(*vals), vals


def same(arg, val):
    if isinstance(val, C.Array):           # an embedded array travels by reference
        return list(arg._obj) == list(val)
    if isinstance(val, C._Pointer):        # a pointer as it is
        return C.addressof(arg.contents) == C.addressof(val.contents)
    return type(arg) is type(val) and arg == val


# kind -> (entry, part, fields of the part in front of the grid sizes, grid sizes the entry takes, fields it does not take)
ALONE = {
    "nfw": ("hmg_nfw_analytic", nat.NfwPart, 0, 3, []),
    "hod": ("hmg_hod", nat.HodPart, 0, 2, ["stage"]),
    "rows": ("hmg_profile_rowparams", nat.RowsPart, 1, 2, ["d_ks", "d_kts", "nk", "fft_m", "d_rowsc"]),
    "fft": ("hmg_profile_fft", nat.ProfileFftPart, 0, 3, ["d_rowsc"]),
}


@pytest.mark.parametrize("kind", list(ALONE))
def test_a_part_alone_is_its_fields_in_order_behind_the_grid_sizes(kind):
    entry, cls, lead, ndims, excluded = ALONE[kind]
    part, vals = sentinel_part(cls)
    got_entry, args, tagged = stages.alone(kind, part, DIMS)
    assert got_entry == entry and tagged == (kind == "fft")
    assert len(args) == len(nat.SIGNATURES[entry]) - 1
    taken = [v for (name, _), v in zip(cls._fields_, vals) if name not in excluded]
    assert len(taken) == len(cls._fields_) - len(excluded)
    want = taken[:lead] + list(DIMS[:ndims]) + taken[lead:]
    assert len(want) == len(args) and all(same(a, w) for a, w in zip(args, want)), (args, want)
    for a, t in zip(args, nat.SIGNATURES[entry][1:]):      # ... each in a form the binding's argument type takes
        t.from_param(a)


def parts():
    st = {k: sentinel_part(cls)[0] for k, cls in (("massfn", nat.MassFnPart), ("nfw", nat.NfwPart), ("hod", nat.HodPart),
                                                  ("rows", nat.RowsPart), ("fft", nat.ProfileFftPart))}
    st["hod"].stage = nat.HOD_ALL
    halo = sentinel_part(nat.HaloStageArgs)[0]
    st["front"] = stages.FrontArgs((3, 48, 77, 0x10, 0x20, 0x30, 0x40, 0.01), 0x50, halo)
    return st


ROLE = {nat.HaloStageArgs: "halo", nat.MassFnPart: "massfn", nat.NfwPart: "nfw", nat.RowsPart: "rows",
        nat.ProfileFftPart: "fft", nat.PowerBatchDesc: "prep"}
HOD_STAGE = {nat.HOD_ALL: "hod:all", nat.HOD_OCCUPATIONS: "hod:occupations", nat.HOD_SUMS: "hod:sums"}


def describe(launches):
    """[(entry, the structures its non-NULL pointer arguments point at, tagged)]; every pointer sits where the entry's
    signature has a pointer to that structure."""
    out = []
    for entry, args, tagged in launches:
        sig = nat.SIGNATURES[entry][1:]
        assert len(args) == len(sig), entry
        roles = []
        for a, t in zip(args, sig):
            t.from_param(a)                    # (raises if the binding's argument type would refuse it)
            if type(a).__name__ == "CArgObject":
                assert t._type_ is type(a._obj), (entry, t, a._obj)
                roles.append(HOD_STAGE[a._obj.stage] if isinstance(a._obj, nat.HodPart) else ROLE[type(a._obj)])
        out.append((entry, " ".join(roles), tagged))
    return out


def run_plan(kinds, prep=False, x=""):
    st = parts()
    desc = nat.PowerBatchDesc() if prep else None
    launches, prepared = stages.plan([(k, st[k], ()) for k in kinds], DIMS, desc, x)
    return describe(launches), prepared


FRONT, ROWS, TENSORS, PROFILE = "hmg_sigma2_halo_front", "hmg_group_rows", "hmg_group_tensors", "hmg_group_profile"
PASS = ["front", "massfn", "nfw", "rows", "fft"]
PLANS = [
    # (queued kinds, prep, HMG_X) -> (launches, prepared)
    ((["front", "massfn", "nfw"], False, ""), ([(FRONT, "halo", False), (ROWS, "massfn nfw", False)], False)),
    ((["front", "massfn", "nfw"], True, ""), ([(FRONT, "halo", False), (ROWS, "massfn nfw", False)], False)),
    ((["front", "massfn", "nfw", "hod"], False, ""),
     ([(FRONT, "halo hod:occupations", False), (ROWS, "massfn nfw", False), (PROFILE, "hod:sums", True)], False)),
    ((["front", "massfn", "nfw", "hod"], True, ""),
     ([(FRONT, "halo hod:occupations", False), (ROWS, "massfn nfw", False), (PROFILE, "hod:sums prep", True)], True)),
    ((PASS, False, ""), ([(FRONT, "halo rows", False), (TENSORS, "massfn nfw fft", True)], False)),
    ((PASS, True, ""), ([(FRONT, "halo rows", False), (TENSORS, "massfn prep nfw fft", True)], True)),
    ((PASS + ["hod"], True, ""),
     ([(FRONT, "halo hod:occupations rows", False), (TENSORS, "massfn hod:sums prep nfw fft", True)], True)),
    ((["massfn", "nfw", "fft"], False, ""), ([(TENSORS, "massfn nfw fft", True)], False)),
    ((["massfn", "nfw", "fft"], True, ""), ([(TENSORS, "massfn prep nfw fft", True)], True)),
    # any HMG_X disables the tensor group
    ((["massfn", "nfw", "fft"], False, "prep_alone"), ([(ROWS, "massfn nfw", False), (PROFILE, "fft", True)], False)),
    ((["massfn", "nfw", "fft"], True, "prep_alone"), ([(ROWS, "massfn nfw", False), (PROFILE, "fft", True)], False)),
    ((["massfn", "nfw", "fft"], False, "rows_alone"), ([(ROWS, "massfn nfw", False), (PROFILE, "fft", True)], False)),
    ((["massfn", "nfw", "fft"], True, "rows_alone"), ([(ROWS, "massfn nfw", False), (PROFILE, "fft prep", True)], True)),
    ((PASS, True, "rows_alone"),
     ([(FRONT, "halo", False), (ROWS, "massfn rows nfw", False), (PROFILE, "fft prep", True)], True)),
    ((["massfn", "nfw", "fft"], False, "nfw_alone"),
     ([(ROWS, "massfn", False), ("hmg_nfw_analytic", "", False), (PROFILE, "fft", True)], False)),
    ((["massfn", "nfw", "fft"], True, "nfw_alone"),
     ([(ROWS, "massfn", False), ("hmg_nfw_analytic", "", False), (PROFILE, "fft prep", True)], True)),
    ((["massfn", "nfw", "fft"], False, "chain_alone"), ([(ROWS, "massfn nfw", False), (PROFILE, "fft", True)], False)),
    ((["massfn", "nfw", "fft"], True, "chain_alone"),
     ([(ROWS, "massfn nfw", False), (PROFILE, "prep", False), (PROFILE, "fft", False)], True)),
    ((["hod"], False, ""), ([("hmg_hod", "", False)], False)),
    ((["hod"], True, ""), ([("hmg_hod", "", False)], False)),
    ((["fft"], False, ""), ([(PROFILE, "fft", True)], False)),
    ((["fft"], True, ""), ([(PROFILE, "fft prep", True)], True)),
    (([], False, ""), ([], False)),
    (([], True, ""), ([], False)),
]


@pytest.mark.parametrize("case,want", PLANS, ids=[f"{'+'.join(c[0]) or 'empty'}{'+prep' if c[1] else ''}{'/' + c[2] if c[2] else ''}"
                                                  for c, _ in PLANS])
def test_plan(case, want):
    assert run_plan(*case) == want


def test_plan_of_an_empty_queue_needs_no_grid_sizes():
    assert stages.plan([], None, None, "") == ([], False)


def test_plan_hands_the_grid_sizes_and_the_front_arguments_through():
    st = parts()
    launches, _ = stages.plan([(k, st[k], ()) for k in PASS], DIMS, None, "")
    (front, fargs, _), (tensors, targs, _) = launches
    assert fargs[:9] == (*st["front"].sigma2, st["front"].d_ms) and fargs[9]._obj is st["front"].halo
    assert targs[:4] == DIMS and targs[4]._obj is st["massfn"] and targs[8]._obj is st["fft"]
    launches, _ = stages.plan([(k, st[k], ()) for k in ("hod", "fft")], DIMS, None, "")
    assert launches[0][1][:2] == DIMS[:2] and launches[1][1][:3] == DIMS[:3]
    # the HOD riding with a front is split: a copy computes the occupations, the queued part itself the sums
    launches, _ = stages.plan([(k, st[k], ()) for k in ("front", "hod")], DIMS, None, "")
    occ, sums = launches[0][1][10]._obj, launches[1][1][4]._obj
    assert occ is not st["hod"] and sums is st["hod"] and (occ.stage, sums.stage) == (nat.HOD_OCCUPATIONS, nat.HOD_SUMS)
    assert occ.d_Nc == sums.d_Nc and occ.d_bg == sums.d_bg


D1, D2 = (3, 48, 96, 77), (3, 64, 96, 77)


@pytest.mark.parametrize("pending,pending_dims,kind,dims,want", [
    (["front", "massfn", "nfw"], D1, "nfw", D1, True),            # the same kind twice
    (["hod"], D1, "hod", D1, True),
    (["nfw", "hod"], D1, "massfn", D1, True),                     # a producer behind its consumer
    (["nfw", "fft"], D1, "rows", D1, True),
    (["massfn", "nfw", "rows", "fft", "hod"], D1, "front", D1, True),     # a new front
    (["nfw"], D1, "front", D1, True),
    (["front", "massfn"], D1, "nfw", D2, True),                   # changed grid sizes
    (["front", "massfn", "nfw"], D1, "hod", (3, 48, 96, 78), True),
    ([], None, "front", D1, False),                               # nothing queued: nothing to issue
    ([], D1, "nfw", D2, False),
    (["front"], D1, "massfn", D1, False),                         # the order of a pass
    (["front", "massfn"], D1, "nfw", D1, False),
    (["front", "massfn", "nfw"], D1, "rows", D1, False),
    (["front", "massfn", "nfw", "rows"], D1, "fft", D1, False),
    (["front", "massfn", "nfw", "rows", "fft"], D1, "hod", D1, False),
    (["massfn"], D1, "hod", D1, False),                           # a consumer behind its producer
    (["rows"], D1, "fft", D1, False),
    (["hod"], D1, "nfw", D1, False),
    (["fft"], D1, "massfn", D1, False),                           # (the transform does not read n, b)
])
def test_must_issue_first(pending, pending_dims, kind, dims, want):
    assert stages.must_issue_first(pending, pending_dims, kind, dims) is want


TAG, DEFER = "hmg_profile_support_epoch", "hmg_prefix_deferral"
SECOND_PASS = {
    "default": [
        "hmg_sigma2_halo_front", TAG, DEFER, "hmg_group_tensors", DEFER, TAG, "hmg_hod", "hmg_group_rows",
        TAG, DEFER, "hmg_group_profile", DEFER, TAG, "hmg_power_batch_run"],
    "HMG_NO_GROUPS": [
        "hmg_sigma2_massfn_halo", "hmg_nfw_analytic", "hmg_profile_rowparams", TAG, DEFER, "hmg_profile_fft", DEFER, TAG,
        "hmg_profile_rowparams", TAG, DEFER, "hmg_profile_fft", DEFER, TAG, "hmg_hod", "hmg_power_batch_run"],
    "HMG_LANES": [
        "hmg_lane_set", "hmg_event_record", "hmg_lane_set", "hmg_event_wait", "hmg_sigma2_massfn", "hmg_event_record",
        "hmg_lane_set", "hmg_lane_set", "hmg_halo_stage", "hmg_lane_set", "hmg_nfw_analytic", "hmg_lane_set",
        "hmg_profile_rowparams", TAG, DEFER, "hmg_profile_fft", DEFER, TAG, "hmg_lane_set", "hmg_profile_rowparams",
        TAG, DEFER, "hmg_profile_fft", DEFER, TAG, "hmg_lane_set", "hmg_event_wait", "hmg_hod", "hmg_event_record",
        "hmg_lane_set", "hmg_lane_set", "hmg_event_wait", "hmg_power_batch_run", "hmg_lane_set", "hmg_event_record"],
}
BRACKETED = {"default": ["hmg_group_tensors", "hmg_group_profile"], "HMG_NO_GROUPS": ["hmg_profile_fft"] * 2,
             "HMG_LANES": ["hmg_profile_fft"] * 2}


@pytest.mark.parametrize("mode", list(SECOND_PASS))
def test_second_pass_of_the_facade_makes_the_recorded_calls(no_switches, mode):
    if mode != "default":
        no_switches.setenv(mode, "1")
    ctx = rc.recording_context()
    h = rc.build_model(ctx)                       # (nz, nm, nk) = (3, 48, 96)
    assert (h._groups, h._use_lanes) == (mode == "default", mode == "HMG_LANES")
    calls = ctx.trace(lambda: rc.second_pass(h))
    names = [name for name, _ in calls]
    assert names == SECOND_PASS[mode]
    assert h._stages == [] and ctx._deferred == []
    # the tag and the deferral flag go up right in front of one launch and come down right behind it
    bracketed, i = [], 0
    while i < len(calls):
        if names[i] in (TAG, DEFER):
            assert names[i:i + 2] == [TAG, DEFER] and names[i + 3:i + 5] == [DEFER, TAG], names[i:i + 5]
            assert [calls[j][1] for j in (i, i + 1, i + 3, i + 4)] == [(h._epoch,), (1,), (0,), (0,)] and h._epoch > 0
            bracketed.append(names[i + 2])
            i += 5
        else:
            i += 1
    assert bracketed == BRACKETED[mode]
    ctx.handle = None


def test_a_failed_capture_drops_the_queue(no_switches):
    ctx = rc.recording_context()
    h = rc.build_model(ctx)
    rc.second_pass(h)
    n = len(ctx.lib.calls)

    def fails():
        h.init_mass_function(rc.MS)
        h.add_nfw_profile("nfw", ignore_existing=True)
        raise KeyError("inside the capture")
    with pytest.raises(KeyError):
        ctx.capture(fails)
    assert h._stages == [] and ctx._deferred == []
    assert [x for x in ctx.lib.names(n) if x.startswith("hmg_graph")] == ["hmg_graph_begin", "hmg_graph_abort"]
    assert not any(x.startswith(("hmg_group", "hmg_sigma2")) for x in ctx.lib.names(n))
    ctx.handle = None


def test_a_tagged_launch_that_fails_inside_a_capture_leaves_no_tag_behind(no_switches):
    fail = []

    def render(name, args):
        if name in fail:
            raise KeyError(name)
        return args
    ctx = rc.recording_context(render)
    h = rc.build_model(ctx)
    rc.second_pass(h)
    n = len(ctx.lib.calls)
    fail.append("hmg_group_tensors")
    with pytest.raises(KeyError):
        ctx.capture(lambda: rc.second_pass(h))
    calls = [(name, args[1:]) for name, args in ctx.lib.calls[n:] if name not in ("hmg_malloc", "hmg_free")]
    assert [name for name, _ in calls] == ["hmg_graph_begin", "hmg_sigma2_halo_front", TAG, DEFER, DEFER, TAG, "hmg_graph_abort"]
    assert [args for _, args in calls[2:6]] == [(h._epoch,), (1,), (0,), (0,)]
    assert h._stages == [] and ctx._deferred == []
    ctx.handle = None
