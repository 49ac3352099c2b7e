"""The shape of the facade, without a GPU: HaloModel is a core (hmvec_amd/halomodel.py) plus one mixin per section of
derived statistics, each in that section's module ("The facade's sections").

The attribute surface of the class - every name of dir(HaloModel), its kind, its signature and a hash of its docstring -
is pinned by tests/golden/facade_surface.json, which tools/make_facade_surface.py writes (the file was recorded from the
class as it was in one file, before the sections moved).  Regenerate it only in a change that means to alter the surface."""
import importlib.util
import inspect
import json
import os
import re
import sys

import pytest

from hmvec_amd.cosmology import Cosmology
from hmvec_amd.halomodel import HaloModel

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIXINS = [c for c in HaloModel.__mro__ if c not in (HaloModel, object) and not issubclass(Cosmology, c)]


def _generator():
    spec = importlib.util.spec_from_file_location("make_facade_surface", os.path.join(REPO, "tools", "make_facade_surface.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_class_is_the_core_and_eight_mixins():
    assert [c.__name__ for c in MIXINS] == ["RealspaceMixin", "AngularMixin", "SampledMixin", "RsdMixin",
                                            "ClusterLensingMixin", "GasProjectionMixin", "OnePointMixin",
                                            "HodEnsembleMixin"]
    assert [c.__module__ for c in MIXINS] == ["hmvec_amd." + m for m in (
        "realspace", "angular", "sampled", "rsd", "lensing", "gasprofiles", "onepoint", "hod_ensemble")]
    assert issubclass(HaloModel, Cosmology) and HaloModel.__init__.__qualname__ == "HaloModel.__init__"
    for c in MIXINS:
        assert c.__bases__ == (object,) and not c.__name__.startswith("_")


def test_the_surface_of_the_class_is_the_recorded_one():
    gen = _generator()
    with open(gen.FIXTURE) as f:
        want = json.load(f)
    got = gen.surface(HaloModel)
    assert sorted(got) == sorted(want), (sorted(set(want) - set(got)), sorted(set(got) - set(want)))
    wrong = {n: (want[n], got[n]) for n in want if want[n] != got[n]}
    assert not wrong, wrong
    # (what the tests, the benchmark and the tools reach for by name)
    for name in ("_tracer", "_bispectrum", "_y_request", "_SMALL_GRID_BYTES", "_HOD_PARAMS", "_model_block", "_XI_TERMS",
                 "TRISPECTRUM_MAX_SAMPLES", "RESPONSE_MAX_PAIRS"):
        assert name in want and hasattr(HaloModel, name)


def test_no_name_is_defined_twice():
    owners = {}
    for c in [HaloModel] + MIXINS:
        for name in vars(c):
            if name not in ("__module__", "__doc__", "__dict__", "__weakref__", "__qualname__", "__firstlineno__",
                            "__static_attributes__"):
                owners.setdefault(name, []).append(c.__name__)
    twice = {n: o for n, o in owners.items() if len(o) > 1}
    assert not twice, twice
    inherited = set(dir(Cosmology)) - set(dir(object))
    for c in MIXINS:
        clash = sorted(n for n in vars(c) if n in inherited and n not in ("__module__", "__doc__", "__dict__", "__weakref__"))
        assert not clash, (c.__name__, clash)


@pytest.mark.parametrize("mixin", MIXINS, ids=lambda c: c.__name__)
def test_a_mixin_holds_no_state_and_does_not_import_the_core(mixin):
    for name in ("__init__", "__new__", "__slots__"):
        assert name not in vars(mixin), f"{mixin.__name__} defines {name}"
    mod = sys.modules[mixin.__module__]
    core = sys.modules["hmvec_amd.halomodel"]
    held = [n for n, v in vars(mod).items() if v is core or v is HaloModel]
    assert not held, f"{mod.__name__} holds the core as {held}"
    src = inspect.getsource(mod)
    assert not re.search(r"^\s*(from\s+(\.|hmvec_amd)\s+import\s+[^\n]*\bhalomodel\b|from\s+(\.|hmvec_amd\.)halomodel\b"
                         r"|import\s+hmvec_amd\.halomodel\b)", src, re.M), f"{mod.__name__} imports halomodel"
