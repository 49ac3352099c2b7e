#!/usr/bin/env python
"""Record the attribute surface of ``HaloModel`` (tests/golden/facade_surface.json; tests/test_facade_cpu.py compares
the class against it).  Needs no device and no built library.

    python tools/make_facade_surface.py            # rewrite the fixture
    python tools/make_facade_surface.py --print    # to stdout

Regenerate only in a change that means to alter the surface (a new public method, a new signature), and say so there:
a refactor of the class must leave the file as it is.
"""
import hashlib
import inspect
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)
FIXTURE = os.path.join(REPO, "tests", "golden", "facade_surface.json")


def _doc(obj):
    return hashlib.sha256((getattr(obj, "__doc__", None) or "").encode()).hexdigest()[:16]


def surface(cls):
    """name -> {kind, signature, doc} for every name in dir(cls).  Signature and docstring hash are taken of what is
    written in Python (functions, static and class methods, properties); everything else - class attributes, the
    slots object provides - is recorded by kind alone, so the record does not depend on the interpreter's version."""
    out = {}
    for name in dir(cls):
        raw = inspect.getattr_static(cls, name)
        if isinstance(raw, staticmethod):
            kind, fn = "staticmethod", raw.__func__
        elif isinstance(raw, classmethod):
            kind, fn = "classmethod", raw.__func__
        elif isinstance(raw, property):
            kind, fn = "property", None
        elif inspect.isfunction(raw):
            kind, fn = "function", raw
        else:
            kind, fn = "other", None
        rec = {"kind": kind}
        if fn is not None:
            rec["signature"] = str(inspect.signature(fn))
            rec["doc"] = _doc(fn)
        elif kind == "property":
            rec["doc"] = _doc(raw)
        out[name] = rec
    return out


def main():
    from hmvec_amd.halomodel import HaloModel
    text = json.dumps(surface(HaloModel), indent=1, sort_keys=True) + "\n"
    if "--print" in sys.argv[1:]:
        sys.stdout.write(text)
    else:
        with open(FIXTURE, "w") as f:
            f.write(text)
        print(f"{FIXTURE}: {len(json.loads(text))} names")


if __name__ == "__main__":
    main()
