"""hmvec_amd/_abi.py, the reader that derives the ctypes binding from include/hmgrid.h, and _native.arguments, which
places keyword arguments by the header's parameter names: every rule of the reader once on a synthetic header, its
refusals, the real header against a C compile of it, and the keyword form of the call sites that take the model block
against the positional tuples they passed before they went by name.  No library, no GPU."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import recording_context as rc  # noqa: E402

from hmvec_amd import _abi  # noqa: E402
from hmvec_amd import _native as nat  # noqa: E402
from hmvec_amd import onepoint  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_I, _D, _P, _Z = C.c_int, C.c_double, C.c_void_p, C.c_size_t

SYNTHETIC = """
/* a block comment with a prototype in it: int hmg_not_this(int a); */
#ifndef X_H
#define X_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif
#define HMG_ABI_VERSION 3      /* a trailing comment */
#define HMG_ID_BYTES 16        // another
#define HMG_NOT_A_NUMBER (1 << 4)
typedef struct hmg_ctx hmg_ctx;
typedef struct {
    int    kind;               /* HMG_KIND_* */
    const double *d_a, *d_b /*[n]*/;
    double fit[9], gamma;
    const int*    d_n;   const double* d_c;
} hmg_inner;
typedef struct {
    const hmg_inner* h_in;
    const int *h_pa, *h_pb;
    double* const* h_out;
    long long serial;
} hmg_outer;
int         hmg_version(void);
const char* hmg_last_error(void);
int hmg_create(int device, hmg_ctx** out);
int hmg_malloc(hmg_ctx* ctx, size_t bytes, void** d_out);
int hmg_copy(hmg_ctx* ctx, void* d_dst, const void* h_src, size_t bytes);
int hmg_work(hmg_ctx* ctx, int n, const double* d_x /*[n]*/, const double* h_x /*[n], same C type*/,
             const double h_fit[9], double scale, const hmg_outer* h_desc /* or NULL */,
             const double* const* h_d_in, double* const* h_d_out, const size_t* h_counts, long long epoch);
int hmg_id(char h_id[HMG_ID_BYTES]);
#ifdef __cplusplus
}
#endif
#endif
"""
NAMES = {"hmg_inner": "Inner", "hmg_outer": "Outer"}


def test_synthetic_header_every_rule_once():
    defines, structs, sig, params = _abi.read(SYNTHETIC, NAMES)
    assert defines == {"HMG_ABI_VERSION": 3, "HMG_ID_BYTES": 16}
    inner, outer = structs["hmg_inner"], structs["hmg_outer"]
    assert (inner.__name__, outer.__name__) == ("Inner", "Outer") and issubclass(inner, C.Structure)
    assert inner._fields_ == [("kind", _I), ("d_a", _P), ("d_b", _P), ("fit", _D * 9), ("gamma", _D), ("d_n", _P), ("d_c", _P)]
    assert outer._fields_ == [("h_in", C.POINTER(inner)), ("h_pa", C.POINTER(_I)), ("h_pb", C.POINTER(_I)),
                              ("h_out", C.POINTER(_P)), ("serial", C.c_longlong)]
    assert sig == {
        "hmg_version": [],
        "hmg_create": [_I, C.POINTER(_P)],
        "hmg_malloc": [_P, _Z, C.POINTER(_P)],
        "hmg_copy": [_P, _P, _P, _Z],
        "hmg_work": [_P, _I, _P, C.POINTER(_D), C.POINTER(_D * 9), _D, C.POINTER(outer), C.POINTER(_P), C.POINTER(_P),
                     C.POINTER(_Z), C.c_longlong],
        "hmg_id": [C.c_char * 16],
    }
    assert params["hmg_version"] == () and params["hmg_id"] == ("h_id",)
    assert params["hmg_work"] == ("ctx", "n", "d_x", "h_x", "h_fit", "scale", "h_desc", "h_d_in", "h_d_out", "h_counts", "epoch")
    assert "hmg_last_error" not in sig and "hmg_not_this" not in sig


@pytest.mark.parametrize("header, offenders", [
    ("int hmg_f(hmg_ctx* ctx, int* pending);", ("hmg_f", "pending")),                       # an unprefixed pointer
    ("typedef struct { double* out; } hmg_inner;", ("hmg_inner", "out")),
    ("int hmg_f(hmg_ctx* ctx, float x);", ("hmg_f", "x", "float")),                         # an unknown base type
    ("int hmg_f(hmg_ctx* ctx, const float* d_x);", ("hmg_f", "d_x", "float")),
    ("int hmg_f(hmg_ctx* ctx, const hmg_other* h_x);", ("hmg_f", "h_x", "hmg_other")),
    ("int hmg_f(hmg_ctx* ctx, int n)\nint hmg_g(hmg_ctx* ctx);", ("hmg_f",)),               # a prototype without its ';'
    ("int hmg_g(hmg_ctx* ctx);\nint hmg_f(hmg_ctx* ctx, int n)\n", ("hmg_f",)),
    ("double hmg_f(hmg_ctx* ctx);", ("hmg_f",)),                                            # not this header's style
    ("int hmg_f(hmg_ctx* ctx, int a, b);", ("hmg_f", "b")),
    ("int hmg_f(hmg_ctx* ctx, int (*h_cb)(int));", ("hmg_f",)),
    ("int hmg_f(hmg_ctx* ctx, double h_v[HMG_UNKNOWN]);", ("hmg_f", "h_v", "HMG_UNKNOWN")),
    ("typedef struct { int a; } hmg_unnamed;", ("hmg_unnamed",)),
])
def test_refusals_name_the_offender(header, offenders):
    with pytest.raises(_abi.HeaderError) as e:
        _abi.read(header, NAMES if "hmg_inner" in header else {})
    assert all(o in str(e.value) for o in offenders), str(e.value)


def test_struct_missing_from_header_is_refused():
    with pytest.raises(_abi.HeaderError, match="hmg_outer"):
        _abi.read("typedef struct { int a; } hmg_inner;", NAMES)


def test_header_error_is_an_import_error():
    assert issubclass(_abi.HeaderError, ImportError)        # what a failing `import hmvec_amd` raises


# ---------------------------------------------------------------- the real header
def _header():
    with open(os.path.join(REPO, "include", "hmgrid.h")) as f:
        return f.read()


def test_real_header_every_prototype_is_bound():
    declared = set(re.findall(r"^int\s+(hmg_\w+)\s*\(", _header(), re.M))
    assert declared == set(nat.SIGNATURES) == set(nat.PARAMS) and len(declared) > 90
    for name in declared:
        assert len(nat.PARAMS[name]) == len(nat.SIGNATURES[name]), name
        assert all(isinstance(p, str) and p.isidentifier() for p in nat.PARAMS[name]), name
    assert nat.HEADER_PATH == os.path.join(REPO, "include", "hmgrid.h")
    assert nat.ABI_VERSION == nat.DEFINES["HMG_ABI_VERSION"] and nat.COMM_ID_BYTES == nat.DEFINES["HMG_COMM_ID_BYTES"]
    for cname, pyname in nat._STRUCTS.items():
        cls = getattr(nat, pyname)
        assert issubclass(cls, C.Structure) and cls.__name__ == pyname and cname in cls.__doc__


def test_real_header_struct_layout_agrees_with_the_compiler(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no host C compiler")
    lines, expected = [], []
    for cname, pyname in nat._STRUCTS.items():
        cls = getattr(nat, pyname)
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        expected.append(f"{cname} {C.sizeof(cls)}")
        for field, _ in cls._fields_:
            lines.append(f'printf("{cname}.{field} %zu\\n", offsetof({cname}, {field}));')
            expected.append(f"{cname}.{field} {getattr(cls, field).offset}")
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hmgrid.h"\nint main(void) {\n'
                   + "\n".join(lines) + "\nreturn 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.run([cc, "-I", os.path.join(REPO, "include"), str(src), "-o", exe], check=True)
    got = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split("\n")
    assert got[:-1] == expected


def test_missing_header_is_an_import_error_naming_the_path(tmp_path):
    """_native's own code run as if the package lay somewhere without include/hmgrid.h beside it."""
    with open(nat.__file__) as f:
        code = compile(f.read(), nat.__file__, "exec")
    where = {"__name__": "hmvec_amd._native_elsewhere", "__package__": "hmvec_amd",
             "__file__": str(tmp_path / "hmvec_amd" / "_native.py")}
    with pytest.raises(ImportError, match=re.escape(str(tmp_path / "include" / "hmgrid.h"))):
        exec(code, where)


# ---------------------------------------------------------------- keyword calls
def test_arguments_response_and_trispectrum_as_their_positional_call_sites():
    v = {n: object() for n in set(nat.PARAMS["hmg_response"]) | set(nat.PARAMS["hmg_trispectrum_1h"])}
    grid = (v["d_nzm"], v["d_bh"], v["d_ms"], v["d_wm"], v["d_ks"], v["d_Pzk"], v["rho_m0"])     # the block, with the bias
    block = {n: v[n] for n in ("d_nzm", "d_bh", "d_ms", "d_wm", "d_ks", "d_Pzk", "rho_m0")}
    # hmg_response: "nz, nm, nk, n, npairs, tr, *grid[:6], d_dlnP.ptr, grid[6], kstar, d_idx.ptr, ..., R.ptr, ptr(P)"
    was = (v["nz"], v["nm"], v["nk"], v["n"], v["np"], v["h_pairs"], *grid[:6], v["d_dlnP"], grid[6], v["kstar"],
           v["d_idx"], v["d_frac"], v["d_scale"], v["d_R"], v["d_parts"])
    kw = dict(d_parts=v["d_parts"], d_R=v["d_R"], kstar=v["kstar"], d_dlnP=v["d_dlnP"], **block, h_pairs=v["h_pairs"],
              np=v["np"], n=v["n"], d_idx=v["d_idx"], d_frac=v["d_frac"], d_scale=v["d_scale"])
    assert nat.arguments("hmg_response", (v["nz"], v["nm"], v["nk"]), kw) == was
    assert nat.arguments("hmg_response", was, {}) == was
    # hmg_trispectrum_1h: "nz, nm, nk, n, *byref(tracers), nzm, ms, wm, rho_m0, d_idx.ptr, ..., ptr(T), ptr(Tz)"
    was = (v["nz"], v["nm"], v["nk"], v["n"], v["h_a"], v["h_b"], v["h_c"], v["h_d"], v["d_nzm"], v["d_ms"], v["d_wm"],
           v["rho_m0"], v["d_idx"], v["d_frac"], v["d_scale"], v["d_zweights"], v["d_T"], v["d_Tz"])
    names = nat.PARAMS["hmg_trispectrum_1h"][1:]
    assert nat.arguments("hmg_trispectrum_1h", (), {n: v[n] for n in reversed(names)}) == was
    assert [n for n in names if n in block] == ["d_nzm", "d_ms", "d_wm", "rho_m0"]      # what HaloModel._model_block keeps


def test_arguments_refusals():
    names = nat.PARAMS["hmg_ssc"][1:]
    kw = dict.fromkeys(names, 0)
    assert nat.arguments("hmg_ssc", (), kw) == (0,) * len(names)
    with pytest.raises(nat.NativeError, match="unknown d_nope"):
        nat.arguments("hmg_ssc", (), dict(kw, d_nope=0))
    with pytest.raises(nat.NativeError, match="duplicate nz"):
        nat.arguments("hmg_ssc", (3,), kw)
    with pytest.raises(nat.NativeError, match="missing d_cov"):
        nat.arguments("hmg_ssc", (), {n: 0 for n in names if n != "d_cov"})
    with pytest.raises(nat.NativeError, match="hmg_ssc"):
        nat.arguments("hmg_ssc", (0,) * (len(names) + 1), {})
    with pytest.raises(nat.NativeError, match="hmg_nope"):
        nat.arguments("hmg_nope", (), {})
    with pytest.raises(nat.NativeError, match="hmg_gnfw_quad_table"):        # no context: not a Context.call
        nat.arguments("hmg_gnfw_quad_table", (), {"h_table": 0})


def test_context_call_places_keywords_before_the_library_and_traces_positionally():
    ctx = rc.recording_context()
    with pytest.raises(nat.NativeError, match="missing d_cov"):
        ctx.call("hmg_ssc", 1, 2, 3, d_R=4, d_zscale=5, d_g=6)
    assert ctx.lib.calls == []                                   # refused before anything reached the library
    calls = ctx.trace(lambda: ctx.call("hmg_ssc", 1, 2, np=3, d_cov=7, d_g=6, d_zscale=5, d_R=4))
    assert calls == [("hmg_ssc", (1, 2, 3, 4, 5, 6, 7))]
    assert ctx.lib.calls == [("hmg_ssc", (ctx.handle, 1, 2, 3, 4, 5, 6, 7))]


def test_the_call_sites_by_name_pass_what_the_positional_ones_did():
    """The nine entry points that take the model block, issued by the facade against the recording stand-in: every call
    is complete, each member of the block sits at the position the header gives its name, and hmg_response and
    hmg_trispectrum_1h carry the block where their positional call sites spliced it."""
    ctx = rc.recording_context()
    h = rc.build_model(ctx)
    sets = np.array([[0.2, 1.0, 10.0, 0.8, 1.5, -0.1]])
    h.trispectrum_device("nfw", "g", kindex=[1, 5])
    h.bispectrum_device("nfw", "nfw", "g", kindex=[1, 5, 9])
    h.response_device([("g", "nfw")], kindex=[1, 5])
    h.rsd_device("g", "nfw", kindex=[1, 5])
    h.multipoles_device("g", "nfw", kindex=[1, 5])
    h.hod_ensemble_device(sets, mthresh=np.full(rc.ZS.size, 10 ** 10.5))
    block = dict(d_nzm=h._d_nzm.ptr, d_bh=h._d_bh.ptr, d_ms=h._d_ms().ptr, d_wm=h._d_wm().ptr, d_ks=h._d_ks().ptr,
                 d_Pzk=h._d_Pzk().ptr, rho_m0=h._rho_m0())
    assert len(set(block.values())) == 7
    last = {name: args for name, args in ctx.lib.calls}
    for entry in ("hmg_trispectrum_1h", "hmg_bispectrum", "hmg_response", "hmg_rsd_wedges", "hmg_rsd_multipoles",
                  "hmg_hod_ensemble", "hmg_hod_ensemble_power"):
        args, names = last[entry], nat.PARAMS[entry]
        assert len(args) == len(names) and args[0] == ctx.handle, entry
        assert {n: a for n, a in zip(names, args) if n in block} == {n: block[n] for n in names if n in block}, entry
    assert last["hmg_response"][7:13] == tuple(block.values())[:6] and last["hmg_response"][14] == block["rho_m0"]
    assert last["hmg_trispectrum_1h"][9:13] == (block["d_nzm"], block["d_ms"], block["d_wm"], block["rho_m0"])
    assert last["hmg_hod_ensemble"][8:12] == (block["d_ms"], block["d_nzm"], block["d_bh"], block["d_wm"])

    nz, nm, nt = 2, 3, 4
    arrays = np.ones((nz, nm, nt)), np.ones((nz, nm, nt)), np.ones((nz, nm)), np.ones(nm), np.ones(nz)
    onepoint.char_exponent(*arrays, 5, 0.25, mwindow=(1, 3), ctx=ctx)
    onepoint.cumulants(*arrays, mwindow=(1, 3), ctx=ctx)
    last = {name: args for name, args in ctx.lib.calls}
    e, m = last["hmg_onepoint_exponent"], last["hmg_onepoint_moments"]
    assert len(e) == len(nat.PARAMS["hmg_onepoint_exponent"]) and len(m) == len(nat.PARAMS["hmg_onepoint_moments"])
    assert e[1:4] == m[1:4] == (nz, nm, nt) and e[6] is None and e[10:14] == (1, 3, 5, 0.25) and m[10:12] == (1, 3)
