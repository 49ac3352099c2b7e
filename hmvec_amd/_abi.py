"""Reader of include/hmgrid.h: the ctypes binding of the C ABI, derived from its one declaration.

Not a C parser.  It reads the style that header is written in - ``#define HMG_<NAME> <integer>``,
``typedef struct { ... } hmg_<x>;`` and ``int hmg_<name>(...);`` - and raises HeaderError on anything else: a
binding that guesses is worse than none.  The type rule, for parameters and struct fields alike:

  int, double, size_t, long long          the ctypes scalar
  hmg_ctx*, void*  /  hmg_ctx**, void**   c_void_p  /  POINTER(c_void_p)
  hmg_<struct>*                           POINTER(that Structure)
  double x[N]  /  char x[N]               POINTER(c_double * N) (a field: c_double * N)  /  c_char * N; N may be a #define
  T* d_<name>                             c_void_p: a device address
  T* h_<name>  /  T** or T* const* h_<name>    POINTER(T)  /  POINTER(c_void_p): host memory
  any other pointer                       an error: the prefix is what tells host memory from device memory
"""
import ctypes as C
import re

_SCALARS = {"int": C.c_int, "double": C.c_double, "size_t": C.c_size_t, "long long": C.c_longlong}


class HeaderError(ImportError):
    pass


def _declarators(decl, where):
    """'const double *d_a, *d_b' or 'double fit[9], gamma' -> [(base type, stars, name, array length or None), ...]"""
    out, base = [], None
    for part in decl.split(","):
        tok = re.findall(r"\w+|[*\[\]]", part)
        dim = None
        if tok[-1:] == ["]"] and tok[-3:-2] == ["["]:
            dim = tok[-2]
            del tok[-3:]
        words = [t for t in tok if t not in ("*", "const")]
        if not re.fullmatch(r"[\w\s*\[\]]+", part) or not words or "[" in words or "]" in words:
            raise HeaderError(f"{where}: cannot read the declaration {part.strip()!r}")
        base = " ".join(words[:-1]) or base
        if base is None:
            raise HeaderError(f"{where}: {words[-1]!r} has no type")
        out.append((base, tok.count("*"), words[-1], dim))
    return out


def _ctype(base, stars, name, dim, structs, defines, where, field=False):
    where = f"{where}: {name}"
    if dim is not None:
        n = int(dim) if dim.isdigit() else defines.get(dim)
        if n is None or stars or base not in ("double", "char") or (field and base == "char"):
            raise HeaderError(f"{where}: cannot bind the array {base} [{dim}]")
        if base == "char":
            return C.c_char * n
        return C.c_double * n if field else C.POINTER(C.c_double * n)
    if base in ("hmg_ctx", "void") and stars in (1, 2):
        return C.c_void_p if stars == 1 else C.POINTER(C.c_void_p)
    if base in structs and stars == 1:
        return C.POINTER(structs[base])
    if base not in _SCALARS or stars > 2:
        raise HeaderError(f"{where}: unknown base type {base + '*' * stars!r}")
    if not stars:
        return _SCALARS[base]
    if name.startswith("d_") and stars == 1:
        return C.c_void_p
    if name.startswith("h_"):
        return C.POINTER(_SCALARS[base]) if stars == 1 else C.POINTER(C.c_void_p)
    raise HeaderError(f"{where}: a pointer must be named d_* (device) or h_* (host)")


def read(text, struct_names):
    """(defines, structs, signatures, params) of a header given as text.  struct_names maps the C name of every struct
    to the name of its Structure class; structs is keyed by the C name; signatures and params hold every function
    that returns int (``const char* hmg_last_error(void)`` is read and left out)."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    defines = {m[1]: int(m[2]) for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+(HMG_\w+)[ \t]+(-?\d+)[ \t]*$", text, re.M)}
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    text = re.sub(r'extern\s+"C"\s*\{', "", text, count=1)

    structs = {}

    def struct(m):
        body, cname = m[1], m[2]
        if cname not in struct_names:
            raise HeaderError(f"struct {cname}: no class name is given for it")
        fields = [(name, _ctype(base, stars, name, dim, structs, defines, f"struct {cname}", field=True))
                  for decl in body.split(";") if decl.strip()
                  for base, stars, name, dim in _declarators(decl, f"struct {cname}")]
        structs[cname] = type(struct_names[cname], (C.Structure,),
                              {"_fields_": fields, "__doc__": f"{cname} (include/hmgrid.h)"})
        return ""

    text = re.sub(r"typedef\s+struct\s*\{([^{}]*)\}\s*(\w+)\s*;", struct, text)
    missing = sorted(set(struct_names) - set(structs))
    if missing:
        raise HeaderError(f"struct {', '.join(missing)}: not declared in the header")

    signatures, params = {}, {}
    *statements, tail = text.split(";")
    if tail.strip() not in ("", "}"):
        raise HeaderError(f"no ';' after {' '.join(tail.split())[:80]!r}")
    for s in statements:
        s = " ".join(s.split())
        if s in ("", "typedef struct hmg_ctx hmg_ctx", "const char* hmg_last_error(void)"):
            continue
        m = re.fullmatch(r"int (hmg_\w+) ?\(([^()]*)\)", s)
        if not m:
            raise HeaderError(f"cannot read {s[:80]!r}")
        name, args = m[1], m[2].strip()
        decls = [] if args == "void" else [d for a in args.split(",") for d in _declarators(a, name)]
        params[name] = tuple(d[2] for d in decls)
        signatures[name] = [_ctype(*d, structs, defines, name) for d in decls]
    return defines, structs, signatures, params
