"""ctypes binding of libmom4d.so, derived from the C ABI's own declaration: include/mom4d.h is read when this module is imported
(constants, argument structs) and when the library is loaded (signatures).  A new entry point, struct member or constant is
declared in the header and nowhere else.

The product path FAILS LOUDLY when the HIP library is missing: there is no CPU or
torch fallback behind these calls.
"""
from __future__ import annotations

import ctypes as C
import os
import re
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MOM4D_LIB") or os.path.join(_HERE, "lib", "libmom4d.so")
_lib = None
HEADER_PATH = os.path.normpath(os.path.join(_HERE, "..", "include", "mom4d.h"))   # as csrc/Makefile's ../../include


class MomError(RuntimeError):
    pass


# ---- include/mom4d.h is the one description of the boundary: constants, argument structs and signatures are read from it ----
# (tests/test_abi.py compares everything derived here with clang's own parse of the header)
_SCALARS = {"int": C.c_int, "unsigned": C.c_uint, "uint32_t": C.c_uint, "size_t": C.c_size_t, "float": C.c_float,
            "double": C.c_double, "mom_stream_t": C.c_void_p}
_RETURNS = {"int": C.c_int, "size_t": C.c_size_t, "const char*": C.c_char_p}
_DECLARATOR = re.compile(r"(.*?)(\w+)((?:\s*\[\d+\])*)$", re.S)           # `const float *` `W1` `[3]`
_PROTOTYPE = re.compile(r"^([\w \t\*]+?)[ \t]*\b(mom_\w+)\s*\(([^()]*)\)\s*;", re.M)   # each prototype starts a line of the header


def _strip_comments(text):
    return re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)


def _ctype(ctext, structs, where):
    """A C type as the header writes it -> its ctypes type.  A pointer to one of `structs` stays typed (byref() of the struct
    converts fastest through POINTER(S)), every other pointer is c_void_p; a scalar outside _SCALARS is an error, not a guess."""
    base = " ".join(re.sub(r"\bconst\b|\*", " ", ctext).split())
    if "*" in ctext:
        return C.POINTER(structs[base]) if base in structs and ctext.count("*") == 1 else C.c_void_p
    if base not in _SCALARS:
        raise MomError(f"{where}: no ctypes type for `{' '.join(ctext.split())}` (include/mom4d.h)")
    return _SCALARS[base]


def parse_constants(text):
    """{name: value} of the integer `#define MOM_*` and of every enum constant, in the header's order."""
    text, out = _strip_comments(text), {}
    for name, value in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(MOM_\w+)[ \t]+(.+?)[ \t]*$", text, flags=re.M):
        m = re.fullmatch(r"\(?\s*(-?\d+)[uU]?(?:\s*<<\s*(\d+))?\s*\)?", value)          # 8, (-1), (1u << 20)
        if m:
            out[name] = int(m.group(1)) << int(m.group(2) or 0)
    for body in re.findall(r"\benum\s*\{([^{}]*)\}", text):
        value = 0
        for item in filter(None, (s.strip() for s in body.split(","))):
            name, eq, given = (s.strip() for s in item.partition("="))
            value = int(given, 0) if eq else value
            out[name] = value
            value += 1
    return out


class _SizedStructure(C.Structure):
    """A struct whose first member is struct_size: set at construction, checked by every entry point that takes the struct."""

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self.struct_size = C.sizeof(type(self))


def parse_structs(text):
    """{name: ctypes.Structure} of every `typedef struct [tag] { ... } name;`, members in the header's order: pointers are
    c_void_p, `T a[n][m]` is (T * m) * n, `int W, H;` is two members."""
    out = {}
    for body, name in re.findall(r"\btypedef\s+struct\s*\w*\s*\{([^{}]*)\}\s*(\w+)\s*;", _strip_comments(text)):
        fields = []
        for decl in filter(None, (s.strip() for s in body.split(";"))):
            base = None
            for declarator in decl.split(","):
                head, member, dims = _DECLARATOR.match(declarator.strip()).groups()
                base = head.replace("*", " ") if base is None else base       # `const float *W0, *b0`: the stars are per declarator
                ctype = _ctype(base + "*" * head.count("*"), {}, f"{name}.{member}")
                for n in reversed(re.findall(r"\d+", dims)):
                    ctype = ctype * int(n)
                fields.append((member, ctype))
        sized = bool(fields) and fields[0][0] == "struct_size"
        out[name] = type(name, (_SizedStructure if sized else C.Structure,), {"_fields_": fields})
    return out


def parse_prototypes(text, structs):
    """{name: (restype, argtypes)} of every `mom_*` prototype (each starts a line of the header)."""
    out = {}
    for ret, name, params in _PROTOTYPE.findall(_strip_comments(text)):
        ret = " ".join(ret.split()).replace(" *", "*")
        if ret not in _RETURNS:
            raise MomError(f"{name}: no ctypes type for the return type `{ret}` (include/mom4d.h)")
        params = [] if params.strip() in ("", "void") else [_DECLARATOR.match(p.strip()).groups() for p in params.split(",")]
        out[name] = (_RETURNS[ret], [_ctype(head + "*" * dims.count("["), structs, f"{name}({arg})") for head, arg, dims in params])
    return out


def _read_header():
    try:
        with open(HEADER_PATH) as f:
            return _strip_comments(f.read())
    except OSError as e:
        raise MomError(f"{HEADER_PATH} is missing or unreadable ({e}): the binding is derived from it") from e


_HEADER = _read_header()
_CONSTS = parse_constants(_HEADER)
_STRUCTS = parse_structs(_HEADER)         # MomRasterArgs, MomHexPlane, ...; MomComm stays opaque (it has no body)
# every constant under its header name and without the MOM_ prefix (MOM_OK / MOM_EINVAL, COMM_F32, DENSIFY_XYZ, ABI_VERSION, ...)
globals().update(_CONSTS, **{k[4:]: v for k, v in _CONSTS.items()}, **_STRUCTS)
# every symbol include/mom4d.h declares (the signatures themselves are worked out in lib())
EXPORTS = [name for _, name, _ in _PROTOTYPE.findall(_HEADER)]

_ERR = {MOM_EINVAL: "invalid argument", MOM_ELAUNCH: "HIP launch/runtime failure", MOM_ECAPACITY: "scratch too small",
        MOM_EUNAVAILABLE: "run-time dependency missing (librccl)"}
# MOM_GACC_FLOATS: floats per Gaussian of the backward's accumulator record
GACC_FLOATS = int(os.environ.get("MOM_GACC_FLOATS", GACC_FLOATS))  # (the override: only for A/B builds with -DMOM_GACC_FLOATS=16)
TRI_BOX_GROW = 2.0 ** -20   # MOM_TRI_BOX_GROW (the header names it in a comment only)


def _abi_structs():
    """The MOM_STRUCT_* ids of include/mom4d.h, in order, with the Structure of each (MOM_STRUCT_RASTER_ARGS: MomRasterArgs)."""
    by_name = {n.lower(): cls for n, cls in _STRUCTS.items()}
    return [(k, by_name["mom" + k[len("MOM_STRUCT_"):].replace("_", "").lower()])
            for k in _CONSTS if k.startswith("MOM_STRUCT_") and k != "MOM_STRUCT_COUNT"]


def build(verbose: bool = False) -> str:
    """Compile every HIP source for gfx950 into lib/libmom4d.so (hipcc cross-compiles without a GPU)."""
    cmd = ["make", "-C", os.path.join(_HERE, "csrc"), "-j8"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise MomError("building libmom4d.so failed:\n" + r.stdout[-4000:])
    if verbose:
        print(r.stdout)
    return LIB_PATH


class _Missing:
    """Lax mode's stand-in for a symbol the library lacks: it raises when called."""
    restype = argtypes = None

    def __init__(self, name):
        self.name = name

    def __call__(self, *a):
        raise MomError(f"{self.name} is not in {LIB_PATH}")


class _LaxCDLL(C.CDLL):
    # MOM4D_LIB_LAX=1, A/B tooling only (tools/kbench.py with MOM4D_LIB naming an OLDER build of the library): bind what that build
    # has (a variant built from the CURRENT header -- tools/variants.sh -- or an older build: symbols the older one lacks raise on
    # call, and its ABI check is skipped when it predates mom_abi_version)
    def __getattr__(self, name):
        try:
            return super().__getattr__(name)
        except AttributeError:
            if name.startswith("__"):
                raise
            stub = _Missing(name)
            setattr(self, name, stub)                 # one stub per name: the restype / argtypes lib() assigns stick to later lookups
            return stub


_CTYPE_NAMES = {C.c_int: "C.c_int", C.c_uint: "C.c_uint", C.c_float: "C.c_float", C.c_void_p: "C.c_void_p",
                C.c_size_t: "C.c_size_t"}


def ctypes_mirror_source(cls, width=112):
    """Python source of the ctypes mirror of one ABI struct, generated from its `_fields_` -- the text INTEGRATION.md section 3
    shows a maintainer; tests/test_abi.py regenerates it and compares, so the document cannot drift from the binding."""
    items = [f'("{n}", {_CTYPE_NAMES[t]})' for n, t in cls._fields_]
    lines, cur = [], "    _fields_ = ["
    for i, it in enumerate(items):
        piece = it + ("," if i + 1 < len(items) else "]")
        if len(cur) + len(piece) + 1 > width:
            lines.append(cur.rstrip())
            cur = " " * 16
        cur += piece + " "
    lines.append(cur.rstrip())
    return (f"class {cls.__name__}(C.Structure):           # include/mom4d.h: {cls.__name__}, ABI version {ABI_VERSION}\n"
            + "\n".join(lines) + "\n\n"
            "    def __init__(self, *args, **kw):\n"
            "        super().__init__(*args, **kw)\n"
            "        self.struct_size = C.sizeof(type(self))   # checked by every entry point: a short struct is MOM_EINVAL\n")


def check_abi(lib):
    """Refuse a library whose ABI is not the one this mirror was written against: the version number, and sizeof of every
    argument struct as the library was compiled against the ctypes mirror's (a short struct would be read past its end)."""
    v = lib.mom_abi_version()
    if v != ABI_VERSION:
        raise MomError(f"{LIB_PATH}: ABI version {v}, this binding was written against {ABI_VERSION} (rebuild the library)")
    for which, (name, cls) in enumerate(_abi_structs()):
        n = lib.mom_abi_sizeof(which)
        if n != C.sizeof(cls):
            raise MomError(f"{LIB_PATH}: sizeof({cls.__name__}) is {n} in the library, {C.sizeof(cls)} in the binding ({name})")


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise MomError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(there is no CPU fallback)")
        # torch first: it brings its own copy of the HIP runtime (torch/lib/libamdhip64.so), and libmom4d must bind to THAT copy --
        # loaded before torch, libmom4d pulls in /opt/rocm's runtime, the process then holds two, and every launch on one of
        # torch's streams fails (seen as "HIP launch/runtime failure" in smoke() when build() had loaded the library first)
        import torch  # noqa: F401
        lax = os.environ.get("MOM4D_LIB_LAX") == "1"
        l = (_LaxCDLL if lax else C.CDLL)(LIB_PATH)
        for name, (restype, argtypes) in parse_prototypes(_HEADER, _STRUCTS).items():
            f = getattr(l, name)  # raises AttributeError if the library lacks a declared symbol (lax mode: a stub that raises when called)
            f.restype, f.argtypes = restype, argtypes
        if lax and isinstance(l.mom_abi_version, _Missing):
            import warnings
            warnings.warn(f"{LIB_PATH}: no mom_abi_version (a build older than ABI 4) bound in lax mode; struct layouts are NOT checked")
        else:
            check_abi(l)
        _lib = l
    return _lib


def check(rc: int, what: str) -> None:
    if rc != MOM_OK:
        raise MomError(f"{what} failed: {_ERR.get(rc, rc)}")


def ptr(t):
    """Device pointer of a torch tensor (None / empty tensor -> NULL, like the reference's empty tensors)."""
    if t is None or t.numel() == 0:
        return None
    return t.data_ptr()


def current_stream():
    """The current HIP stream's handle.  (torch.cuda.current_stream() builds a Stream object after four layers of device-index
    resolution: 10 us a call, and a training step asks a dozen times.)"""
    global _TC
    if _TC is None:
        import torch
        _TC = torch._C
    return _TC._cuda_getCurrentRawStream(_TC._cuda_getDevice())


_TC = None
