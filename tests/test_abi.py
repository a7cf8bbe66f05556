"""The C ABI library loads on a GPU-less machine and exports every symbol include/mom4d.h declares; the binding _native.py derives
from that header -- signatures, argument structs, constants -- is what clang reads in it."""
import ctypes as C
import functools
import importlib
import json
import os
import re
import subprocess

import pytest

N = importlib.import_module("iclr2025_3d-mom_amd._native")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mom4d.h")

# the C types of the header's vocabulary, as clang spells them once typedefs are resolved (size_t: unsigned long, uint32_t:
# unsigned int, mom_stream_t: void *), and the ctypes type the binding must give each
_SCALARS = {"int": C.c_int, "unsigned int": C.c_uint, "unsigned long": C.c_size_t, "float": C.c_float, "double": C.c_double}
_RETURNS = {"int": C.c_int, "size_t": C.c_size_t, "const char *": C.c_char_p}


def _run_clang(args, source=None):
    clang = os.path.join(os.environ.get("ROCM_PATH") or "/opt/rocm", "llvm", "bin", "clang")
    assert os.path.exists(clang), f"{clang} is missing: the library cannot be built without that tree either"
    r = subprocess.run([clang, "-x", "c", "-I", os.path.dirname(HEADER)] + args, input=source, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout


@functools.lru_cache(maxsize=None)
def _clang():
    """clang's reading of include/mom4d.h (none of _native's parser is used): functions {name: (return type, [parameter types])},
    structs {typedef name: [(member, type)]} and constants {name: value} -- every MOM_* macro, evaluated by clang as the value of an
    enum constant of a translation unit made for that, and every enum constant of the header."""
    macros = re.findall(r"^#define (MOM_\w+) \S", _run_clang(["-dM", "-E", HEADER]), flags=re.M)
    unit = '#include "mom4d.h"\nenum {\n' + "".join(f"  value_of_{m} = ({m}),\n" for m in macros) + "};\n"
    top = json.loads(_run_clang(["-fsyntax-only", "-Xclang", "-ast-dump=json", "-"], unit))["inner"]

    def kids(node, kind):
        return [c for c in node.get("inner", []) if c["kind"] == kind]

    def spelled(node):
        return node["type"].get("desugaredQualType", node["type"]["qualType"])

    functions = {n["name"]: (n["type"]["qualType"].split("(")[0].strip(), [spelled(p) for p in kids(n, "ParmVarDecl")])
                 for n in top if n["kind"] == "FunctionDecl" and n["name"].startswith("mom_")}
    records = {n["id"]: [(f["name"], spelled(f)) for f in kids(n, "FieldDecl")]
               for n in top if n["kind"] == "RecordDecl" and n.get("completeDefinition")}

    def record_of(node):                                               # the RecordDecl a typedef's type names, however it is wrapped
        if "decl" in node:
            return node["decl"]["id"]
        return next(filter(None, map(record_of, node.get("inner", []))), None)

    structs = {n["name"]: records[record_of(n)] for n in top if n["kind"] == "TypedefDecl" and n["name"].startswith("Mom")
               and record_of(n) in records}                            # MomComm is declared, never defined: it stays opaque

    def evaluated(node):                                               # the value clang gives an enum constant's initialiser (it may sit under a cast)
        if node["kind"] == "ConstantExpr":
            return node["value"]
        return next((v for v in map(evaluated, node.get("inner", [])) if v is not None), None)

    constants = {}
    for enum in (n for n in top if n["kind"] == "EnumDecl"):
        value = -1
        for c in kids(enum, "EnumConstantDecl"):
            given = evaluated(c)                                       # none: one more than the constant before it
            value = int(given) if given is not None else value + 1
            constants[c["name"].replace("value_of_", "")] = value
    return functions, structs, constants


def _ctype(spelling, typed_struct_pointers):
    """The ctypes type for a C type as clang spells it: the table of the binding, written out again."""
    base, dims = re.fullmatch(r"(.*?)((?:\[\d+\])*)", spelling).groups()
    base = re.sub(r"\b(const|struct)\b", "", base).strip()
    if base.endswith("*"):
        pointee = getattr(N, base[:-1].strip(), None)                 # "MomComm *" (of MomComm **) and MomComm itself: no such Structure
        typed = typed_struct_pointers and isinstance(pointee, type) and issubclass(pointee, C.Structure)
        ctype = C.POINTER(pointee) if typed else C.c_void_p
    else:
        ctype = _SCALARS[base]
    for n in reversed(re.findall(r"\d+", dims)):                     # T a[n][m] is (T * m) * n
        ctype = ctype * int(n)
    return ctype


def test_every_declared_symbol_is_exported_and_bound():
    """restype and argtypes of every entry point are what clang's prototype says: an entry too few in a list of 21 pointers, or a
    *_bytes function left at the default int return, is undefined behaviour no other test would see."""
    lib = N.lib()
    functions = _clang()[0]
    assert len(functions) >= 100
    assert sorted(N.EXPORTS) == sorted(functions) and len(N.EXPORTS) == len(functions), "the ctypes binding and the header disagree"
    for name, (ret, params) in functions.items():
        assert hasattr(lib, name), f"{name} declared in include/mom4d.h but not exported by libmom4d.so"
        f = getattr(lib, name)
        assert f.restype is _RETURNS[ret], (name, ret, f.restype)
        assert list(f.argtypes) == [_ctype(p, True) for p in params], (name, params, f.argtypes)
    assert b"gfx950" in lib.mom_version()


def test_struct_members_are_the_headers():
    """Every argument struct: member names in order, element type and array extents.  (A reordered member of MomHexPlane,
    MomDeformMLP, MomRegPlane or MomDensifyTensor keeps sizeof and would pass the size check at load.)"""
    structs = _clang()[1]
    assert len(structs) >= 10 and "MomRowSelect" in structs and "MomComm" not in structs
    for name, members in structs.items():
        cls = getattr(N, name)
        assert issubclass(cls, C.Structure)
        assert [(n, t) for n, t in cls._fields_] == [(n, _ctype(t, False)) for n, t in members], name
    assert sorted(structs) == sorted(n for n, v in vars(N).items()
                                     if isinstance(v, type) and issubclass(v, C.Structure) and n.startswith("Mom"))
    assert set(cls.__name__ for _, cls in N._abi_structs()) <= set(structs)


def test_constants_are_the_headers():
    constants = _clang()[2]
    for name in ("MOM_OK", "MOM_EINVAL", "MOM_ELAUNCH", "MOM_ECAPACITY", "MOM_EUNAVAILABLE"):
        assert getattr(N, name) == constants[name], name
    for name in ("ABI_VERSION", "COMM_F32", "COMM_I32", "COMM_SUM", "COMM_MAX", "SSIM_SUM_SLOTS", "SELECT_MAX_TENSORS",
                 "DENSIFY_MAX_TENSORS", "DENSIFY_MAX_ROW_BYTES", "TRI_LANE_BOX", "DENSIFY_COPY", "DENSIFY_MOMENT", "DENSIFY_XYZ",
                 "DENSIFY_SCALING", "DENSIFY_ROTATION", "DENSIFY_ZERO"):
        assert getattr(N, name) == constants["MOM_" + name], name
    assert N.MOM_EINVAL == -1 and N.DENSIFY_MAX_ROW_BYTES == 1 << 20 and N.DENSIFY_ZERO == 5
    for name, value in constants.items():                              # and every other MOM_* macro or enum constant there is
        assert getattr(N, name) == value, name
    ids = [n for n in constants if n.startswith("MOM_STRUCT_")]
    assert ids == [n for n, _ in N._abi_structs()] + ["MOM_STRUCT_COUNT"] and [constants[n] for n in ids] == list(range(len(ids)))


def test_a_prototype_with_an_unknown_type_is_refused():
    """With the next two: the smallest inputs at which _native's reading of the header can go wrong -- one prototype, one struct."""
    assert N.parse_prototypes("int mom_f(const float* x, size_t n);", {}) == {"mom_f": (C.c_int, [C.c_void_p, C.c_size_t])}
    with pytest.raises(N.MomError, match="long double"):
        N.parse_prototypes("int mom_f(long double x);", {})
    with pytest.raises(N.MomError, match="mom_f"):
        N.parse_prototypes("long double mom_f(int x);", {})


def test_a_struct_member_of_an_unknown_type_is_refused():
    with pytest.raises(N.MomError, match="MomS.x"):
        N.parse_structs("typedef struct MomS { int n; long double x; } MomS;")


def test_a_struct_that_starts_with_struct_size_gets_it_set():
    sized = N.parse_structs("typedef struct MomS { uint32_t struct_size; /* first */ float* p; int a[2][3], b; } MomS;")["MomS"]
    assert [(n, t) for n, t in sized._fields_] == [("struct_size", C.c_uint), ("p", C.c_void_p), ("a", (C.c_int * 3) * 2), ("b", C.c_int)]
    assert sized().struct_size == C.sizeof(sized) == 48
    plain = N.parse_structs("typedef struct { int n; uint32_t struct_size; } MomT;")["MomT"]
    assert plain().struct_size == 0                                    # only a struct that STARTS with struct_size is sized


def test_a_missing_header_is_named(monkeypatch):
    monkeypatch.setattr(N, "HEADER_PATH", os.path.join(ROOT, "include", "no_such_header.h"))
    with pytest.raises(N.MomError, match="no_such_header.h"):
        N._read_header()


def test_sizing_functions_need_no_gpu():
    lib = N.lib()
    assert lib.mom_raster_geom_bytes(1000) >= 1000 * (48 + 24 + 4 + 48)
    assert lib.mom_raster_image_bytes(960, 540) >= 960 * 540 * 8
    assert lib.mom_raster_binning_bytes(1000, 960, 540, 5000) >= 5000 * 12
    assert lib.mom_knn_scratch_bytes(1000) > 0
    lay = N.MomRasterLayout()
    import ctypes as C
    assert lib.mom_raster_layout(1000, 64, 64, 5000, C.byref(lay)) == 0
    assert lay.geom_cov3D >= 1000 * 48 and lay.bin_point_list == 0 and lay.bin_keys >= 5000 * 4      # point_list first: see mom4d.h


def test_invalid_arguments_are_rejected_without_a_gpu():
    import ctypes as C
    lib = N.lib()
    a = N.MomRasterArgs()
    a.P, a.W, a.H = 10, 0, 16          # zero width
    assert lib.mom_raster_forward_geometry(C.byref(a), None, None, None, None, None, None) == N.MOM_EINVAL
    assert lib.mom_mark_visible(-1, None, None, None, None, None) == N.MOM_EINVAL
    assert lib.mom_profile_enable(99, 1) == N.MOM_EINVAL


def test_an_unknown_mlp_backward_form_is_refused(monkeypatch):
    """MOM_MLP_BWD selects the MLP backward's form per call (unset / "b3" / "split", csrc/deform_mlp.hip); any other value --
    "fused" named a form that no longer exists -- is MOM_EINVAL before anything is launched, not a silent choice.  Every pointer
    of the call and of the descriptor is non-null, so the environment value is the only thing there is to refuse (a value that
    selected a form would get as far as the launch and fail there: MOM_ELAUNCH on a machine without a GPU)."""
    import ctypes as C
    lib, fake = N.lib(), 1 << 20          # a non-null pointer value; the calls are refused before it could be followed
    w = N.MomDeformMLP()
    for name, ctype in N.MomDeformMLP._fields_:
        setattr(w, name, fake if ctype is C.c_void_p else ctype(fake, fake, fake))
    for bad in ("fused", "f32", "Split", "b", "split "):
        monkeypatch.setenv("MOM_MLP_BWD", bad)
        assert lib.mom_deform_backward_split(C.byref(w), 32, fake, fake, fake, fake, fake, fake, fake, None, None) == N.MOM_EINVAL, bad
        assert lib.mom_deform_backward(C.byref(w), 32, fake, fake, fake, fake, fake, fake, fake, None) == N.MOM_EINVAL, bad


def test_abi_version_and_struct_sizes_are_checked_at_load():
    """mom_abi_version / mom_abi_sizeof (include/mom4d.h, "ABI versioning"): the binding refuses a library of another ABI."""
    import ctypes as C
    lib = N.lib()
    header = open(os.path.join(ROOT, "include", "mom4d.h")).read()
    assert int(re.search(r"#define MOM_ABI_VERSION (\d+)", header).group(1)) == N.ABI_VERSION == lib.mom_abi_version()
    ids = re.search(r"enum \{(.*?)\};", header, flags=re.S).group(1)
    ids = [t.strip().split("=")[0].strip() for t in ids.replace("\n", " ").split(",") if t.strip()]
    assert ids == [n for n, _ in N._abi_structs()] + ["MOM_STRUCT_COUNT"]
    for which, (_, cls) in enumerate(N._abi_structs()):
        assert lib.mom_abi_sizeof(which) == C.sizeof(cls)
    assert lib.mom_abi_sizeof(len(ids) - 1) == 0

    class Fake:                                   # a library of another ABI version
        def mom_abi_version(self):
            return N.ABI_VERSION - 1
    import pytest
    with pytest.raises(N.MomError, match="ABI version"):
        N.check_abi(Fake())


def test_a_short_or_unsized_raster_args_struct_is_refused():
    """a binder written against an older header passed a struct without the newest field.  struct_size is the
    first field now and every entry point that takes MomRasterArgs compares it with its own sizeof."""
    import ctypes as C
    lib = N.lib()
    a = N.MomRasterArgs()
    assert a.struct_size == C.sizeof(N.MomRasterArgs)
    a.P, a.W, a.H = 0, 16, 16                      # P == 0 is otherwise valid and needs no GPU
    nr = (C.c_uint * 2)()
    for size in (0, C.sizeof(N.MomRasterArgs) - 4, C.sizeof(N.MomRasterArgs) + 8):
        a.struct_size = size
        assert lib.mom_raster_forward_geometry(C.byref(a), None, None, None, nr, None, None) == N.MOM_EINVAL
        assert lib.mom_raster_backward_render(C.byref(a), None, None, 0, None, None, None, None) == N.MOM_EINVAL
        assert lib.mom_raster_backward_geometry(C.byref(a), None, None, None, None) == N.MOM_EINVAL
        assert lib.mom_raster_backward(C.byref(a), None, None, None, 0, None, None, None, None, None) == N.MOM_EINVAL


def test_integration_md_shows_the_binding_as_it_is():
    """INTEGRATION.md section 3's ctypes mirror is generated from _native.py (tools/gen_integration_stub.py); the document's
    copy must be that text, and executing it must give the binding's layout."""
    import ctypes as C
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    begin = "# --- generated from iclr2025_3d-mom_amd/_native.py"
    i = text.index("\n", text.index(begin)) + 1
    j = text.index("# --- end generated ---", i)
    assert text[i:j] == N.ctypes_mirror_source(N.MomRasterArgs), "run tools/gen_integration_stub.py"
    ns = {"C": C}
    exec(text[i:j], ns)
    doc = ns["MomRasterArgs"]
    assert [(n, t) for n, t in doc._fields_] == [(n, t) for n, t in N.MomRasterArgs._fields_]
    assert C.sizeof(doc) == C.sizeof(N.MomRasterArgs) and doc().struct_size == C.sizeof(doc)
    assert f"lib.mom_abi_version() == {N.ABI_VERSION}" in text
    # and the header's struct has the same member names in the same order
    header = open(os.path.join(ROOT, "include", "mom4d.h")).read()
    body = header[header.index("typedef struct MomRasterArgs {"):header.index("} MomRasterArgs;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    members = []
    for decl in body.split("{", 1)[1].split(";"):
        decl = decl.strip()
        if decl:
            head, *rest = decl.split(",")
            members += [re.findall(r"[A-Za-z_0-9]+", head)[-1]] + [re.findall(r"[A-Za-z_0-9]+", r)[-1] for r in rest]
    assert members == [n for n, _ in N.MomRasterArgs._fields_]
