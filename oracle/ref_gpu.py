"""The reference's own rasterizer and k-NN kernels, built with hipcc for gfx950 -- TEST INFRASTRUCTURE ONLY.

build() copies the reference's cuda_rasterizer/*.{cu,h} and simple_knn.{cu,h} from a reference checkout into oracle/_ref/src/
(git-ignored, never committed), joins the `<< <` ... `>> >` launch brackets clang wants joined, and compiles them beside
oracle/ref_gpu/ref_driver.cpp (our extern "C" layer) against the redirecting headers in oracle/ref_gpu/shim/ into

    oracle/_ref/libref_gfx950.so       -ffp-contract=off, the setting the CPU oracle and the projection kernel are built with
    oracle/_ref/libref_gfx950_fma.so   the compiler's default contraction, as a CUDA build of the reference contracts too

Where there is no reference checkout (MOM_REFERENCE_DIR, default /root/reference) build() returns and leaves oracle/_ref/ as
it is.  The rest of the module is the ctypes binding: forward() / backward() / mark_visible() / knn_mean_dist2() with
raster_oracle's signatures and state field names, so that a reference state passes through the comparisons a HIP state or an
oracle state passes through (tests/raster_compare.py, tests/test_reference_kernels_gpu.py).
"""
from __future__ import annotations

import ctypes as C
import hashlib
import json
import os
import re
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from .raster_oracle import RasterState, _p, _prep

_HERE = os.path.dirname(os.path.abspath(__file__))
RECIPE = os.path.join(_HERE, "ref_gpu")
OUT = os.path.join(_HERE, "_ref")
SRC = os.path.join(OUT, "src")
VARIANTS = {"off": ("libref_gfx950.so", ["-ffp-contract=off"]), "fma": ("libref_gfx950_fma.so", [])}
ENTRY_POINTS = ("ref_forward", "ref_state_copy", "ref_backward", "ref_free", "ref_mark_visible", "ref_knn")
MAX_JOBS = 16
_RASTER_SUB = os.path.join("submodules", "depth-diff-gaussian-rasterization")
_KNN_SUB = os.path.join("submodules", "simple-knn")
_LIBS = {}


def reference_dir() -> str:
    return os.environ.get("MOM_REFERENCE_DIR", "/root/reference")


def lib_path(variant: str = "off") -> str:
    return os.path.join(OUT, VARIANTS[variant][0])


def available(variant: str = "off") -> bool:
    return os.path.exists(lib_path(variant))


# ---- build ----------------------------------------------------------------------------------------------------------------

def _reference_sources(ref):
    """{name in oracle/_ref/src: path in the checkout}, or None where the checkout (or a part of it) is absent."""
    ras = os.path.join(ref, _RASTER_SUB, "cuda_rasterizer")
    knn = os.path.join(ref, _KNN_SUB)
    if not (os.path.isdir(ras) and os.path.isfile(os.path.join(knn, "simple_knn.cu"))):
        return None
    files = {n: os.path.join(ras, n) for n in sorted(os.listdir(ras)) if n.endswith((".cu", ".h"))}
    files.update({n: os.path.join(knn, n) for n in ("simple_knn.cu", "simple_knn.h")})
    return files


def _join_launch_brackets(text: str) -> str:
    return re.sub(r">>[ \t]+>", ">>>", re.sub(r"<<[ \t]+<", "<<<", text))


def _recipe_files():
    out = [os.path.abspath(__file__)]
    for d, _, names in sorted(os.walk(RECIPE)):
        out += [os.path.join(d, n) for n in sorted(names) if n.endswith((".h", ".cuh", ".cpp"))]
    return out


def _stamp(texts, hipcc):
    h = hashlib.sha256()
    h.update(subprocess.run([hipcc, "--version"], capture_output=True, text=True, check=True).stdout.encode())
    for name in sorted(texts):
        h.update(name.encode() + b"\0" + texts[name].encode() + b"\0")
    for path in _recipe_files():
        with open(path, "rb") as f:
            h.update(os.path.relpath(path, _HERE).encode() + b"\0" + f.read() + b"\0")
    return h.hexdigest()


def build(force: bool = False, verbose: bool = False) -> bool:
    """Compile both libraries from the reference checkout.  Returns True if the libraries are there and current afterwards,
    False -- touching nothing -- where there is no checkout.  Rebuilds only when a source, the recipe or the compiler changed."""
    ref = reference_dir()
    files = _reference_sources(ref)
    if files is None:
        return False
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    texts = {}
    for name, path in files.items():
        with open(path, encoding="utf-8") as f:
            texts[name] = _join_launch_brackets(f.read())
    stamp = _stamp(texts, hipcc)
    stamp_path = os.path.join(OUT, "stamp.json")
    if not force and all(available(v) for v in VARIANTS) and os.path.exists(stamp_path):
        with open(stamp_path) as f:
            if json.load(f).get("stamp") == stamp:
                return True
    os.makedirs(SRC, exist_ok=True)
    if os.path.exists(stamp_path):
        os.remove(stamp_path)
    for name, text in texts.items():
        with open(os.path.join(SRC, name), "w", encoding="utf-8") as f:
            f.write(text)
    common = ["--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-I", os.path.join(RECIPE, "shim"), "-I", SRC,
              "-I", os.path.join(ref, _RASTER_SUB, "third_party", "glm"), "-D__trap=__builtin_trap", "-Wno-unused-result"]
    units = [(os.path.join(SRC, n), ["-x", "hip"] + (["-include", "float.h"] if n == "simple_knn.cu" else []))
             for n in sorted(texts) if n.endswith(".cu")]
    units.append((os.path.join(RECIPE, "ref_driver.cpp"), []))
    jobs = []
    for variant, (_, flags) in VARIANTS.items():
        objdir = os.path.join(OUT, "obj_" + variant)
        os.makedirs(objdir, exist_ok=True)
        for src, extra in units:
            obj = os.path.join(objdir, os.path.splitext(os.path.basename(src))[0] + ".o")
            jobs.append([hipcc] + common + flags + extra + ["-c", src, "-o", obj])

    def run(cmd):
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("reference build failed:\n" + " ".join(cmd) + "\n" + r.stderr[-4000:])
        if verbose and r.stderr:
            print(r.stderr)

    with ThreadPoolExecutor(max_workers=min(MAX_JOBS, len(jobs))) as pool:
        list(pool.map(run, jobs))
    for variant in VARIANTS:
        objdir = os.path.join(OUT, "obj_" + variant)
        objs = [os.path.join(objdir, os.path.splitext(os.path.basename(src))[0] + ".o") for src, _ in units]
        tmp = lib_path(variant) + ".tmp"
        run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", tmp] + objs)
        os.replace(tmp, lib_path(variant))
    with open(stamp_path, "w") as f:
        json.dump({"stamp": stamp, "hipcc": subprocess.run([hipcc, "--version"], capture_output=True, text=True).stdout.splitlines()[:2]}, f)
    return True


def compiler_version() -> str:
    """The compiler the libraries in oracle/_ref/ were built with (recorded at build time)."""
    with open(os.path.join(OUT, "stamp.json")) as f:
        return " / ".join(json.load(f)["hipcc"])


# ---- binding --------------------------------------------------------------------------------------------------------------

class RefError(RuntimeError):
    pass


def _lib(variant: str):
    if variant not in _LIBS:
        if not available(variant):
            raise RefError(f"{lib_path(variant)} is not built (oracle.ref_gpu.build() needs a reference checkout)")
        lib = C.CDLL(lib_path(variant))
        for name in ENTRY_POINTS:
            getattr(lib, name).restype = C.c_int
        _LIBS[variant] = lib
    return _LIBS[variant]


def _check(status: int, what: str) -> None:
    if status != 0:
        raise RefError(f"{what}: " + ("the reference threw" if status < 0 else f"hipError_t {status}"))


class RefState(RasterState):
    """RasterState of a reference forward; owns the device buffers the backward reads until close()."""

    def close(self):
        h = self.pop("_handle", None)
        if h:
            _lib(self["_variant"]).ref_free(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def forward(means3D, opacities, viewmatrix, projmatrix, campos, W, H, tanfovx, tanfovy, bg,
            shs=None, sh_degree=0, colors_precomp=None, scales=None, rotations=None, cov3D_precomp=None,
            scale_modifier=1.0, variant="off") -> RefState:
    """RasterizeGaussiansCUDA (rasterize_points.cu:35-117) around the reference's Rasterizer::forward, on the GPU."""
    f32 = np.float32
    means3D = _prep(means3D, f32, False)
    P = means3D.shape[0]
    opacities = _prep(opacities, f32, False).reshape(-1)
    shs, colors_precomp, scales = _prep(shs, f32), _prep(colors_precomp, f32), _prep(scales, f32)
    rotations, cov3D_precomp = _prep(rotations, f32), _prep(cov3D_precomp, f32)
    viewmatrix, projmatrix = _prep(viewmatrix, f32, False).reshape(-1), _prep(projmatrix, f32, False).reshape(-1)
    campos, bg = _prep(campos, f32, False).reshape(-1), _prep(bg, f32, False).reshape(-1)
    M = 0 if shs is None else shs.shape[1]
    if P != 0 and shs is None and colors_precomp is None:
        raise ValueError("need shs or colors_precomp")
    if P != 0 and cov3D_precomp is None and (scales is None or rotations is None):
        raise ValueError("need scales and rotations, or cov3D_precomp")
    gx, gy = (W + 15) // 16, (H + 15) // 16
    st = RefState()
    st["P"], st["W"], st["H"], st["M"], st["D"], st["grid"], st["_variant"] = P, W, H, M, sh_degree, (gx, gy), variant
    st["radii"] = np.zeros(P, np.int32)
    st["means2D"], st["depths"], st["cov3D"] = np.zeros((P, 2), f32), np.zeros(P, f32), np.zeros((P, 6), f32)
    st["rgb"], st["conic_opacity"] = np.zeros((P, 3), f32), np.zeros((P, 4), f32)
    st["tiles_touched"], st["point_offsets"] = np.zeros(P, np.uint32), np.zeros(P, np.uint32)
    st["clamped"] = np.zeros((P, 3), np.uint8)
    st["out_color"], st["out_depth"] = np.zeros((3, H, W), f32), np.zeros((1, H, W), f32)
    st["ranges"] = np.zeros((gx * gy, 2), np.uint32)
    st["final_T"], st["n_contrib"] = np.zeros(H * W, f32), np.zeros(H * W, np.uint32)
    st["num_rendered"] = 0
    st["point_list"], st["point_list_keys"] = np.zeros(0, np.uint32), np.zeros(0, np.uint64)
    if P == 0:  # rasterize_points.cu:82 short-circuit
        return st
    lib = _lib(variant)
    handle, R = C.c_void_p(0), C.c_int(0)
    _check(lib.ref_forward(C.byref(handle), C.c_int(P), C.c_int(sh_degree), C.c_int(M), _p(bg), C.c_int(W), C.c_int(H),
                           _p(means3D), _p(shs), _p(colors_precomp), _p(opacities), _p(scales), C.c_float(scale_modifier),
                           _p(rotations), _p(cov3D_precomp), _p(viewmatrix), _p(projmatrix), _p(campos),
                           C.c_float(tanfovx), C.c_float(tanfovy), C.byref(R)), "ref_forward")
    st["_handle"] = handle
    st["num_rendered"] = R.value
    st["point_list"], st["point_list_keys"] = np.zeros(R.value, np.uint32), np.zeros(R.value, np.uint64)
    _check(lib.ref_state_copy(handle, _p(st.depths), _p(st.means2D), _p(st.cov3D), _p(st.conic_opacity), _p(st.rgb),
                              _p(st.clamped), _p(st.tiles_touched), _p(st.point_offsets), _p(st.point_list_keys),
                              _p(st.point_list), _p(st.ranges), _p(st.n_contrib), _p(st.final_T), _p(st.radii),
                              _p(st.out_color), _p(st.out_depth)), "ref_state_copy")
    st["_inputs"] = dict(colors_precomp=colors_precomp, cov3D_precomp=cov3D_precomp)
    return st


GRADS = (("dL_dmeans2D", 3), ("dL_dconic", 4), ("dL_dopacity", 1), ("dL_dcolors", 3), ("dL_ddepths", 1), ("dL_dmeans3D", 3),
         ("dL_dcov3D", 6), ("dL_dsh", None), ("dL_dscales", 3), ("dL_drotations", 4))


def backward(st: RefState, dL_dout_color, dL_dout_depth=None) -> dict:
    """RasterizeGaussiansBackwardCUDA (rasterize_points.cu:119-202) around the reference's Rasterizer::backward: all ten tensors."""
    P, W, H, M = st.P, st.W, st.H, st.M
    f32 = np.float32
    g = {n: np.zeros((P, M, 3) if w is None else (P, w), f32) for n, w in GRADS}
    if P == 0:
        return g
    dpix = _prep(dL_dout_color, f32, False)
    ddep = np.zeros((1, H, W), f32) if dL_dout_depth is None else _prep(dL_dout_depth, f32, False)
    assert dpix.shape == (3, H, W) and ddep.size == H * W
    _check(_lib(st["_variant"]).ref_backward(st["_handle"], _p(dpix), _p(ddep), *[_p(g[n]) for n, _ in GRADS]), "ref_backward")
    return g


def mark_visible(means3D, viewmatrix, projmatrix, variant="off"):
    m = _prep(means3D, np.float32, False)
    out = np.zeros(m.shape[0], np.uint8)
    if m.shape[0]:
        _check(_lib(variant).ref_mark_visible(C.c_int(m.shape[0]), _p(m), _p(_prep(viewmatrix, np.float32).reshape(-1)),
                                              _p(_prep(projmatrix, np.float32).reshape(-1)), _p(out)), "ref_mark_visible")
    return out.astype(bool)


def knn_mean_dist2(points, variant="off"):
    """simple_knn._C.distCUDA2 (simple-knn/spatial.cu:15-25) around the reference's SimpleKNN::knn."""
    p = _prep(points, np.float32, False)
    out = np.zeros(p.shape[0], np.float32)
    if p.shape[0]:
        _check(_lib(variant).ref_knn(C.c_int(p.shape[0]), _p(p), _p(out)), "ref_knn")
    return out
