"""Writes tests/golden/g20_eulerian_warp.npz: the warp of the REFERENCE's own video generator on the inputs of
tests/eulerian_warp_cases.py -- euler_integration, blend_feature, feature_inpaint_conv and warp_one_level of
thirdparty/StyleCineGAN/utils/cinemagraph_utils.py.

Run by hand on a machine that has a checkout of the reference; the tests read only the file it writes.

    python tools/gen_eulerian_warp_golden.py --reference /path/to/ICLR2025_3D-MOM [--out tests/golden/g20_eulerian_warp.npz]

The reference's warp needs CUDA twice over, and the recipe removes exactly that:
  * softmax_splatting.py imports cupy at module level: an empty stand-in is served for it (nothing of it is called);
  * cinemagraph_utils.py writes device='cuda' and .cuda(): torch.linspace / zeros / ones drop the `device` argument and
    Tensor.cuda returns the tensor, while the reference's functions run;
  * _FunctionSoftsplat.apply, whose forward launches the CUDA string, is replaced by eulerian_warp_cases.splat_for_reference: the
    same four weights and products in fp32, accumulated in float64.  That one function is the part no one can run without CUDA, so
    parity on IT is pinned by the restatement and not by the reference; everything around it -- the Euler chains, the cut, the
    padding, Z, the double canvas, the normalisation, the blank mask from a second blend of ones, the box filter, the crop -- is
    the reference's own code.

The fixture holds outputs only (the inputs are closed forms of eulerian_warp_cases).  Per family S of eulerian_warp_cases.GOLDEN and
per frame idx: the two integrated displacement maps, the blended padded map, its blank mask (from the reference's blend of ones),
warp_one_level's result and the shapes.  The S = 256 maps are too large for a committed file: of the float maps every
STRIDE[256] = 8th row and column is kept, the blank masks are kept whole as packed bits.  One all-frames euler_integration of a
non-square 24 x 40 field is kept whole."""
import argparse
import importlib
import importlib.abc
import importlib.machinery
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import eulerian_warp_cases as ec  # noqa: E402


class _Stub(types.ModuleType):
    __path__ = []

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        child = _Stub(self.__name__ + "." + name)
        setattr(self, name, child)
        return child

    def __call__(self, *a, **k):
        return self


class _StubFinder(importlib.abc.MetaPathFinder, importlib.abc.Loader):
    def __init__(self, names):
        self.names = set(names)

    def find_spec(self, fullname, path=None, target=None):
        if fullname.split(".")[0] in self.names:
            return importlib.machinery.ModuleSpec(fullname, self, is_package=True)
        return None

    def create_module(self, spec):
        return _Stub(spec.name)

    def exec_module(self, module):
        pass


class on_the_cpu:
    """While active: device='cuda' is dropped from the three factory calls the reference makes, and .cuda() is the identity."""
    def __enter__(self):
        self.saved = {n: getattr(torch, n) for n in ("linspace", "zeros", "ones")}
        self.cuda = torch.Tensor.cuda
        for n, fn in self.saved.items():
            setattr(torch, n, (lambda fn: lambda *a, **k: fn(*a, **{x: y for x, y in k.items() if x != "device"}))(fn))
        torch.Tensor.cuda = lambda self, *a, **k: self
        return self

    def __exit__(self, *exc):
        for n, fn in self.saved.items():
            setattr(torch, n, fn)
        torch.Tensor.cuda = self.cuda


def import_reference(ref_dir):
    sys.meta_path.append(_StubFinder(("cupy",)))
    sys.path.insert(0, ref_dir)
    cu = importlib.import_module("thirdparty.StyleCineGAN.utils.cinemagraph_utils")
    ss = importlib.import_module("thirdparty.StyleCineGAN.utils.softmax_splatting")
    ss._FunctionSoftsplat.apply = staticmethod(
        lambda inp, flw: torch.from_numpy(ec.splat_for_reference(inp.numpy(), flw.numpy())))
    return cu


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="a checkout of cvsp-lab/ICLR2025_3D-MOM")
    ap.add_argument("--out", default=ec.G20)
    a = ap.parse_args()
    cu = import_reference(os.path.abspath(a.reference))
    torch.set_num_threads(1)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x))
    out = {}
    with on_the_cpu(), torch.no_grad():
        m = ec.flow(24, 40)
        disp, _ = cu.euler_integration(t(m)[None], 5, return_all_frames=True)
        out["euler_24x40_all"] = disp.numpy()
        disp, _ = cu.euler_integration(t(m)[None], 5)
        out["euler_24x40_last"] = disp.numpy()[0]
        for S, (_, C, n_frames, idxs) in ec.GOLDEN.items():
            r = ec.STRIDE[S]
            feature, flow = t(ec.features(C, S))[None], t(ec.flow(S))[None]
            cut, pad, P, crop0 = ec.geometry(S)
            inner = flow[:, :, cut:-cut, cut:-cut] if cut else flow
            for idx in idxs:
                key = f"s{S}_i{idx}_"
                fut, _ = cu.euler_integration(cu.pad_tensor(inner, mode="reflect").float(), idx)
                past, _ = cu.euler_integration(cu.pad_tensor(-inner, mode="reflect").float(), n_frames - idx - 1)
                blended = cu.blend_feature(feature, flow.clone(), idx, n_frames)
                ones = cu.blend_feature(torch.ones(1, 1, S, S), flow.clone(), idx, n_frames)
                final = cu.warp_one_level(feature, flow.clone(), idx, n_frames)
                assert blended.shape == (1, C, P, P) and final.shape == (1, C, S, S) and fut.shape == (1, 2, P, P)
                assert torch.isfinite(blended).all() and torch.isfinite(final).all()
                blank = (ones[0, 0] == 0).numpy()
                out[key + "future"] = fut.numpy()[0][:, ::r, ::r]
                out[key + "past"] = past.numpy()[0][:, ::r, ::r]
                out[key + "blended"] = blended.numpy()[0][:, ::r, ::r]
                out[key + "final"] = final.numpy()[0][:, ::r, ::r]
                out[key + "blank_bits"] = np.packbits(blank)
                out[key + "shapes"] = np.array([C, S, cut, pad, P, crop0, n_frames, idx], np.int64)
                inside = blank[crop0:crop0 + S, crop0:crop0 + S]
                print(f"S {S} idx {idx}: blank {blank.mean() * 100:.3f} % of the padded map, {int(inside.sum())} inside the crop; "
                      f"reset displacement {float((fut[0].abs().sum(0) == 0).float().mean()) * 100:.0f} % / "
                      f"{float((past[0].abs().sum(0) == 0).float().mean()) * 100:.0f} %")
            assert any(np.unpackbits(out[f"s{S}_i{i}_blank_bits"])[:P * P].reshape(P, P)[crop0:crop0 + S, crop0:crop0 + S].any()
                       for i in idxs), f"S = {S}: no frame has a blank pixel inside the crop; make eulerian_warp_cases.flow more divergent"
    np.savez_compressed(a.out, **out)
    print(a.out, os.path.getsize(a.out), "bytes")
    assert os.path.getsize(a.out) < (1 << 20)


if __name__ == "__main__":
    main()
