"""MI355X-native hot path of the 4D Gaussian Splatting train/render loop of cvsp-lab/ICLR2025_3D-MOM.

The directory name is not a Python identifier; load it with
    importlib.import_module("iclr2025_3d-mom_amd")
or call `install_dropin()` (below) and import the reference's own module names
(`diff_gaussian_rasterization`, `simple_knn`, `gaussian_renderer`, `scene.gaussian_model`, ...).
"""
import importlib
import sys

from . import _native
from ._native import build, lib, MomError  # noqa: F401

# reference module name -> module of this package.  Everything the reference's train_4DGS.py / render_4DGS.py import from
# the repository itself (third-party packages such as imageio / mmcv / torchvision are the caller's business).
_DROPIN = {
    "diff_gaussian_rasterization": ".diff_gaussian_rasterization",
    "diff_gaussian_rasterization._C": ".diff_gaussian_rasterization._C",
    "simple_knn": ".simple_knn",
    "simple_knn._C": ".simple_knn._C",
    "gaussian_renderer": ".gaussian_renderer",
    "gaussian_renderer.network_gui": ".gaussian_renderer.network_gui",
    "scene": ".scene",
    "scene.gaussian_model": ".scene.gaussian_model",
    "scene.deformation": ".scene.deformation",
    "scene.hexplane": ".scene.hexplane",
    "scene.regulation": ".scene.regulation",
    "scene.cameras": ".scene.cameras",
    "scene.dataset": ".scene.dataset",
    "scene.dataset_readers": ".scene.dataset_readers",
    "arguments": ".arguments",
    "utils": ".utils",
    "utils.loss_utils": ".utils.loss_utils",
    "utils.image_utils": ".utils.image_utils",
    "utils.general_utils": ".utils.general_utils",
    "utils.graphics_utils": ".utils.graphics_utils",
    "utils.sh_utils": ".utils.sh_utils",
    "utils.system_utils": ".utils.system_utils",
    "utils.camera_utils": ".utils.camera_utils",
    "utils.params_utils": ".utils.params_utils",
    "utils.timer": ".utils.timer",
    "utils.loader_utils": ".utils.loader_utils",
    "utils.scene_utils": ".utils.scene_utils",
}


def install_dropin(only=None) -> None:
    """Register this package's modules under the names the reference scripts import (`from scene import Scene, GaussianModel`,
    `from gaussian_renderer import render, network_gui`, `from utils.loss_utils import l1_loss, ssim`, ...), so that the
    reference's own train_4DGS.py / render_4DGS.py run against libmom4d unchanged.  `only`: an iterable of public names to
    register instead of all of them."""
    names = _DROPIN if only is None else {k: _DROPIN[k] for k in only}
    for public, rel in names.items():
        sys.modules[public] = importlib.import_module(rel, __name__)


# the modules of the reference's video generator that this package mirrors, kept apart from _DROPIN, which is what train_4DGS.py /
# render_4DGS.py import.  _VIDEO_DROPIN: the three modules whose names .cinemagraph mirrors (the generator's warp: the Euler
# integration, the splat, warp_one_level).  _STYLEGAN_OP_DROPIN: the `op` package of its StyleGAN2 and that package's two
# submodules, whose names .stylegan_op mirrors (upfirdn2d and the fused bias + leaky ReLU, which the reference compiles from CUDA
# sources at import); the model files that import them and the checkpoints stay the caller's
_VIDEO_DROPIN = ("thirdparty.StyleCineGAN.utils.softmax_splatting", "thirdparty.StyleCineGAN.utils.joint_splatting",
                 "thirdparty.StyleCineGAN.utils.cinemagraph_utils")
_STYLEGAN_OP_DROPIN = ("thirdparty.StyleCineGAN.models.stylegan2.op", "thirdparty.StyleCineGAN.models.stylegan2.op.fused_act",
                       "thirdparty.StyleCineGAN.models.stylegan2.op.upfirdn2d")


def install_video_dropin() -> None:
    """Register .cinemagraph under the names the reference's video generator imports its warp from (`from
    thirdparty.StyleCineGAN.utils.softmax_splatting import FunctionSoftsplat`, `...utils.joint_splatting import joint_splatting,
    backwarp`, `...utils.cinemagraph_utils import warp_one_level, ...`), so that its cupy kernel is never compiled, and
    .stylegan_op under the names its StyleGAN2 imports its native ops from (`from thirdparty.StyleCineGAN.models.stylegan2.op import
    FusedLeakyReLU, fused_leaky_relu, upfirdn2d`, `...op.fused_act`, `...op.upfirdn2d`), so that its CUDA sources are never
    compiled.  The parent packages are the caller's own (a checkout of the reference on sys.path); one that cannot be imported is
    stood in for by an empty package."""
    import types
    warp, op = importlib.import_module(".cinemagraph", __name__), importlib.import_module(".stylegan_op", __name__)
    for public, module in [(n, warp) for n in _VIDEO_DROPIN] + [(n, op) for n in _STYLEGAN_OP_DROPIN]:
        parts = public.split(".")
        for i in range(1, len(parts)):
            name = ".".join(parts[:i])
            if name not in sys.modules:
                try:
                    importlib.import_module(name)
                except ImportError:
                    pkg = types.ModuleType(name)
                    pkg.__path__ = []
                    sys.modules[name] = pkg
                    if i > 1:
                        setattr(sys.modules[".".join(parts[:i - 1])], parts[i - 1], pkg)
        sys.modules[public] = module
        parent = sys.modules[".".join(parts[:-1])]
        if parent is not module:       # op.upfirdn2d stays the function, as the reference's op/__init__.py leaves it
            setattr(parent, parts[-1], module)
