"""The warp of the reference's video generator (thirdparty/StyleCineGAN) on libmom4d, and a video made with it alone.

The reference turns one image and its Eulerian flow (stage 1's `our_flow`) into a looping video by warping the deep features of a
StyleGAN: per frame and per warped level, `warp_one_level` integrates the flow forwards and backwards (`euler_integration`), splats
the level's features along both displacements (`joint_splatting` on a CUDA string compiled through cupy) and fills the holes.  This
module mirrors the names of the three reference modules that hold that warp --

    thirdparty/StyleCineGAN/utils/softmax_splatting.py   FunctionSoftsplat, ModuleSoftsplat, _FunctionSoftsplat
    thirdparty/StyleCineGAN/utils/joint_splatting.py     joint_splatting, backwarp
    thirdparty/StyleCineGAN/utils/cinemagraph_utils.py   euler_integration, pad_tensor, crop_padded_tensor, resize_flow, resize_feature,
                                                         blend_feature, feature_inpaint_conv, warp_one_level, feature_inpaint

-- with the reference's signatures, on the kernels of csrc/eulerian_warp.hip (`install_video_dropin()` of the package registers it
under those three names).  Forward only: the generator runs under no_grad.

The same call registers stylegan_op.py, the mirror of the generator's other native dependency -- the `op` package of its StyleGAN2
(models/stylegan2/op: upfirdn2d and the fused bias + leaky ReLU) -- under `thirdparty.StyleCineGAN.models.stylegan2.op`, so the
reference's model.py, which imports `warp_one_level` from here and those ops from there, imports on ROCm.  The model files and the
checkpoints are not mirrored.

`pixel_video` is NOT the reference's output.  The reference's frames come out of StyleGAN, which needs a model file and checkpoints
this package does not have; `pixel_video` warps the PIXELS of the input image with the same `warp_one_level` and composites them like the reference
(main_jih.py:160-161).  It is a substitute that makes stage 2 runnable from this package's own stage-1 outputs, no more.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from . import ops
from ._native import MomError

# warp_one_level's default route: the two-launch fused route, or the reference's op sequence (DESIGN.md 3.18 has the measurement
# that decides it)
FUSED_DEFAULT = True
# ops.eulerian_blend's form per channel count (both forms measured for C = 1 and 3)
SMALL_C_FORM = "channels"


# ----------------------------------------------------------------------------------------------- utils/softmax_splatting.py
class _FunctionSoftsplat(torch.autograd.Function):
    """The summation splat (softmax_splatting.py:236-269) on ops.softsplat_sum."""
    @staticmethod
    def forward(ctx, input, flow, ordered=None):
        assert flow.shape[1] == 2 and input.shape[2:] == flow.shape[2:]
        assert input.is_contiguous() and flow.is_contiguous()
        return ops.softsplat_sum(input.detach(), flow.detach(), ordered=ordered)

    @staticmethod
    def backward(ctx, gradOutput):
        raise NotImplementedError("the splat's backward (softmax_splatting.py:271-322) is not built: the video generator calls the "
                                  "warp under torch.no_grad() only")


def FunctionSoftsplat(tensorInput, tensorFlow, tensorMetric, strType, output_size=None, ordered=None):
    """softmax_splatting.py:325-349.  ordered: ops.softsplat_sum's (None follows _C.set_deterministic); the reference's signature
    stays callable as it is."""
    assert tensorMetric is None or tensorMetric.shape[1] == 1
    assert strType in ['summation', 'average', 'linear', 'softmax']
    if strType == 'average':
        tensorInput = torch.cat([tensorInput, tensorInput.new_ones(tensorInput.shape[0], 1, *tensorInput.shape[2:])], 1)
    elif strType == 'linear':
        tensorInput = torch.cat([tensorInput * tensorMetric, tensorMetric], 1)
    elif strType == 'softmax':
        tensorInput = torch.cat([tensorInput * tensorMetric.exp(), tensorMetric.exp()], 1)
    tensorOutput = _FunctionSoftsplat.apply(tensorInput.contiguous(), tensorFlow.contiguous(), ordered)
    if strType != 'summation':
        metric = tensorOutput[:, -1:, :, :]
        metric[metric == 0] = 1
        tensorOutput = tensorOutput[:, :-1, :, :] / metric
    if output_size is not None:
        tensorOutput = tensorOutput[:, :, :output_size[0], :output_size[1]]
    return tensorOutput


class ModuleSoftsplat(torch.nn.Module):
    def __init__(self, strType):
        super().__init__()
        self.strType = strType

    def forward(self, tensorInput, tensorFlow, tensorMetric, output_size=None, ordered=None):
        return FunctionSoftsplat(tensorInput, tensorFlow, tensorMetric, self.strType, output_size, ordered=ordered)


# ----------------------------------------------------------------------------------------------- utils/joint_splatting.py
backwarp_tenGrid = {}


def backwarp(tenIn, tenFlow):
    key = (str(tenFlow.shape), str(tenFlow.device))
    if key not in backwarp_tenGrid:
        H, W = tenFlow.shape[2:]
        hor = torch.linspace(-1.0 + (1.0 / W), 1.0 - (1.0 / W), W).view(1, 1, 1, -1).repeat(1, 1, H, 1)
        ver = torch.linspace(-1.0 + (1.0 / H), 1.0 - (1.0 / H), H).view(1, 1, -1, 1).repeat(1, 1, 1, W)
        backwarp_tenGrid[key] = torch.cat([hor, ver], 1).to(tenFlow.device)
    tenFlow = torch.cat([tenFlow[:, 0:1] / ((tenIn.shape[3] - 1.0) / 2.0), tenFlow[:, 1:2] / ((tenIn.shape[2] - 1.0) / 2.0)], 1)
    return F.grid_sample(input=tenIn, grid=(backwarp_tenGrid[key] + tenFlow).permute(0, 2, 3, 1), mode='bilinear',
                         padding_mode='zeros', align_corners=False)


def joint_splatting(feature_map1, weights1, flow1, feature_map2, weights2, flow2, mode="full", output_size=None, ordered=None):
    assert feature_map1.shape == feature_map2.shape
    assert flow1.shape == flow2.shape
    assert feature_map1.shape[-2:] == flow1.shape[-2:]
    flow2_offset = flow2.clone()
    flow2_offset[:, 0, :, :] -= feature_map1.shape[-1]
    flow = torch.cat([flow1, flow2_offset], dim=-1)
    feature_map = torch.cat([feature_map1, feature_map2], dim=-1)
    blending_weights = torch.cat([weights1, weights2], dim=-1)
    if mode == "full":
        return FunctionSoftsplat(tensorInput=feature_map, tensorFlow=flow, tensorMetric=blending_weights, strType='linear',
                                 output_size=output_size, ordered=ordered)
    if mode == "no_forward_warping":
        result = backwarp(feature_map, flow)
        if output_size is not None:
            result = result[:, :, :output_size[0], :output_size[1]]
        return result
    raise ValueError(f"joint_splatting: mode must be 'full' or 'no_forward_warping', got {mode!r}")


# ----------------------------------------------------------------------------------------------- utils/cinemagraph_utils.py
def _device(t):
    """Where the reference says .cuda(): the tensor's own device if it is on one already, else the current one."""
    return t.device if t.is_cuda else torch.device("cuda", torch.cuda.current_device())


def euler_integration(motion, destination_frame, return_all_frames=False):
    """cinemagraph_utils.py:9-59 in one launch (ops.euler_integrate).  motion [1,2,H,W] -> (displacements, visible_pixels): the
    displacement to frame `destination_frame` [1,2,H,W], or to every frame [destination_frame+1,2,H,W]."""
    assert motion.dim() == 4
    b, c, height, width = motion.shape
    assert b == 1, 'Function only implemented for batch = 1'
    assert c == 2, f'Input motion field should be Bx2xHxW. Given tensor is: {motion.shape}'
    motion = motion.to(_device(motion)).float().contiguous()
    disp = ops.euler_integrate(motion[0], destination_frame, all_frames=return_all_frames)
    visible = torch.ones((b + 1 if return_all_frames else 1), 1, height, width, device=motion.device)
    return (disp if return_all_frames else disp.unsqueeze(0)), visible


def pad_size_of(size):
    return int(size / 4) + int(size / 8)


def cut_size_of(size):
    return {1024: 3, 512: 2, 256: 1}.get(size, 0)


def pad_tensor(tensor, mode="reflect", number=None):
    pad_size = pad_size_of(tensor.size(2))
    if mode == "reflect":
        return F.pad(tensor, (pad_size,) * 4, mode="reflect")
    if mode == "constant":
        return F.pad(tensor, (pad_size,) * 4, "constant", number)
    raise ValueError(f"pad_tensor: mode must be 'reflect' or 'constant', got {mode!r}")


def crop_padded_tensor(padded_tensor, size):
    start = int((padded_tensor.size(2) - size) / 2)
    return padded_tensor[:, :, start:start + size, start:start + size]


def resize_feature(feature, size):
    if feature.size(2) < size:
        while feature.size(2) < size:
            feature = F.interpolate(feature, size=(feature.shape[2] * 2, feature.shape[3] * 2), mode='bilinear', align_corners=False)
    elif feature.size(2) > size:
        feature = F.interpolate(feature, size=(int(feature.shape[2] / 2), int(feature.shape[3] / 2)), mode='bilinear',
                                align_corners=False)
    return feature


def resize_flow(flow, size):
    """Halve or double the flow image, and its values with it, until its height is `size` (cinemagraph_utils.py:105-128).  Like the
    reference it never ends when `size` is not the height times a power of two; that is refused here."""
    h = flow.size(2)
    big, small = max(h, size), min(h, size)
    if small < 1 or big % small or (big // small) & (big // small - 1):
        raise ValueError(f"resize_flow: {h} -> {size} is not a sequence of halvings or doublings")
    first = h
    while flow.size(2) != size:
        down = first > size
        hw = (int(flow.size(2) / 2), int(flow.size(3) / 2)) if down else (int(flow.size(2) * 2), int(flow.size(3) * 2))
        flow = F.interpolate(flow, size=hw, mode='bilinear', align_corners=False)
        flow = flow / 2 if down else flow * 2
    return flow


def _blend_ops(feature, flow, idx, n_frames, ordered=None):
    """blend_feature as the reference's own op sequence (cinemagraph_utils.py:131-178) on the device's euler_integration and splat."""
    size = feature.size(2)
    alpha = idx / (n_frames - 1)
    cut = cut_size_of(size)
    if cut:
        feature = feature[:, :, cut:-cut, cut:-cut]
        flow = flow[:, :, cut:-cut, cut:-cut]
    dev = _device(flow)
    future_flow = pad_tensor(flow, mode="reflect").float().to(dev)
    past_flow = pad_tensor(-flow, mode="reflect").float().to(dev)
    future_flow, _ = euler_integration(future_flow, idx)
    past_flow, _ = euler_integration(past_flow, n_frames - idx - 1)
    Z = torch.ones(1, 1, size - 2 * cut, size - 2 * cut, device=dev)
    future_Z = pad_tensor(Z, mode="reflect") * (1 - alpha)
    past_Z = pad_tensor(Z, mode="reflect") * alpha
    feature = pad_tensor(feature.to(dev), mode="reflect").float()
    return joint_splatting(feature, future_Z, future_flow, feature, past_Z, past_flow, mode="full",
                           output_size=feature.shape[-2:], ordered=ordered).float()


def _fused_args(feature, flow):
    if feature.dim() != 4 or feature.shape[0] != 1 or flow.dim() != 4 or flow.shape[0] != 1:
        raise MomError(f"the warp takes one image at a time ([1,C,S,S] and [1,2,S,S], as the reference's euler_integration does), got "
                       f"{tuple(feature.shape)} and {tuple(flow.shape)}")
    dev = _device(flow)
    return feature[0].to(dev).float().contiguous(), flow[0].to(dev).float().contiguous()


def _form(channels):
    return SMALL_C_FORM if channels <= 3 else "channels"


def blend_feature(feature, flow, idx, n_frames, fused=None, ordered=None):
    """cinemagraph_utils.py:131-178: the feature [1,C,S,S] warped to frame idx of n_frames along flow [1,2,S,S] from both ends of the
    loop and blended, on the cut and reflection-padded domain: [1,C,P,P].  fused (default FUSED_DEFAULT): one blend launch and one
    finish launch; otherwise the reference's sequence of ops.  ordered: as warp_one_level's."""
    if not (FUSED_DEFAULT if fused is None else fused):
        return _blend_ops(feature, flow, idx, n_frames, ordered=ordered)
    f, m = _fused_args(feature, flow)
    acc = ops.eulerian_blend(f, m, idx, n_frames, form=_form(f.shape[0]), ordered=ordered)
    return ops.eulerian_finish(acc, f.shape[1], full=True).unsqueeze(0)


def feature_inpaint_conv(feature, flow, idx, n_frames, fused=None, ordered=None):
    """cinemagraph_utils.py:498-531: the padded blended map with its blank pixels -- those no splat reached -- replaced by the 7 x 7
    box mean.  The reference's sequence: a second blend of a tensor of ones tells the blank pixels apart."""
    bn_feature = torch.ones(1, 1, flow.size(2), flow.size(3), device=feature.device)
    warped_bn_feature = blend_feature(bn_feature, flow, idx, n_frames, fused=fused, ordered=ordered)
    blank_mask = torch.where(warped_bn_feature == 0, 1, 0)
    full_mask = 1 - blank_mask
    if blank_mask.max() == 1:
        weights = torch.ones(1, 1, 7, 7, device=feature.device) / 49
        filtered = torch.zeros_like(feature)
        for i in range(feature.size(1)):
            filtered[:, i] = F.conv2d(feature[:, i].unsqueeze(0), weights, padding=3)
        return blank_mask * filtered + full_mask * feature
    return feature


def warp_one_level(out, flow, idx, n_frames, fused=None, ordered=None):
    """cinemagraph_utils.py:181-190: one level's features [1,C,S,S] at frame idx of n_frames.  fused (default FUSED_DEFAULT): after
    the flow resize, ops.eulerian_blend and ops.eulerian_finish -- the blank mask is the weight accumulator's zeros, the box mean is
    computed at those pixels only, only the crop is written.  fused=False: the reference's sequence of ops on ops.softsplat_sum.
    ordered (None: as diff_gaussian_rasterization._C.deterministic() says): the splat of either route adds in the order
    include/mom4d.h defines ("ordered splat of the video generator's warp") instead of with float atomics, and the result is the same
    bits run after run.  The two routes have different entry orders -- the op-by-op route splats the concatenated double canvas, whose
    entries run row by row over both halves, the fused route takes all of the future half first -- so they need not agree with each
    other in bits, only each with itself."""
    orig_size = out.size(2)
    flow = resize_flow(flow, orig_size)
    if not (FUSED_DEFAULT if fused is None else fused):
        out = _blend_ops(out, flow, idx, n_frames, ordered=ordered)
        out = feature_inpaint_conv(out, flow, idx, n_frames, fused=False, ordered=ordered)
        return crop_padded_tensor(out, orig_size)
    f, m = _fused_args(out, flow)
    acc = ops.eulerian_blend(f, m, idx, n_frames, form=_form(f.shape[0]), ordered=ordered)
    return ops.eulerian_finish(acc, orig_size).unsqueeze(0)


def feature_inpaint(feature, flow, idx, n_frames, mode="full"):
    raise NotImplementedError("feature_inpaint (cinemagraph_utils.py:475-495) runs a fast-marching inpainting on the host, pixel by "
                              "pixel in Python, behind the generator's image_inpainting option, which is off by default; it is not "
                              "built here.  feature_inpaint_conv / warp_one_level fill the blank pixels with the box mean.")


# ----------------------------------------------------------------------------------------------- the pixel video
def _as_uint8_hwc(image, size, what):
    """PIL image or uint8 [H,W(,3)] array -> uint8 array at size x size, resized the way the reference does it (PIL's resize)."""
    from PIL import Image
    if not isinstance(image, Image.Image):
        a = np.asarray(image.cpu() if torch.is_tensor(image) else image)
        if a.dtype != np.uint8:
            raise ValueError(f"pixel_video: {what} must be a PIL image or a uint8 array, got {a.dtype}")
        image = Image.fromarray(a)
    return np.array(image.resize((size, size)))


def pixel_video_frames(image, our_flow, mask, n_frames=120, size=1024, device=None, ordered=None):
    """pixel_video's frames one at a time, where they are made: a generator of n_frames contiguous [size,size,3] float32 tensors in
    [0, 1] on the device, so that a consumer on the device (save_video(writer="device")) never holds the video.  ordered:
    warp_one_level's."""
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    rgb = _as_uint8_hwc(image, size, "image")
    if rgb.ndim != 3 or rgb.shape[2] < 3:
        raise ValueError(f"pixel_video: the image must have three channels, got {rgb.shape}")
    m = _as_uint8_hwc(mask, size, "mask")
    m = m[..., 0] if m.ndim == 3 else m
    with torch.no_grad():
        x = torch.from_numpy(rgb[..., :3].copy()).float().permute(2, 0, 1).unsqueeze(0).to(dev) / 127.5 - 1     # ip_utils.to_tensor
        flow = F.interpolate(torch.as_tensor(our_flow).float().to(dev), size=(size, size), mode='bilinear', align_corners=False)
        up_mask = resize_feature((torch.from_numpy(np.array(m) / 255).unsqueeze(0).unsqueeze(0).to(dev)).float(), size)
    for idx in range(n_frames):
        with torch.no_grad():                       # per frame: a generator must not leave the caller's grad mode switched off
            result = warp_one_level(x, flow, idx, n_frames, ordered=ordered)
            result = result * up_mask + x * (1 - up_mask)
            frame = ((result + 1) / 2).permute(0, 2, 3, 1)[0].contiguous()                                      # ip_utils.to_numpy
        yield frame


def pixel_video(image, our_flow, mask, n_frames=120, size=1024, device=None, ordered=None):
    """A looping video from one image and its Eulerian flow WITHOUT the reference's StyleGAN: the frames of the reference's
    VideoGenerator (thirdparty/StyleCineGAN/main_jih.py) with the input image standing where the GAN's result would.  This is a
    substitute that warps pixels, not the reference's deep-feature output.

    image: PIL image or uint8 [H,W,3]; our_flow [1,2,h,w] (stage 1's, pixels per frame); mask: PIL image or uint8 [H,W], 255 where
    the scene moves.  As main_jih.py:33-39 all three are resized to size x size (the flow bilinearly, its values unscaled, as
    there).  Per frame idx: warp_one_level(image, flow, idx, n_frames), then result mask + image (1 - mask) (:160-161).
    ordered: warp_one_level's (None follows _C.set_deterministic): the same frames, bit for bit, run after run.
    Returns n_frames arrays [size,size,3] float32 in [0, 1], as VideoGenerator does (to_numpy)."""
    return [f.cpu().numpy() for f in pixel_video_frames(image, our_flow, mask, n_frames=n_frames, size=size, device=device,
                                                        ordered=ordered)]


VIDEO_WRITERS = ("host", "device")


def save_video(frames, output_path, W, H, writer=None):
    """The frames as train_motion.save_video names them (train_motion.py:402-412): <output_path>/video/%06d.png at W x H, through
    this package's PNG writer.  No mp4 is written.
    writer "host" (the default, also None): frames are float arrays [h,w,3]; each is quantised with (frame * 255).astype(uint8),
    resized by PIL (bicubic) and deflated by zlib, on the calling thread.  writer "device": frames are [h,w,3] float32 tensors on the
    GPU, taken one at a time as the iterable makes them (pixel_video_frames); each goes through ops.pil_resize(to8b=True) -- the same
    quantisation and PIL's bytes -- and render.AsyncPNGWriter(encoder="device"), so what crosses to the host is the finished zlib
    stream.  The files of both writers decode to the same pixels; their zlib streams differ.  Returns the paths, in frame order."""
    import os
    if writer not in (None,) + VIDEO_WRITERS:
        raise ValueError(f"save_video: writer must be one of {VIDEO_WRITERS}, got {writer!r}")
    out = os.path.join(output_path, "video")
    os.makedirs(out, exist_ok=True)
    paths = []
    if writer == "device":
        from .render import AsyncPNGWriter
        png = AsyncPNGWriter(H, W, 3, slots=8, encoder="device")
        rgb8 = scratch = None
        try:
            for i, frame in enumerate(frames):
                if not (torch.is_tensor(frame) and frame.is_cuda and frame.dim() == 3 and frame.shape[2] == 3):
                    raise MomError("save_video(writer='device') takes [h,w,3] float32 tensors on the GPU (pixel_video_frames), got "
                                   + (f"{frame.dtype} {list(frame.shape)} on {frame.device}" if torch.is_tensor(frame) else type(frame).__name__))
                if rgb8 is None:       # one output and one intermediate for all frames: every use is ordered on the frames' stream
                    rgb8 = torch.empty((H, W, 3), dtype=torch.uint8, device=frame.device)
                    scratch = ops.pil_resize_scratch(frame.shape, (W, H), frame.device)
                ops.pil_resize(frame, (W, H), to8b=True, out=rgb8, scratch=scratch)
                paths.append(os.path.join(out, f"{str(i).zfill(6)}.png"))
                png.submit_rgb8(rgb8, paths[-1])
        finally:
            png.close()
        return paths
    from PIL import Image
    from .utils import image_io
    for i, frame in enumerate(frames):
        a = np.array(Image.fromarray((frame * 255).astype(np.uint8)).resize((W, H)))
        paths.append(os.path.join(out, f"{str(i).zfill(6)}.png"))
        image_io.save_uint8(a, paths[-1])
    return paths
