"""The render script's body (reference render_4DGS.py:45-91: render_set / render_sets) on libmom4d.

What render_set produces is the reference's: <model_path>/frame_result/<name>/%05d.png -- every frame of the path, quantised
like torchvision.utils.save_image -- and, when imageio is installed, <model_path>/vid_result/<name>.mp4 of the frames cropped by
32 pixels.  How it gets there differs: the reference encodes each PNG inside the render loop, on the thread that also launches
the kernels, so its printed FPS is the PNG encoder's (render_4DGS.py:60-71).  Here the loop only enqueues GPU work -- render,
one quantisation kernel (mom_image_to_rgb8), an async copy into a ring of pinned host buffers -- and a pool of threads encodes
finished frames behind it (PIL releases the GIL inside zlib).  With MOM_PNG_ENCODER=device (or AsyncPNGWriter(encoder="device"))
the frame is deflated on the GPU as well (mom_png_encode, csrc/png_encode.hip): what crosses to the host is a finished zlib
stream, and the threads only frame it in PNG chunks and write it.  `scripted=True` keeps the reference's blocking order for
comparison.  Frames whose binning buffer overflowed in async mode are rendered again at the end (FusedRender.overflowed).

The video: MOM_VIDEO_ENCODER unset (or "imageio") is the reference's imageio.mimwrite of the retained frames, when imageio is
installed.  "device" and "host" need nothing installed but Pillow: vid_result/<name>.avi, Motion-JPEG -- every cropped frame a
baseline JPEG (AsyncVideoWriter), encoded behind the frame's own kernels on the frame's stream (mom_jpeg_encode_chw,
csrc/jpeg_encode.hip; only the finished file crosses to the host), or by PIL on the worker threads with the same bytes as result."""
import contextlib
import io
import os
import queue
import struct
import threading
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import _native as N
from . import gaussian_renderer as GR
from .gaussian_renderer import render
from .utils.image_io import save_image, save_uint8, save_zlib_stream


# zlib level of the asynchronous writer's PNGs.  PNG is lossless at every level: the decoded pixels are the same bytes, only the
# files are larger (1.2 MB instead of 1.0 MB per 960x540 frame of the synthetic scene) -- and deflate is what the as-scripted
# render loop waits for (a frame takes 0.26 ms to render and ~35 ms of one host core to compress at level 6, torchvision's / PIL's
# default, which the blocking order `scripted=True` keeps).
PNG_COMPRESS_LEVEL = int(os.environ.get("MOM_PNG_LEVEL", "1"))
PNG_ENCODERS = ("host", "device")      # MOM_PNG_ENCODER / AsyncPNGWriter(encoder=): who deflates the asynchronous writer's frames


def png_encoder(encoder=None):
    """"host" or "device": the argument, or MOM_PNG_ENCODER when it is None (unset or empty: "host"); anything else is a ValueError."""
    if encoder is None:
        encoder = os.environ.get("MOM_PNG_ENCODER") or "host"
    if encoder not in PNG_ENCODERS:
        raise ValueError(f"the PNG encoder must be one of {PNG_ENCODERS}, got {encoder!r}")
    return encoder


class AsyncPNGWriter:
    """submit(image [3,H,W] on the GPU, path): quantise on the device, copy to a pinned slot behind the frame's kernels, encode on
    a worker thread.  At most `slots` frames are in flight; submit() blocks only when all slots are busy.

    encoder: "host" (the default; None reads MOM_PNG_ENCODER) -- the raw bytes cross to the host and a worker deflates them with
    zlib at `compress_level`, filter type 0; "device" -- mom_png_encode makes the IDAT's zlib stream behind the quantisation kernel
    (row filters, constant Huffman tables, run-length matches), the slot's pinned buffer receives the stream and its length in one
    copy, and the worker only adds the chunk framing and the CRC.  Both files decode to the same bytes.  A frame the device encoder
    does not take (a channel count other than 1, 3, 4; a tensor that is not on the GPU) goes the host way."""

    def __init__(self, H, W, C=3, slots=48, workers=None, compress_level=None, encoder=None):
        self.H, self.W, self.C = H, W, C
        self.encoder = encoder = png_encoder(encoder)
        self.zcap = 0                       # device encoder: the stream's capacity, a multiple of 16; its length word follows
        if encoder == "device":
            bound = int(N.lib().mom_png_bound(C, H, W))
            if bound:
                self.zcap = (bound + 15) & ~15
                self.zhost = [torch.empty(self.zcap + 4, dtype=torch.uint8).pin_memory() for _ in range(slots)]
                self.zdev = [None] * slots      # (stream and length word, scratch) per slot
        self.level = PNG_COMPRESS_LEVEL if compress_level is None else int(compress_level)
        self.host = [torch.empty((H, W, C), dtype=torch.uint8).pin_memory() for _ in range(slots)]
        self.dev = [None] * slots
        self.free = queue.Queue()
        for i in range(slots):
            self.free.put(i)
        self.pool = ThreadPoolExecutor(max_workers=workers or min(slots, max(4, (os.cpu_count() or 8) // 2)))
        self.futures = []
        list(self.pool.map(lambda _: time.sleep(0.002), range(self.pool._max_workers)))     # start the threads now, not per frame

    def submit(self, image, path):
        slot = self.free.get()
        if self.dev[slot] is None or self.dev[slot].device != image.device:
            self.dev[slot] = torch.empty((self.H, self.W, self.C), dtype=torch.uint8, device=image.device)
        img = image if (image.is_contiguous() and image.dtype == torch.float32) else image.contiguous().float()
        N.check(N.lib().mom_image_to_rgb8(self.C, self.H, self.W, img.data_ptr(), self.dev[slot].data_ptr(), N.current_stream()),
                "mom_image_to_rgb8")
        if self.zcap and image.is_cuda:
            if self.zdev[slot] is None or self.zdev[slot][0].device != image.device:
                self.zdev[slot] = (torch.empty(self.zcap + 4, dtype=torch.uint8, device=image.device),
                                   torch.empty(N.lib().mom_png_scratch_bytes(self.C, self.H, self.W), dtype=torch.uint8,
                                               device=image.device))
            z, scratch = self.zdev[slot]
            N.check(N.lib().mom_png_encode(self.C, self.H, self.W, self.dev[slot].data_ptr(), z.data_ptr(), self.zcap,
                                           z.data_ptr() + self.zcap, scratch.data_ptr(), N.current_stream()), "mom_png_encode")
            self.zhost[slot].copy_(z, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            self.futures.append(self.pool.submit(self._frame, slot, ev, path))
            return
        self.host[slot].copy_(self.dev[slot], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self.futures.append(self.pool.submit(self._encode, slot, ev, path))

    def submit_rgb8(self, rgb8, path):
        """submit() without its quantisation launch, for a frame that is bytes already: rgb8 [H,W,C] uint8, contiguous, on the GPU
        (what ops.pil_resize writes).  Everything that reads rgb8 is enqueued on the current stream before this returns, so the caller
        may overwrite it with work enqueued on that stream afterwards.  Both encoders."""
        if not (torch.is_tensor(rgb8) and rgb8.is_cuda and rgb8.dtype == torch.uint8 and rgb8.is_contiguous()
                and tuple(rgb8.shape) == (self.H, self.W, self.C)):
            raise N.MomError(f"submit_rgb8 takes a contiguous uint8 [{self.H},{self.W},{self.C}] tensor on the GPU, got "
                             + (f"{rgb8.dtype} {list(rgb8.shape)} on {rgb8.device}" if torch.is_tensor(rgb8) else type(rgb8).__name__))
        slot = self.free.get()
        if self.zcap:
            if self.zdev[slot] is None or self.zdev[slot][0].device != rgb8.device:
                self.zdev[slot] = (torch.empty(self.zcap + 4, dtype=torch.uint8, device=rgb8.device),
                                   torch.empty(N.lib().mom_png_scratch_bytes(self.C, self.H, self.W), dtype=torch.uint8,
                                               device=rgb8.device))
            z, scratch = self.zdev[slot]
            N.check(N.lib().mom_png_encode(self.C, self.H, self.W, rgb8.data_ptr(), z.data_ptr(), self.zcap,
                                           z.data_ptr() + self.zcap, scratch.data_ptr(), N.current_stream()), "mom_png_encode")
            self.zhost[slot].copy_(z, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            self.futures.append(self.pool.submit(self._frame, slot, ev, path))
            return
        self.host[slot].copy_(rgb8, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self.futures.append(self.pool.submit(self._encode, slot, ev, path))

    def _frame(self, slot, ev, path):
        try:
            ev.synchronize()
            z = self.zhost[slot].numpy()
            size = int(z[self.zcap:].view(np.uint32)[0])
            if not 8 <= size <= self.zcap:
                raise N.MomError(f"mom_png_encode reported a stream of {size} bytes for {path} (capacity {self.zcap})")
            save_zlib_stream(memoryview(z)[:size], path, self.H, self.W, self.C)
        finally:
            self.free.put(slot)

    def _encode(self, slot, ev, path):
        try:
            ev.synchronize()
            save_uint8(self.host[slot].numpy(), path, self.level)
        finally:
            self.free.put(slot)

    def drain(self):
        for f in self.futures:
            f.result()
        self.futures.clear()

    def close(self):
        self.drain()
        self.pool.shutdown()


VIDEO_ENCODERS = ("imageio", "host", "device")       # MOM_VIDEO_ENCODER: who makes render_set's video
JPEG_PIL_OPTIONS = dict(subsampling=2, optimize=False)          # with quality and restart_marker_blocks: the file mom_jpeg_encode writes


def video_encoder(encoder=None):
    """"imageio", "host" or "device": the argument, or MOM_VIDEO_ENCODER when it is None (unset or empty: "imageio", the reference's
    vid_result/<name>.mp4 where imageio is installed); anything else is a ValueError."""
    if encoder is None:
        encoder = os.environ.get("MOM_VIDEO_ENCODER") or "imageio"
    if encoder not in VIDEO_ENCODERS:
        raise ValueError(f"the video encoder must be one of {VIDEO_ENCODERS}, got {encoder!r}")
    return encoder


def avi_file(frames, H, W, fps=30):
    """The bytes of an AVI file with one Motion-JPEG video stream: RIFF 'AVI ' = LIST 'hdrl' (avih, LIST 'strl' (strh, strf)),
    LIST 'movi' (one 00dc chunk per frame, padded to even length), idx1.  No OpenDML: a file of 2^31 bytes or more is refused."""
    fps = int(fps)
    chunk = lambda cc, body: cc + struct.pack("<I", len(body)) + body + (b"\0" if len(body) & 1 else b"")
    biggest = max((len(f) for f in frames), default=0)
    total = sum(8 + len(f) + (len(f) & 1) for f in frames)
    if total + 16 * len(frames) + 4096 >= 1 << 31:
        raise ValueError(f"the video would be {total} bytes: an AVI without OpenDML extensions ends below 2^31")
    avih = struct.pack("<14I", 1000000 // fps, biggest * fps, 0, 0x10, len(frames), 0, 1, biggest, W, H, 0, 0, 0, 0)
    strh = b"vids" + b"MJPG" + struct.pack("<IHHIIIIIIII", 0, 0, 0, 0, 1, fps, 0, len(frames), biggest, 0xFFFFFFFF, 0) \
        + struct.pack("<4h", 0, 0, W, H)
    strf = struct.pack("<IiiHH4sIiiII", 40, W, H, 1, 24, b"MJPG", 3 * W * H, 0, 0, 0, 0)
    hdrl = chunk(b"LIST", b"hdrl" + chunk(b"avih", avih) + chunk(b"LIST", b"strl" + chunk(b"strh", strh) + chunk(b"strf", strf)))
    movi, index, at = [b"movi"], [], 4
    for f in frames:
        movi.append(chunk(b"00dc", f))
        index.append(struct.pack("<4sIII", b"00dc", 0x10, at, len(f)))
        at += len(movi[-1])
    body = b"AVI " + hdrl + chunk(b"LIST", b"".join(movi)) + chunk(b"idx1", b"".join(index))
    return b"RIFF" + struct.pack("<I", len(body)) + body


class AsyncVideoWriter:
    """submit(image [3,IH,IW] floats, index, y0, x0): the H x W window at (y0, x0) becomes frame `index` of a Motion-JPEG AVI,
    quantised like the reference's to8b; close() writes the file, frames in index order.  Submitting an index again replaces
    that frame (render_set renders frames again whose binning buffer overflowed).

    encoder: "device" -- mom_jpeg_encode_chw runs behind the frame's kernels on the current stream; the slot's pinned buffer
    receives the length word and the first `prefix` bytes of the file in one copy (a frame of a rendered scene is far below
    the worst-case capacity the encoder asks for), and a worker fetches the rest in the rare case that there is more; "host"
    -- the window crosses to the host and a worker encodes it with PIL, whose file has the same DQT, SOF0, DHT, DRI, SOS and scan
    (a CPU tensor always goes this way).  None reads MOM_VIDEO_ENCODER; unset, or "imageio", which is not this writer's: "host"."""

    def __init__(self, path, H, W, fps=30, quality=None, encoder=None, slots=16, workers=None):
        if encoder is None:
            encoder = video_encoder()
            encoder = "host" if encoder == "imageio" else encoder
        if encoder not in ("host", "device"):
            raise ValueError(f"AsyncVideoWriter encodes on the \"host\" or the \"device\", got {encoder!r}")
        self.quality = int(os.environ.get("MOM_VIDEO_QUALITY") or 90) if quality is None else int(quality)
        if not 1 <= self.quality <= 100:
            raise ValueError(f"the JPEG quality must be in 1..100, got {self.quality}")
        if H < 1 or W < 1:
            raise ValueError(f"the video's frame is empty: {H} x {W}")
        self.path, self.H, self.W, self.fps, self.encoder = path, H, W, fps, encoder
        self.frames, self.lock = {}, threading.Lock()
        self.restart = _jpeg_restart()
        self.cap = 0
        if encoder == "device":
            self.cap = int(N.lib().mom_jpeg_bound(H, W))
            if not self.cap:
                raise ValueError(f"mom_jpeg_encode does not take a frame of {H} x {W}")
            self.prefix = min(self.cap, max(4096, (H * W * 3 // 4 + 15) & ~15))
            self.zhost = [torch.empty(16 + self.prefix, dtype=torch.uint8).pin_memory() for _ in range(slots)]
            self.zdev = [None] * slots          # (length word and file, scratch) per slot
        self.free = queue.Queue()
        for i in range(slots):
            self.free.put(i)
        self.pool = ThreadPoolExecutor(max_workers=workers or min(slots, max(4, (os.cpu_count() or 8) // 2)))
        self.futures = []

    def submit(self, image, index, y0=0, x0=0):
        IH, IW = int(image.shape[1]), int(image.shape[2])
        if image.shape[0] != 3 or y0 < 0 or x0 < 0 or y0 + self.H > IH or x0 + self.W > IW:
            raise ValueError(f"the window {self.H} x {self.W} at ({y0}, {x0}) is not inside an image of shape {tuple(image.shape)}")
        if self.encoder == "device" and image.is_cuda:
            slot = self.free.get()
            if self.zdev[slot] is None or self.zdev[slot][0].device != image.device:
                self.zdev[slot] = (torch.empty(16 + self.cap, dtype=torch.uint8, device=image.device),
                                   torch.empty(N.lib().mom_jpeg_scratch_bytes(self.H, self.W), dtype=torch.uint8, device=image.device))
            z, scratch = self.zdev[slot]
            img = image if (image.is_contiguous() and image.dtype == torch.float32) else image.contiguous().float()
            N.check(N.lib().mom_jpeg_encode_chw(IH, IW, y0, x0, self.H, self.W, img.data_ptr(), self.quality, z.data_ptr() + 16, self.cap,
                                                z.data_ptr(), scratch.data_ptr(), N.current_stream()), "mom_jpeg_encode_chw")
            self.zhost[slot].copy_(z[:16 + self.prefix], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            self.futures.append(self.pool.submit(self._collect, slot, ev, index))
            return
        window = image[:, y0:y0 + self.H, x0:x0 + self.W]
        self.futures.append(self.pool.submit(self._encode, to8b(window).transpose(1, 2, 0), index))

    def _collect(self, slot, ev, index):
        try:
            ev.synchronize()
            z = self.zhost[slot].numpy()
            size = int(z[:4].view(np.uint32)[0])
            if not 0 < size <= self.cap:
                raise N.MomError(f"mom_jpeg_encode_chw reported a file of {size} bytes for frame {index} (capacity {self.cap})")
            data = z[16:16 + min(size, self.prefix)].tobytes()
            if size > self.prefix:                  # the event says the whole file is in the slot's device buffer
                data += self.zdev[slot][0][16 + self.prefix:16 + size].cpu().numpy().tobytes()
            with self.lock:
                self.frames[index] = data
        finally:
            self.free.put(slot)

    def _encode(self, rgb8, index):
        from PIL import Image
        buf = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(rgb8)).save(buf, "JPEG", quality=self.quality, restart_marker_blocks=self.restart,
                                                         **JPEG_PIL_OPTIONS)
        with self.lock:
            self.frames[index] = buf.getvalue()

    def drain(self):
        for f in self.futures:
            f.result()
        self.futures.clear()

    def close(self):
        """Waits for the frames and writes the file; returns its path."""
        try:
            self.drain()
        finally:
            self.pool.shutdown()
        data = avi_file([self.frames[k] for k in sorted(self.frames)], self.H, self.W, self.fps)
        os.makedirs(os.path.dirname(os.path.abspath(self.path)), exist_ok=True)
        with open(self.path, "wb") as f:
            f.write(data)
        return self.path


def _jpeg_restart():
    """The restart interval of mom_jpeg_encode's files, in MCUs (the host route asks PIL for the same)."""
    import ctypes as C
    quant, counts, symbols, n, r = (C.c_uint8 * 128)(), (C.c_uint8 * 64)(), (C.c_uint8 * 648)(), (C.c_int * 4)(), C.c_int(0)
    N.check(N.lib().mom_jpeg_tables(90, quant, counts, symbols, n, C.byref(r)), "mom_jpeg_tables")
    return r.value


# Streams render_set deals consecutive frames to when it writes them asynchronously (1: every frame on the current stream).  Two,
# not three: the device has four hardware queues, and a process that has trained (the step's two streams) and then renders on three
# more lands two of them on one queue -- 4400 frames/s instead of 5700, where two streams give 5300 every time
# (tools/probe/fps_leg.py).
RENDER_STREAMS = 2

to8b = lambda x: (255 * np.clip(x.cpu().numpy(), 0, 1)).astype(np.uint8)      # render_4DGS.py:44


def render_set(model_path, name, iteration, views, gaussians, pipeline, background, cam_type, delta_scale=1, scripted=False,
               video=True, writer=None):
    """Returns {"frames", "seconds", "fps"}: fps = (frames - 1) / seconds from the start of the first render to the last PNG on
    disk (the reference's definition, render_4DGS.py:61,70-71, made honest about the writes it overlaps)."""
    render_path = os.path.join(model_path, 'frame_result', name)
    os.makedirs(render_path, exist_ok=True)
    print("point nums:", gaussians._xyz.shape[0])
    views = list(views)
    fr = None
    streams_before = GR.render_streams()
    if gaussians._xyz.is_cuda:
        # the forward-only launch sequence reports async-mode overflows per frame; collect them instead of raising mid-loop
        from .fused_render import FusedRender, FusedRenderPool
        if not scripted and RENDER_STREAMS > 1:
            # consecutive frames on alternating streams (FusedRenderPool): every frame is quantised and copied to the host on the
            # stream it was rendered on, so nothing here ever waits for a frame on another stream
            GR.set_render_streams(RENDER_STREAMS)
            fr = getattr(gaussians, "_fused_render_pool", None)
            if fr is None or fr.n != RENDER_STREAMS:
                fr = gaussians._fused_render_pool = FusedRenderPool(gaussians, RENDER_STREAMS)
        else:
            GR.set_render_streams(1)
            fr = getattr(gaussians, "_fused_render", None)
            if fr is None:
                fr = gaussians._fused_render = FusedRender(gaussians)
        fr.collect, fr.bad = True, []
    try:
        return _render_set_body(model_path, name, views, gaussians, pipeline, background, cam_type, delta_scale, scripted, video, writer,
                                render_path, fr)
    finally:
        GR.set_render_streams(streams_before)
        if fr is not None:
            fr.collect = False


def _render_set_body(model_path, name, views, gaussians, pipeline, background, cam_type, delta_scale, scripted, video, writer,
                     render_path, fr):
    own_writer = None
    crop = 32
    frames, images = [], []
    venc = video_encoder() if video else None           # refused before anything is rendered
    vw = None                                           # the Motion-JPEG writer of the "host" and "device" routes
    with torch.no_grad():
        t0 = time.time()
        pooled = fr is not None and hasattr(fr, "slots")
        first = fr.count if pooled else (fr.serial if fr is not None else 0)      # the loop's frame 0 in the renderer's numbering
        for idx, view in enumerate(views):
            out = render(view, gaussians, pipeline, background, cam_type=cam_type, delta_scale=delta_scale)
            rendering = out["render"]
            path = os.path.join(render_path, '{0:05d}'.format(idx) + ".png")
            if scripted or not rendering.is_cuda:
                save_image(rendering, path)                      # blocking, inside the loop: the reference's order
            else:
                if writer is None and own_writer is None:
                    own_writer = AsyncPNGWriter(rendering.shape[1], rendering.shape[2])
                with (torch.cuda.stream(out["stream"]) if "stream" in out else contextlib.nullcontext()):
                    (writer or own_writer).submit(rendering, path)
            frames.append((idx, view, path))
            if venc in ("host", "device"):
                if vw is None:
                    vh, vwid = rendering.shape[1] - 2 * crop, rendering.shape[2] - 2 * crop
                    if vh < 1 or vwid < 1:
                        raise ValueError(f"a frame of {rendering.shape[1]} x {rendering.shape[2]} is empty after the video's crop of "
                                         f"{crop} pixels on every side")
                    vw = AsyncVideoWriter(os.path.join(model_path, 'vid_result', name + '.avi'), vh, vwid, fps=30,
                                          encoder=venc if (rendering.is_cuda and not scripted) else "host")
                with (torch.cuda.stream(out["stream"]) if "stream" in out else contextlib.nullcontext()):
                    vw.submit(rendering, idx, crop, crop)          # on the stream the frame was rendered on, like the PNG
            elif video:
                images.append(rendering)
        w = writer or own_writer
        if w is not None:
            # async binning: frames flagged as overflowed are rendered again (the capacity was raised), before the clock stops
            bad = (fr.bad + fr.overflowed()) if fr is not None else []
            if fr is not None:
                fr.bad = []
            if bad:
                from .diff_gaussian_rasterization import _C as RC
                mode = RC._state["mode"]
                RC._state["mode"] = "exact"                       # the repairs size their buffer from their own instance count
                GR.set_render_streams(1)                          # ... on the current stream, one after the other
                torch.cuda.synchronize()
                try:
                    for s in bad:
                        idx = (s - first) if pooled else (s - first - 1)       # a pool numbers frames from 0, a FusedRender's serial counts from 1
                        if 0 <= idx < len(views):
                            rendering = render(views[idx], gaussians, pipeline, background, cam_type=cam_type, delta_scale=delta_scale)["render"]
                            w.submit(rendering, frames[idx][2])
                            if vw is not None:
                                vw.submit(rendering, idx, crop, crop)
                            elif video:
                                images[idx] = rendering
                finally:
                    RC._state["mode"] = mode
            w.drain()
        if rendering.is_cuda:
            torch.cuda.synchronize()
        dt = time.time() - t0
    fps = (len(views) - 1) / dt if dt > 0 else float("inf")
    print("FPS:", fps)
    if own_writer is not None:
        own_writer.close()
    if vw is not None:
        vw.close()
    elif video:
        try:
            import imageio
            video_path = os.path.join(model_path, 'vid_result')
            os.makedirs(video_path, exist_ok=True)
            imageio.mimwrite(os.path.join(video_path, name + '.mp4'),
                             [to8b(im).transpose(1, 2, 0)[crop:-crop, crop:-crop] for im in images], fps=30)
        except ImportError:
            print("imageio is not installed: skipping vid_result/" + name + ".mp4 (the PNG frames are complete)")
    return {"frames": len(views), "seconds": dt, "fps": fps}


def render_sets(dataset, hyperparam, iteration, pipeline, skip_train, skip_test, skip_video, TrainData_path, Gaussian_path, **kw):
    """render_4DGS.py:77-91.  One AsyncPNGWriter serves the four trajectories."""
    from .scene import GaussianModel, Scene
    with torch.no_grad():
        gaussians = GaussianModel(dataset.sh_degree, hyperparam)
        scene = Scene(TrainData_path, Gaussian_path, dataset, gaussians, load_iteration=iteration, shuffle=False)
        dev = gaussians._xyz.device
        background = torch.tensor([1, 1, 1] if dataset.white_background else [0, 0, 0], dtype=torch.float32, device=dev)
        out = {}
        writer = None
        if dev.type == "cuda" and not kw.get("scripted") and "writer" not in kw:
            c0 = scene.getVideoCameras_up()[0]
            writer = kw["writer"] = AsyncPNGWriter(int(c0.image_height), int(c0.image_width))
        try:
            for name, cams in (("up_down", scene.getVideoCameras_up()), ("side", scene.getVideoCameras_side()),
                               ("zoom", scene.getVideoCameras_zoom()), ("circle", scene.getVideoCameras_circle())):
                out[name] = render_set(Gaussian_path, name, scene.loaded_iter, cams, gaussians, pipeline, background,
                                       scene.dataset_type, **kw)
        finally:
            if writer is not None:
                writer.close()
    return out
