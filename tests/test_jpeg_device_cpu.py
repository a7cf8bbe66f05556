"""The device JPEG encoder's file, checked without a GPU: mom_jpeg_encode_host runs the coder of csrc/jpeg_dev.h -- the code the
kernels run per thread and per lane, all of it 32-bit integer arithmetic -- serially in the kernels' order, and its file must be
what PIL (libjpeg) writes under the oracle call of tests/jpeg_cases.py: every segment but APPn, and the scan bit for bit.
test_jpeg_device_gpu.py then pins the kernels to this file byte for byte.  Also here: the AVI container, AsyncVideoWriter's host
route and the MOM_VIDEO_ENCODER switch of render_set.

The quantiser divides (csrc/jpeg_dev.h jpeg_quantise), so there is no reciprocal to prove exact."""
import ctypes as C
import importlib
import os
import sys
import types

import numpy as np
import pytest

import jpeg_cases as J

N = importlib.import_module("iclr2025_3d-mom_amd._native")
FAKE = 1 << 20          # a non-null pointer value: the calls below are refused before it could be followed
JPEG_EXPORTS = ("mom_jpeg_bound", "mom_jpeg_scratch_bytes", "mom_jpeg_encode", "mom_jpeg_encode_chw", "mom_jpeg_encode_host",
                "mom_jpeg_tables")


def encode_host(arr, Q, row_stride=None):
    """The host entry's file of `arr`, after the checks every caller wants: MOM_OK, size within the bound, nothing written behind
    the file."""
    lib = N.lib()
    H, W, _ = arr.shape
    bound = lib.mom_jpeg_bound(H, W)
    out = np.full(bound + 64, J.SENTINEL, np.uint8)
    size = C.c_uint32(0)
    a = np.ascontiguousarray(arr)
    stride = 3 * W if row_stride is None else row_stride
    assert lib.mom_jpeg_encode_host(H, W, a.ctypes.data, stride, Q, out.ctypes.data, bound, C.byref(size)) == N.MOM_OK
    assert J.HEADER_BYTES + 3 <= size.value <= bound
    assert (out[size.value:] == J.SENTINEL).all()
    return out[:size.value].tobytes()


@pytest.fixture(scope="module")
def files():
    return {name: encode_host(arr, Q) for name, (arr, Q) in J.cases().items()}


def test_abi_version_and_exports():
    assert N.ABI_VERSION == 8 and N.lib().mom_abi_version() == 8
    for name in JPEG_EXPORTS:
        assert name in N.EXPORTS and hasattr(N.lib(), name)


def test_bound_is_the_formula():
    lib = N.lib()
    shapes = {a.shape[:2] for a, _ in J.cases().values()} | {(540, 960), (1, 65535), (65535, 1), (2160, 3840)}
    for H, W in shapes:
        assert lib.mom_jpeg_bound(H, W) == J.bound_formula(H, W), (H, W)
        assert lib.mom_jpeg_scratch_bytes(H, W) > 0
    for H, W in ((0, 4), (4, 0), (-1, 4), (4, 65536), (65536, 4), (40000, 40000)):
        assert lib.mom_jpeg_bound(H, W) == 0, (H, W)
        assert lib.mom_jpeg_scratch_bytes(H, W) == 0, (H, W)


def test_invalid_arguments_are_refused_before_any_launch_or_write():
    lib = N.lib()
    b = lib.mom_jpeg_bound(20, 24)
    size = C.c_uint32(0)
    sp = C.addressof(size)
    ok = dict(H=20, W=24, rgb8=FAKE, stride=72, Q=90, out=FAKE, cap=b, size=sp, scratch=FAKE)

    def dev(**kw):
        a = dict(ok, **kw)
        return lib.mom_jpeg_encode(a["H"], a["W"], a["rgb8"], a["stride"], a["Q"], a["out"], a["cap"], a["size"], a["scratch"], None)

    def host(**kw):
        a = dict(ok, **kw)
        return lib.mom_jpeg_encode_host(a["H"], a["W"], a["rgb8"], a["stride"], a["Q"], a["out"], a["cap"], a["size"])
    bad = [dict(Q=0), dict(Q=101), dict(Q=-5), dict(H=0), dict(W=0), dict(H=-20), dict(W=65536), dict(cap=b - 1), dict(cap=0),
           dict(rgb8=None), dict(out=None), dict(size=None), dict(stride=71)]
    for kw in bad:
        assert dev(**kw) == N.MOM_EINVAL, kw
        assert host(**kw) == N.MOM_EINVAL, kw
    assert dev(scratch=None) == N.MOM_EINVAL

    def chw(IH=84, IW=88, y0=32, x0=32, H=20, W=24, img=FAKE, Q=90, out=FAKE, cap=b, size=sp, scratch=FAKE):
        return lib.mom_jpeg_encode_chw(IH, IW, y0, x0, H, W, img, Q, out, cap, size, scratch, None)
    for kw in (dict(Q=0), dict(Q=101), dict(H=0), dict(W=-1), dict(cap=b - 1), dict(img=None), dict(out=None), dict(size=None),
               dict(scratch=None), dict(y0=-1), dict(x0=-1), dict(y0=65), dict(x0=65), dict(IH=51), dict(IW=55), dict(IH=0)):
        assert chw(**kw) == N.MOM_EINVAL, kw
    assert size.value == 0
    q, cnt, sym, n, r = (C.c_uint8 * 128)(), (C.c_uint8 * 64)(), (C.c_uint8 * 648)(), (C.c_int * 4)(), C.c_int(0)
    for Q in (0, 101):
        assert lib.mom_jpeg_tables(Q, q, cnt, sym, n, C.byref(r)) == N.MOM_EINVAL
    assert lib.mom_jpeg_tables(90, None, cnt, sym, n, C.byref(r)) == N.MOM_EINVAL
    assert lib.mom_jpeg_tables(90, q, cnt, sym, n, None) == N.MOM_EINVAL


def test_a_capacity_below_the_bound_writes_nothing():
    lib = N.lib()
    arr, Q = J.cases()["noise_44x56_q100"]
    bound = lib.mom_jpeg_bound(44, 56)
    out = np.full(bound + 64, J.SENTINEL, np.uint8)
    size = C.c_uint32(77)
    a = np.ascontiguousarray(arr)
    for cap in (bound - 1, J.HEADER_BYTES, 1):
        assert lib.mom_jpeg_encode_host(44, 56, a.ctypes.data, 3 * 56, Q, out.ctypes.data, cap, C.byref(size)) == N.MOM_EINVAL
        assert (out == J.SENTINEL).all() and size.value == 77


@pytest.mark.parametrize("name", list(J.cases()))
def test_host_file_is_pils(files, name):
    """The golden segments and scan (PIL's, recorded by tools/gen_jpeg_golden.py), and live PIL where this Pillow takes the options."""
    arr, Q = J.cases()[name]
    mine = files[name]
    assert mine[:2] == b"\xff\xd8" and mine[2:4] == b"\xff\xe0" and mine[6:11] == b"JFIF\0"
    J.assert_is_golden(name, mine)
    live = J.pil_encode(arr, Q)
    if J.tables(J.split(live)[0])[3] == J.RESTART:          # an older Pillow ignores restart_marker_blocks
        assert J.split(mine) == J.split(live)
        np.testing.assert_array_equal(J.pil_decode(mine), J.pil_decode(live))


@pytest.mark.parametrize("name", [n for n in J.cases() if n != J.FRAME])
def test_pil_decodes_the_file_to_the_pixels_of_its_own(files, name):
    arr, _ = J.cases()[name]
    got = J.pil_decode(files[name])
    assert got.shape == arr.shape
    np.testing.assert_array_equal(got, J.pil_decode(J.golden_file(name)))


def test_a_row_stride_is_honoured(files):
    arr, Q = J.cases()["noise_17x33_q90"]
    wide = np.full((17, 40, 3), 0x33, np.uint8)
    wide[:, :33] = arr
    assert encode_host(wide[:, :33], Q) == files["noise_17x33_q90"]               # ascontiguousarray: the plain layout
    lib = N.lib()
    bound = lib.mom_jpeg_bound(17, 33)
    out = np.empty(bound, np.uint8)
    size = C.c_uint32(0)
    assert lib.mom_jpeg_encode_host(17, 33, wide.ctypes.data, 120, Q, out.ctypes.data, bound, C.byref(size)) == N.MOM_OK
    assert out[:size.value].tobytes() == files["noise_17x33_q90"]


def test_the_cases_cover_the_coder_on_pils_own_streams():
    """Read from PIL's streams (the golden file) with the decoder of jpeg_cases.py: a condition on the case list, not on the encoder."""
    seen = dict(zrl=0, no_eob=0, dc11=0, ac10=0, stuffed=0, rst_wrap=0, dummy_right=0, dummy_below=0)
    for name, (arr, _) in J.cases().items():
        if name == J.FRAME:
            continue
        d = J.decode_scan(J.golden_file(name))
        H, W = d["size"]
        assert (H, W) == arr.shape[:2] and d["dri"] == J.RESTART
        mw = -(-W // 16)
        assert len(d["blocks"]) == 6 * mw * -(-H // 16)
        for k, (comp, cat, diff, syms, vals, eob) in enumerate(d["blocks"]):
            seen["zrl"] += 0xF0 in syms
            seen["no_eob"] += not eob
            seen["dc11"] += cat == 11
            seen["ac10"] += any(s & 15 == 10 for s in syms)
            m, b = divmod(k, 6)
            if b < 4:
                right = 2 * (m % mw) + (b & 1) >= -(-W // 8)
                below = 2 * (m // mw) + (b >> 1) >= -(-H // 8)
                if right or below:
                    assert (cat, diff, syms) == (0, 0, [0]), (name, k)            # the previous block's DC, no AC
                seen["dummy_right"] += right
                seen["dummy_below"] += below
        seen["stuffed"] += d["stuffed"]
        r = d["rst"]
        assert r == [i % 8 for i in range(len(r))]
        seen["rst_wrap"] += any(r[i] == 7 and r[i + 1] == 0 for i in range(len(r) - 1))
    print(seen)
    assert all(v > 0 for v in seen.values()), seen


def test_tables_are_annex_k_as_pil_writes_them():
    lib = N.lib()
    zz = None
    for Q in (1, 10, 49, 50, 51, 75, 90, 100):
        q, cnt, sym, n, r = (C.c_uint8 * 128)(), (C.c_uint8 * 64)(), (C.c_uint8 * 648)(), (C.c_int * 4)(), C.c_int(0)
        assert lib.mom_jpeg_tables(Q, q, cnt, sym, n, C.byref(r)) == N.MOM_OK
        assert r.value == J.RESTART
        quant, huff, _, _ = J.tables(J.split(J.pil_encode(np.zeros((8, 8, 3), np.uint8), Q))[0])
        if zz is None:
            sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
            import jpeg_tables
            zz = jpeg_tables.zigzag()
        for t in (0, 1):
            natural = [0] * 64
            for k in range(64):
                natural[zz[k]] = quant[t][k]
            assert list(q)[64 * t:64 * t + 64] == natural, (Q, t)
        for t, key in enumerate((0x00, 0x10, 0x01, 0x11)):
            counts, symbols = huff[key]
            assert list(cnt)[16 * t:16 * t + 16] == counts and n[t] == len(symbols)
            assert list(sym)[162 * t:162 * t + 162] == symbols + [0] * (162 - len(symbols))
    import jpeg_tables
    committed = os.path.join(os.path.dirname(jpeg_tables.OUT), "jpeg_tables.h")
    assert open(committed).read() == jpeg_tables.render(), "run tools/jpeg_tables.py"


# ---- the container and the writer -------------------------------------------------------------------------------------------
def _frames(H, W, n):
    import torch
    g = torch.Generator().manual_seed(3)
    y, x = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    out = []
    for k in range(n):
        s = torch.stack([0.5 + 0.6 * torch.sin(0.1 * x + 0.05 * y + k), 0.3 + 0.01 * x, 1.1 - 0.02 * y])
        out.append(s + 0.05 * torch.rand((3, H, W), generator=g))
    return out


def _to8b_window(img, y0, x0, H, W):
    a = (255 * np.clip(img.numpy(), 0, 1)).astype(np.uint8)
    return a[:, y0:y0 + H, x0:x0 + W].transpose(1, 2, 0)


def test_host_writer_writes_an_avi_of_pils_frames(tmp_path):
    R = importlib.import_module("iclr2025_3d-mom_amd.render")
    H, W, n = 21, 38, 5
    frames = _frames(H + 9, W + 6, n + 1)
    path = str(tmp_path / "v" / "a.avi")
    w = R.AsyncVideoWriter(path, H, W, fps=24, quality=80, encoder="host", slots=2, workers=2)
    for k in (3, 0, 1, 4, 2):                                   # any order: the file is in index order
        w.submit(frames[k], k, 5, 3)
    w.submit(frames[5], 1, 5, 3)                                # frame 1 again: replaced
    assert w.close() == path
    avi = J.parse_avi(open(path, "rb").read())
    assert avi["avih"]["total_frames"] == n and avi["avih"]["us_per_frame"] == 1000000 // 24
    assert avi["avih"]["flags"] == 0x10 and avi["avih"]["streams"] == 1
    assert (avi["avih"]["width"], avi["avih"]["height"]) == (W, H)
    sh, sf = avi["strh"], avi["strf"]
    assert (sh["type"], sh["handler"], sh["scale"], sh["rate"], sh["length"]) == (b"vids", b"MJPG", 1, 24, n)
    assert sh["frame"] == (0, 0, W, H)
    assert (sf["size"], sf["width"], sf["height"], sf["planes"], sf["bits"]) == (40, W, H, 1, 24)
    assert sf["compression"] == int.from_bytes(b"MJPG", "little") and sf["size_image"] == 3 * W * H
    assert len(avi["frames"]) == n
    for k, data in enumerate(avi["frames"]):
        src = frames[5] if k == 1 else frames[k]
        assert data == J.pil_encode(_to8b_window(src, 5, 3, H, W), 80), k
        assert J.pil_decode(data).shape == (H, W, 3)
    with pytest.raises(ValueError):
        R.AsyncVideoWriter(path, H, W, encoder="host").submit(frames[0], 0, 9, 7)        # the window leaves the image


def test_avi_chunks_are_padded_to_even_length():
    R = importlib.import_module("iclr2025_3d-mom_amd.render")
    frames = [b"\xff\xd8" + bytes(k) + b"\xff\xd9" for k in (1, 2, 3, 0)]
    data = R.avi_file(frames, 10, 12, fps=30)
    avi = J.parse_avi(data)
    assert avi["frames"] == frames and len(data) % 2 == 0
    assert J.parse_avi(R.avi_file([], 10, 12))["frames"] == []


def test_writer_arguments_and_environment(monkeypatch, tmp_path):
    R = importlib.import_module("iclr2025_3d-mom_amd.render")
    monkeypatch.delenv("MOM_VIDEO_ENCODER", raising=False)
    monkeypatch.delenv("MOM_VIDEO_QUALITY", raising=False)
    assert R.video_encoder() == "imageio"
    for e in ("imageio", "host", "device"):
        assert R.video_encoder(e) == e
    monkeypatch.setenv("MOM_VIDEO_ENCODER", "device")
    assert R.video_encoder() == "device" and R.video_encoder("host") == "host"
    monkeypatch.setenv("MOM_VIDEO_ENCODER", "")
    assert R.video_encoder() == "imageio"
    for bad in ("gpu", "Device", "1", "mjpeg"):
        monkeypatch.setenv("MOM_VIDEO_ENCODER", bad)
        with pytest.raises(ValueError):
            R.video_encoder()
    monkeypatch.delenv("MOM_VIDEO_ENCODER")
    with pytest.raises(ValueError):
        R.video_encoder("x264")
    with pytest.raises(ValueError):
        R.AsyncVideoWriter(str(tmp_path / "a.avi"), 8, 8, encoder="imageio")
    with pytest.raises(ValueError):
        R.AsyncVideoWriter(str(tmp_path / "a.avi"), 8, 8, encoder="host", quality=0)
    with pytest.raises(ValueError):
        R.AsyncVideoWriter(str(tmp_path / "a.avi"), 0, 8, encoder="host")
    w = R.AsyncVideoWriter(str(tmp_path / "a.avi"), 8, 8)
    assert w.encoder == "host" and w.quality == 90 and w.restart == J.RESTART
    w.close()
    monkeypatch.setenv("MOM_VIDEO_QUALITY", "55")
    w = R.AsyncVideoWriter(str(tmp_path / "b.avi"), 8, 8, encoder="host")
    assert w.quality == 55
    w.close()


def _cpu_render_set(R, monkeypatch, tmp_path, name, H, W, n=3):
    """render_set with a stand-in for the renderer that needs no GPU: frame k is a closed form."""
    import torch
    frames = _frames(H, W, n)
    views = [types.SimpleNamespace(k=k) for k in range(n)]
    monkeypatch.setattr(R, "render", lambda view, *a, **k: {"render": frames[view.k]})
    gaussians = types.SimpleNamespace(_xyz=torch.zeros((5, 3)))
    out = R.render_set(str(tmp_path / name), "side", 1, views, gaussians, None, None, None)
    return frames, out


def test_render_set_unset_is_as_before_and_host_writes_the_avi(monkeypatch, tmp_path, capsys):
    R = importlib.import_module("iclr2025_3d-mom_amd.render")
    monkeypatch.setitem(sys.modules, "imageio", None)           # not installed
    monkeypatch.delenv("MOM_VIDEO_ENCODER", raising=False)
    monkeypatch.delenv("MOM_VIDEO_QUALITY", raising=False)
    _cpu_render_set(R, monkeypatch, tmp_path, "unset", 70, 81)
    assert "imageio is not installed: skipping vid_result/side.mp4 (the PNG frames are complete)" in capsys.readouterr().out
    assert not os.path.exists(str(tmp_path / "unset" / "vid_result"))
    monkeypatch.setenv("MOM_VIDEO_ENCODER", "imageio")
    _cpu_render_set(R, monkeypatch, tmp_path, "named", 70, 81)
    assert "imageio is not installed: skipping vid_result/side.mp4" in capsys.readouterr().out

    monkeypatch.setenv("MOM_VIDEO_ENCODER", "host")
    frames, out = _cpu_render_set(R, monkeypatch, tmp_path, "host", 70, 81)
    assert "imageio" not in capsys.readouterr().out and out["frames"] == 3
    assert sorted(os.listdir(str(tmp_path / "host" / "frame_result" / "side"))) == ["00000.png", "00001.png", "00002.png"]
    avi = J.parse_avi(open(str(tmp_path / "host" / "vid_result" / "side.avi"), "rb").read())
    assert (avi["avih"]["width"], avi["avih"]["height"], avi["strh"]["rate"]) == (81 - 64, 70 - 64, 30)
    for k, data in enumerate(avi["frames"]):
        assert data == J.pil_encode(_to8b_window(frames[k], 32, 32, 6, 17), 90), k

    for H, W in ((64, 81), (70, 64), (40, 40)):                 # nothing is left of the frame after the crop
        with pytest.raises(ValueError, match="empty"):
            _cpu_render_set(R, monkeypatch, tmp_path, f"empty_{H}_{W}", H, W)
    monkeypatch.setenv("MOM_VIDEO_ENCODER", "x264")
    with pytest.raises(ValueError):
        _cpu_render_set(R, monkeypatch, tmp_path, "bad", 70, 81)
