"""What tests/test_field_ordered_cpu.py and tests/test_field_ordered_gpu.py share: the documented order of the ordered field backward
(include/mom4d.h, "ordered HexPlane backward" and "ordered MLP weight gradients") restated in numpy, the descriptor of a field for
the host twin, and the scratch layouts as the header states them.  numpy and ctypes only; nothing here touches a GPU."""
import ctypes as C
import importlib

import numpy as np

import hexplane_box_cases as hb
import hexplane_order_cases as hoc

pkg = hb.pkg
N = importlib.import_module(pkg + "._native")

PLANES = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))        # (ca, cb) of plane p over (x, y, z, t): W = res[ca], H = res[cb]
BLOCK = 64
F32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def align_up(n, a=256):
    return (n + a - 1) // a * a


def level_res(shape):
    """[[res x, y, z, t] per level] of a shape (name or tuple) of hexplane_order_cases: the time axis is not scaled."""
    res, multires, _ = hoc.spec(shape)
    return [[res[0] * m, res[1] * m, res[2] * m, res[3]] for m in multires]


def field_res(f):
    """The same from a HexPlaneField's planes ([1, C, H, W] each)."""
    out = []
    for g in f.grids:
        r = [0, 0, 0, 0]
        for p, (a, b) in enumerate(PLANES):
            r[a], r[b] = g[p].shape[3], g[p].shape[2]
        out.append(r)
    return out


# ---------------------------------------------------------------------------------------- cells and corner weights, fp32 on the CPU
def axis_sample(x, a0, a1, size, is_time=False):
    """(ix clipped, x0) along one axis, every operation rounded to fp32: hb.coord_torch_form and hb.unnormalize on arrays with ATen's
    clip; the time axis takes the timestamp as the coordinate itself."""
    x = np.asarray(x, F32)
    if is_time:
        c = x
    else:
        a0, a1 = F32(a0), F32(a1)
        scale = F32(2.0) / F32(a1 - a0)
        c = ((x - a0) * scale).astype(F32) - F32(1.0)
    v = (((c + F32(1.0)) / F32(2.0)).astype(F32) * F32(size - 1)).astype(F32)
    v = np.where(v <= 0, F32(0), np.where(v >= F32(size - 1), F32(size - 1), v)).astype(F32)
    return v, np.floor(v).astype(np.int64)


def plane_samples(pts, time, box, res, p):
    """(cell key y0 W + x0 [P], corner weights [P, 4] = w00 w01 w10 w11, W, H) of plane p at one level."""
    hi, lo, _ = hb.BOXES[box] if isinstance(box, str) else box
    pts = np.asarray(pts, F32)
    ca, cb = PLANES[p]
    Wd, Hd = res[ca], res[cb]
    ix, x0 = axis_sample(pts[:, ca], hi[ca], lo[ca], Wd)
    if cb < 3:
        iy, y0 = axis_sample(pts[:, cb], hi[cb], lo[cb], Hd)
    else:
        iy, y0 = axis_sample(np.full(len(pts), time, F32), 0, 0, Hd, is_time=True)
    x1, y1 = (x0 + 1).astype(F32), (y0 + 1).astype(F32)
    fx0, fy0 = x0.astype(F32), y0.astype(F32)
    w = np.stack([(x1 - ix) * (y1 - iy), (ix - fx0) * (y1 - iy), (x1 - ix) * (iy - fy0), (ix - fx0) * (iy - fy0)], 1).astype(F32)
    return y0 * Wd + x0, w, Wd, Hd


def seq_sum(rows):
    """((+0.0 + r_0) + r_1) + ... over the first axis, in fp32."""
    acc = np.zeros(rows.shape[1:], F32)
    for r in rows:
        acc = (acc + r).astype(F32)
    return acc


def class_sum(e):
    """s_k of one class: the terms [n, C] cut into blocks of 64 from the first, block sums left to right, then those left to right."""
    blocks = [seq_sum(e[i:i + BLOCK]) for i in range(0, len(e), BLOCK)]
    return seq_sum(np.stack(blocks)) if blocks else np.zeros(e.shape[1:], F32)


def plane_grad_numpy(key, w, Wd, Hd, gv, grad_in):
    """The documented order for one plane: gv [P, C] in point order, grad_in [H, W, C]; returns (grad, stats)."""
    Cn = gv.shape[1]
    out = np.array(grad_in, F32, copy=True)
    members = {}
    for g, k in enumerate(key):                      # ascending g inside a cell
        members.setdefault(int(k), []).append(g)
    stats = dict(written=0, empty_class=0, border=0, lengths=set())
    for y in range(Hd):
        for x in range(Wd):
            s, lens = [], []
            for k in range(4):
                cx, cy = x - (k & 1), y - (k >> 1)
                gs = members.get(cy * Wd + cx, []) if cx >= 0 and cy >= 0 else []
                lens.append(len(gs))
                if gs:
                    e = (gv[gs] * w[gs, k][:, None]).astype(F32)          # one fp32 multiply per term
                    s.append(class_sum(e))
                else:
                    s.append(np.zeros(Cn, F32))
            if not any(lens):
                continue
            stats["written"] += 1
            stats["lengths"] |= {n for n in lens if n}
            stats["empty_class"] += 0 in lens
            stats["border"] += x == Wd - 1 or y == Hd - 1
            T = ((s[0] + s[1]).astype(F32) + (s[2] + s[3]).astype(F32)).astype(F32)
            out[y, x] = (out[y, x] + T).astype(F32)
    return out, stats


def hexplane_numpy(pts, time, box, res_levels, gv, grads_in, part, dxyz_in):
    """All planes and dxyz: gv [L, 6, P, C], grads_in [[H, W, C] x 6] x L, part [L, P, 3]; ([[grad]], dxyz, [[stats]])."""
    grads, stats = [], []
    for l, res in enumerate(res_levels):
        grads.append([])
        stats.append([])
        for p in range(6):
            key, w, Wd, Hd = plane_samples(pts, time, box, res, p)
            g, st = plane_grad_numpy(key, w, Wd, Hd, gv[l, p], grads_in[l][p])
            grads[l].append(g)
            stats[l].append(st)
    v = np.array(part[0], F32)
    for l in range(1, len(res_levels)):
        v = (v + part[l]).astype(F32)
    return grads, (np.asarray(dxyz_in, F32) + v).astype(F32), stats


# ---------------------------------------------------------------------------------------- the host twin
def host_desc(channels, box, res_levels, grads=None, planes=None):
    """MomHexPlane of a field by hand: aabb row 0 is the maximum; grads / planes [[array or pointer] x 6] x L (kept alive by the caller)."""
    hi, lo, _ = hb.BOXES[box] if isinstance(box, str) else box
    d = N.MomHexPlane()
    d.levels, d.channels = len(res_levels), channels
    for l, res in enumerate(res_levels):
        for k in range(4):
            d.res[l][k] = int(res[k])
        for p in range(6):
            for name, src in (("grads", grads), ("planes", planes)):
                if src is not None:
                    a = src[l][p]
                    getattr(d, name)[l][p] = a if isinstance(a, int) else a.ctypes.data
    for k in range(3):
        d.aabb[k], d.aabb[3 + k] = hi[k], lo[k]
    return d


def host_twin(channels, box, res_levels, pts, time, gv, grads_in, part, dxyz_in):
    """mom_hexplane_ordered_sum_host on copies of the incoming gradients; ([[grad]], dxyz)."""
    grads = [[np.array(g, F32, copy=True, order="C") for g in lv] for lv in grads_in]
    d = host_desc(channels, box, res_levels, grads)
    pts = np.ascontiguousarray(pts, F32)
    gv, part = np.ascontiguousarray(gv, F32), np.ascontiguousarray(part, F32)
    dxyz = np.array(dxyz_in, F32, copy=True, order="C")
    rc = N.lib().mom_hexplane_ordered_sum_host(C.byref(d), len(pts), pts.ctypes.data, float(time), gv.ctypes.data, part.ctypes.data,
                                               dxyz.ctypes.data)
    assert rc == N.MOM_OK, rc
    return grads, dxyz


def hex_scratch_views(scratch_u8, levels, channels, P):
    """(gv [L, 6, P, C], part [L, P, 3]) of a read-back scratch (numpy uint8 from its 256-byte aligned start), as the header lays it out."""
    n_gv = levels * 6 * P * channels * 4
    o_part = align_up(n_gv)
    gv = scratch_u8[:n_gv].view(F32).reshape(levels, 6, P, channels)
    part = scratch_u8[o_part:o_part + levels * P * 3 * 4].view(F32).reshape(levels, P, 3)
    return gv, part


# ---------------------------------------------------------------------------------------- the CPU test's synthetic cloud
SYN_SHAPE = ((8, 6, 10, 5), (1, 2, 4), 0.3)            # three levels: the dxyz order has three operands


def synthetic_cloud(box=hoc.BOX, shape=SYN_SHAPE):
    """Clusters of exactly 64, 65 and 129 points, each inside ONE cell of the finest (x, y) plane with no other point in it, 3 points
    in a cell of their own, the box's minimum corner and three points beyond the minimum (border positions: the aabb rows are flipped,
    a point beyond the minimum clips to the LAST texel)."""
    hi, lo, _ = hb.BOXES[box]
    hi, lo = np.asarray(hi, F32), np.asarray(lo, F32)
    finest = np.asarray(hoc.level_sizes(shape)[-1], F32)
    rng = np.random.default_rng(41)
    out = []
    for n, cell in ((64, (2, 2, 2)), (65, (6, 5, 4)), (129, (11, 9, 7)), (3, (15, 13, 20))):
        centre = hi - ((np.asarray(cell, F32) + F32(0.5)) / (finest - 1)) * (hi - lo)
        u = rng.random((n, 3)).astype(F32) - F32(0.5)
        out.append((centre + u * F32(0.2) * (hi - lo) / (finest - 1)).astype(F32))
    ext = hi - lo
    out.append(np.stack([lo, lo - F32(0.1) * ext, np.array([lo[0] - F32(0.2) * ext[0], 0.1, 0.2], F32), lo - F32(0.3) * ext]).astype(F32))
    return np.concatenate(out)


# ---------------------------------------------------------------------------------------- the MLP's records
MLP_THIN, MLP_LAYER, MLP_PARTS = 12 * 64 + 16, 64 * 64 + 64, 256


def mlp_scratch_views(scratch_f32, P):
    """(dx records [256, 784], dW records [4, 256, 4160]) of a read-back scratch viewed as float32, as the header lays it out."""
    o = (4 * P * 64 + 63) // 64 * 64
    dx = scratch_f32[o:o + MLP_PARTS * MLP_THIN].reshape(MLP_PARTS, MLP_THIN)
    o += MLP_PARTS * MLP_THIN
    dw = scratch_f32[o:o + 4 * MLP_PARTS * MLP_LAYER].reshape(4, MLP_PARTS, MLP_LAYER)
    return dx, dw


def mlp_reduce_numpy(dx, dw, P, n_in, names):
    """{gradient name: total} of the records in ascending workgroup index from +0.0 (the caller adds it onto what the buffer held)."""
    nblocks = min((P + 31) // 32, MLP_PARTS)
    thin = seq_sum(dx[:nblocks])
    out = {}
    for L in range(4):
        tot = seq_sum(dw[L])
        wname, bname = ("dW0", "db0") if L == 0 else ("dW1_%d" % (L - 1), "db1_%d" % (L - 1))
        cols = n_in if L == 0 else 64
        out[wname] = tot[:64 * cols].reshape(64, cols)
        out[bname] = tot[64 * 64:64 * 64 + 64]
    for k, nout in enumerate((3, 3, 4)):
        out["dW2_%d" % k] = thin[k * 256:k * 256 + nout * 64].reshape(nout, 64)
        out["db2_%d" % k] = thin[768 + 4 * k:768 + 4 * k + nout]
    return {n: out[n] for n in names}
