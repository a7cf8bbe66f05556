"""Inputs shared by tests/test_hexplane_orders_cpu.py and tests/test_hexplane_orders_gpu.py: processing orders the two-pass
HexPlane backward must accept, the texel cells they walk through, and the oracle's answer for the clouds they are used on.

The module rebuilds its Morton order and its six plane orders every REORDER_EVERY calls only, so most training steps walk orders
that were sorted for other positions; "an order is a permutation whatever the keys were, and only speed depends on it".  The
scatter kernels recompute every cell from the current positions and detect runs of one cell along the order: under a sorted
order they see long runs and neighbouring cells, under any other order they see whatever `events` below counts.  The families:

  fresh        the library's own orders for the positions used (the control)
  stale        the library's orders for DISPLACED positions (`displaced`), used with the true ones
  random       independent random permutations for the Morton slot and each (plane, level) slot
  reversed     fresh, reversed
  adversarial  per (plane, level) from the emulated cells: the cell-sorted order with its halves interleaved, so consecutive
               positions alternate between distant cells, and border positions moved between two positions of one interior cell

`fresh` and `stale` need the library's sort: the caller passes `lib_orders`, a function positions -> (morton, order, inverse).  On
the CPU `emulated_lib_orders` stands in for it (a stable argsort of the emulated Morton key; tests/test_hexplane_orders_gpu.py
holds mom_hexplane_orders to exactly that).

A position is a BORDER position of a plane when a corner of its texel lies outside: the point is at or beyond the box MINIMUM
on one of the plane's axes (the aabb rows are flipped, row 0 is the maximum, so the minimum maps to the last texel).  A point
beyond the maximum clips to texel 0 and is an ordinary interior position."""
import functools
import importlib
from collections import namedtuple

import numpy as np
import torch

import hexplane_box_cases as hb

pkg = hb.pkg
BOX = "asym_a"
# "mid": few points per texel and short runs; "small" has thousands of points per texel at the large sizes and runs that span
# chunk boundaries
SHAPES = dict(hb.SHAPES, mid=((32, 24, 40, 12), (1, 2), 0.3))
CLOUD_SEED, ORDER_SEED, STALE_SEED = 5, 11, 17
PLANE_AXES = ((0, 1), (0, 2), (1, 2))          # order slot -> (ca, cb); slot 1 carries its time line on cb, the others on ca


def spec(shape):
    """(resolution, multires, timestamp) of a named shape, or the tuple itself."""
    return SHAPES[shape] if isinstance(shape, str) else shape


def field(channels, box, shape, seed=hb.FIELD_SEED):
    """hb.field, also for the shapes only this module has (given by name or as a tuple): the same construction and the same random
    stream, which tests/test_hexplane_orders_cpu.py pins by building "small" both ways."""
    if isinstance(shape, str) and shape in hb.SHAPES:
        return hb.field(channels, box, shape, seed)
    HexPlaneField = importlib.import_module(pkg + ".scene.hexplane").HexPlaneField
    res, multires, _ = spec(shape)
    torch.manual_seed(seed)
    cfg = {'grid_dimensions': 2, 'input_coordinate_dim': 4, 'output_coordinate_dim': channels, 'resolution': list(res)}
    f = HexPlaneField(1.6, cfg, list(multires))
    hi, lo, _ = hb.BOXES[box]
    f.set_aabb(list(hi), list(lo))
    with torch.no_grad():
        for g in f.grids:
            for p in g:
                p.add_(torch.randn_like(p) * 0.2)
    return f


def level_sizes(shape):
    """[[W of axis 0, 1, 2] per level]."""
    res, multires, _ = spec(shape)
    return [[res[k] * m for k in range(3)] for m in multires]


# ---------------------------------------------------------------------------------------- clouds
def cloud(P, box=BOX, seed=CLOUD_SEED):
    """[P, 3] fp32 on `box`; about 4 % of the points lie outside on some axis.  P = 300: hb.points(box), which has the face,
    corner and one-ulp points."""
    if P == hb.P:
        return hb.points(box)
    hi, lo, _ = hb.BOXES[box]
    hi, lo = np.asarray(hi, np.float32), np.asarray(lo, np.float32)
    g = torch.Generator().manual_seed(seed + 1000003 * (P % 9973))
    u = torch.rand(P, 3, generator=g).numpy()
    pts = (lo + (np.float32(0.02) + np.float32(0.96) * u) * (hi - lo)).astype(np.float32)
    out = torch.rand(P, generator=g).numpy() < 0.04
    axis = torch.randint(0, 3, (P,), generator=g).numpy()
    far = (torch.rand(P, generator=g).numpy() * 0.5 - 0.25).astype(np.float32)          # +-25 % of the extent beyond a face
    for k in range(3):
        m = out & (axis == k)
        pts[m, k] = np.where(far[m] < 0, lo[k] + far[m] * (hi[k] - lo[k]), hi[k] + far[m] * (hi[k] - lo[k])).astype(np.float32)
    return torch.from_numpy(pts)


def displaced(pts, shape, box=BOX, seed=STALE_SEED):
    """The positions a `stale` order was sorted for: every point moved by 0 to 3 finest-level cells per axis, either way, and 5 %
    of them teleported uniformly over 1.5 x the box."""
    hi, lo, _ = hb.BOXES[box]
    hi, lo = np.asarray(hi, np.float32), np.asarray(lo, np.float32)
    n = pts.shape[0]
    g = torch.Generator().manual_seed(seed)
    finest = np.asarray(level_sizes(shape)[-1], np.float32)
    cell = (hi - lo) / (finest - 1)
    step = (torch.rand(n, 3, generator=g).numpy() * 6 - 3).astype(np.float32) * cell
    q = pts.numpy() + step
    tele = torch.rand(n, generator=g).numpy() < 0.05
    w = torch.rand(n, 3, generator=g).numpy().astype(np.float32)
    mid, ext = (hi + lo) / 2, (hi - lo) * np.float32(1.5)
    q[tele] = (mid - ext / 2 + w * ext)[tele]
    return torch.from_numpy(q.astype(np.float32))


def one_cell_cloud(n=hb.P, box=BOX, shape="small"):
    """n distinct points inside ONE texel of every plane and level: a small cube around an interior point, well inside a cell of
    the finest level (and so of the coarser one, checked by the CPU test)."""
    hi, lo, _ = hb.BOXES[box]
    hi, lo = np.asarray(hi, np.float32), np.asarray(lo, np.float32)
    finest = np.asarray(level_sizes(shape)[-1], np.float32)
    # the centre of finest-level cell (2, 2, 2) counted from the maximum (coordinate c = -1 there)
    centre = hi - (np.float32(2.5) / (finest - 1)) * (hi - lo)
    u = torch.rand(n, 3, generator=torch.Generator().manual_seed(23)).numpy().astype(np.float32) - np.float32(0.5)
    return torch.from_numpy((centre + u * np.float32(0.2) * (hi - lo) / (finest - 1)).astype(np.float32))


def outside_cloud(n=hb.P, box=BOX):
    """n points beyond the box minimum on at least two axes each (all three for every third point), so every position of every
    plane is a border position; the remaining axis is anywhere, the far side of the maximum included (its ride row may be inside)."""
    hi, lo, _ = hb.BOXES[box]
    hi, lo = np.asarray(hi, np.float32), np.asarray(lo, np.float32)
    g = torch.Generator().manual_seed(29)
    u = torch.rand(n, 3, generator=g).numpy().astype(np.float32)
    pts = lo - (np.float32(0.01) + u) * (hi - lo)                     # beyond the minimum on every axis
    free = torch.randint(0, 3, (n,), generator=g).numpy()
    w = torch.rand(n, generator=g).numpy().astype(np.float32)
    for i in range(n):
        if i % 3:
            pts[i, free[i]] = lo[free[i]] + (np.float32(-0.2) + np.float32(1.4) * w[i]) * (hi[free[i]] - lo[free[i]])
    return torch.from_numpy(pts.astype(np.float32))


# ---------------------------------------------------------------------------------------- texel cells, in fp32 on the CPU
Cells = namedtuple("Cells", "x0 y0 W H interior cell row row_in")


def texel(x, a0, a1, size, ft=np.float32):
    """(floor of the clipped unnormalised coordinate, one more texel exists) along one axis: hb.coord_torch_form and
    hb.unnormalize on arrays, with ATen's clip to [0, size - 1].  ft = np.float64: the same on the fp32 inputs in float64."""
    x = np.asarray(x, np.float32).astype(ft)
    a0, a1 = ft(np.float32(a0)), ft(np.float32(a1))
    scale = ft(2.0) / ft(a1 - a0)
    c = ((x - a0) * scale).astype(ft) - ft(1.0)
    v = (((c + ft(1.0)) / ft(2.0)) * ft(size - 1)).astype(ft)
    v = np.where(v <= 0, ft(0), np.where(v >= ft(size - 1), ft(size - 1), v))
    x0 = np.floor(v).astype(np.int64)
    return x0, x0 + 1 < size


def cells(pts, shape, box=BOX, ft=np.float32):
    """{(order slot, level): Cells} of a cloud.  `cell` is y0 * W + x0, `interior` says that all four corners exist; `row` is the
    texel along the axis the slot's time line rides on, `row_in` that its upper neighbour exists."""
    hi, lo, _ = hb.BOXES[box]
    p = pts.numpy() if torch.is_tensor(pts) else np.asarray(pts, np.float32)
    sizes = level_sizes(shape)
    out = {}
    for si, (ca, cb) in enumerate(PLANE_AXES):
        for l, sz in enumerate(sizes):
            x0, hx = texel(p[:, ca], hi[ca], lo[ca], sz[ca], ft)          # aabb row 0 is the maximum
            y0, hy = texel(p[:, cb], hi[cb], lo[cb], sz[cb], ft)
            on_b = si == 1
            out[si, l] = Cells(x0, y0, sz[ca], sz[cb], hx & hy, y0 * sz[ca] + x0, y0 if on_b else x0, hy if on_b else hx)
    return out


def spread16(x):
    x = np.asarray(x, np.uint32) & np.uint32(0xFFFF)
    x = (x | (x << np.uint32(8))) & np.uint32(0x00FF00FF)
    x = (x | (x << np.uint32(4))) & np.uint32(0x0F0F0F0F)
    x = (x | (x << np.uint32(2))) & np.uint32(0x33333333)
    x = (x | (x << np.uint32(1))) & np.uint32(0x55555555)
    return x


def plane_key(c):
    """The sort key of plane_key_kernel: the 2-D Morton interleave of (x0, y0)."""
    return spread16(c.x0) | (spread16(c.y0) << np.uint32(1))


def key_bits(c):
    bits = 0
    while (1 << bits) < max(c.W, c.H):
        bits += 1
    return 2 * bits


def inverse_of(order):
    inv = np.empty_like(order)
    inv[order] = np.arange(order.shape[0], dtype=order.dtype)
    return inv


def emulated_lib_orders(pts, shape, box=BOX):
    """What the library's sorts return, restated on the CPU: (morton, order [3, L, P], inverse [3, L, P]), int32.  The plane
    orders are stable argsorts of `plane_key`; the Morton slot is a 3-D Morton order of the cloud in its own bounding box (any
    permutation would do there: nothing compares it with the library's)."""
    p = pts.numpy()
    n = p.shape[0]
    cs = cells(pts, shape, box)
    L = len(level_sizes(shape))
    order = np.empty((3, L, n), np.int32)
    for (si, l), c in cs.items():
        order[si, l] = np.argsort(plane_key(c), kind="stable").astype(np.int32)
    lo, hi = p.min(0), p.max(0)
    q = np.clip((p - lo) / np.where(hi > lo, hi - lo, 1) * 1023, 0, 1023).astype(np.uint64)
    code = np.zeros(n, np.uint64)
    for b in range(10):
        for k in range(3):
            code |= ((q[:, k] >> np.uint64(b)) & np.uint64(1)) << np.uint64(3 * b + k)
    morton = np.argsort(code, kind="stable").astype(np.int32)
    return morton, order, np.stack([np.stack([inverse_of(order[si, l]) for l in range(L)]) for si in range(3)])


# ---------------------------------------------------------------------------------------- the order families
FAMILIES = ("fresh", "stale", "random", "reversed", "adversarial")


def _adversarial_slot(c):
    n = c.cell.shape[0]
    srt = np.argsort(np.where(c.interior, c.cell, c.W * c.H + c.cell), kind="stable")
    border = [int(i) for i in srt if not c.interior[i]]
    # pairs of one interior cell, at most one per cell and one per border position
    pairs, cells_taken = [], set()
    inner = [int(i) for i in srt if c.interior[i]]
    for a, b in zip(inner, inner[1:]):
        if len(pairs) == len(border):
            break
        if c.cell[a] == c.cell[b] and int(c.cell[a]) not in cells_taken:
            cells_taken.add(int(c.cell[a]))
            pairs.append((a, b))
    used = {i for ab in pairs for i in ab} | set(border[:len(pairs)])
    rest = [int(i) for i in srt if int(i) not in used]
    h = (len(rest) + 1) // 2
    walk = [None] * len(rest)
    walk[0::2], walk[1::2] = rest[:h], rest[h:]
    # the triples (interior, border, the same interior cell) go in at evenly spaced places of the interleaved walk
    out, at = [], {(k * len(walk)) // max(len(pairs), 1): k for k in range(len(pairs))}
    for j in range(len(walk) + 1):
        if j in at:
            a, b = pairs[at[j]]
            out += [a, border[at[j]], b]
        if j < len(walk):
            out.append(walk[j])
    assert len(out) == n
    return np.asarray(out, np.int32)


def orders(family, pts, shape, lib_orders=None, box=BOX):
    """(morton [P], order [3, L, P], inverse [3, L, P]) of one family, int32 numpy, validated.  lib_orders(positions) returns the
    same triple from the library's sorts (or from `emulated_lib_orders` on the CPU); `fresh`, `stale` and `reversed` need it."""
    n = pts.shape[0]
    L = len(level_sizes(shape))
    if family == "fresh":
        morton, order, inv = lib_orders(pts)
    elif family == "stale":
        morton, order, inv = lib_orders(displaced(pts, shape, box))
    elif family == "reversed":
        morton, order, _ = lib_orders(pts)
        morton, order = morton[::-1].copy(), order[:, :, ::-1].copy()
        inv = None
    elif family == "random":
        g = torch.Generator().manual_seed(ORDER_SEED)
        morton = torch.randperm(n, generator=g).numpy().astype(np.int32)
        order = np.stack([np.stack([torch.randperm(n, generator=g).numpy().astype(np.int32) for _ in range(L)]) for _ in range(3)])
        inv = None
    elif family == "adversarial":
        cs = cells(pts, shape, box)
        h = (n + 1) // 2
        morton = np.empty(n, np.int32)
        morton[0::2], morton[1::2] = np.arange(h), np.arange(h, n)
        order = np.stack([np.stack([_adversarial_slot(cs[si, l]) for l in range(L)]) for si in range(3)])
        inv = None
    else:
        raise KeyError(family)
    morton, order = np.ascontiguousarray(morton, np.int32), np.ascontiguousarray(order, np.int32)
    if inv is None:
        inv = np.stack([np.stack([inverse_of(order[si, l]) for l in range(L)]) for si in range(3)])
    inv = np.ascontiguousarray(inv, np.int32)
    validate(morton, order, inv, n, L)
    return morton, order, inv


def is_permutation(a, n):
    a = np.asarray(a)
    return a.shape == (n,) and a.dtype == np.int32 and np.array_equal(np.sort(a), np.arange(n, dtype=np.int32))


def validate(morton, order, inv, n, L):
    """Nothing that is not a permutation of 0..n-1 with its matching inverse may reach a kernel: the kernels index with it."""
    assert is_permutation(morton, n), "Morton slot is not a permutation"
    assert order.shape == inv.shape == (3, L, n), (order.shape, inv.shape)
    for si in range(3):
        for l in range(L):
            assert is_permutation(order[si, l], n), ("order is not a permutation", si, l)
            assert inv[si, l].dtype == np.int32 and np.array_equal(inv[si, l][order[si, l]], np.arange(n, dtype=np.int32)), \
                ("inverse does not match its order", si, l)


# ---------------------------------------------------------------------------------------- what a walk meets
Events = namedtuple("Events", "cell_changes evictions sandwiches row_stays chunk_crossing_runs")


def events(order, c, chunk, walk=None):
    """What the scatter's run detection meets when it walks `order` over the cells `c` of one (plane, level) in chunks of `chunk`
    (32 for 32 channels, 16 for 16) -- counted on the whole order as one walk:
      cell_changes         positions whose cell differs from the predecessor's, or where either touches the border
      evictions            a pending row replaced by a DIFFERENT row of the same (x & 1, y & 1) parity, i.e. of the same slot
      sandwiches           interior, border, interior with the same interior cell on both sides
      row_stays            positions whose ride row equals the predecessor's (both with an upper neighbour) while the cell changes
      chunk_crossing_runs  multiples of `chunk` at which a run of one interior cell continues; with `walk` (the positions one walker
                           takes: per_half32 / per_group16), only those inside a walker's range, where the carry is the kernel's"""
    o = np.asarray(order, np.int64)
    n = o.shape[0]
    cell, inner, row, row_in = c.cell[o], c.interior[o], c.row[o], c.row_in[o]
    same = np.zeros(n, bool)
    same[1:] = (cell[1:] == cell[:-1]) & inner[1:] & inner[:-1]
    row_same = np.zeros(n, bool)
    row_same[1:] = (row[1:] == row[:-1]) & row_in[1:] & row_in[:-1]
    changes = int((~same[1:]).sum())
    sand = int((inner[:-2] & ~inner[1:-1] & inner[2:] & (cell[:-2] == cell[2:])).sum()) if n >= 3 else 0
    stays = int((row_same[1:] & ~same[1:]).sum())
    at = np.arange(chunk, n, chunk)
    if walk is not None:
        at = at[at % walk != 0]
    crossing = int(same[at].sum())
    # the four pending slots: the texel (x, y) goes to slot 2 (y & 1) + (x & 1); a corner outside the plane takes no slot
    x0, y0 = c.x0[o], c.y0[o]
    # (a position's four corners take four different slots, so it offers each slot one texel at most)
    offered = np.full((4, n), -1, np.int64)
    pos = np.arange(n)
    for dy in (0, 1):
        for dx in (0, 1):
            x, y = x0 + dx, y0 + dy
            ok = (x < c.W) & (y < c.H)
            offered[(2 * (y & 1) + (x & 1))[ok], pos[ok]] = (y * c.W + x)[ok]
    ev = 0
    for k in range(4):
        t = offered[k][offered[k] >= 0]
        ev += int((t[1:] != t[:-1]).sum())
    return Events(changes, ev, sand, stays, crossing)


# ---------------------------------------------------------------------------------------- walk lengths (the launchers' formulas)
def per_half32(P):
    """hexplane_backward_launch<32> (csrc/hexplane.hip): 512 workgroups x 8 half-waves, ranges rounded up to the 32-position chunk."""
    per = -(-P // (512 * 8))
    return -(-per // 32) * 32


def per_group16(P):
    """hexplane_backward_launch<16> (csrc/hexplane.hip): 512 workgroups x 16 groups, ranges rounded up to the 16-position chunk."""
    per = -(-P // (512 * 16))
    return -(-per // 16) * 16


GATHER_ONE_TRIP = 1536 * 4 * 32          # points the gathers take in one trip through their chunk loop


# ---------------------------------------------------------------------------------------- oracles
def freeze(ref):
    for a in (ref[0], ref[1], *[g for lv in ref[2] for g in lv]):
        a.setflags(write=False)
    return ref


def oracle_for(channels, shape, pts, dtype=torch.float32, box=BOX):
    """(features, d xyz, [[d plane]]) of oracle.torch_ref.hexplane_features on the CPU in `dtype`, loss = sum(features * w), for
    the seeded field and weights of (channels, shape) at the positions `pts`."""
    from oracle import torch_ref as tr
    f = field(channels, box, shape)
    w = hb.weights(f.feat_dim, n=pts.shape[0])
    if dtype == torch.float32:
        return hb.oracle_of(f, pts, spec(shape)[2], w)
    p = pts.to(dtype).requires_grad_(True)
    planes = [[q.detach().to(dtype).contiguous().requires_grad_(True) for q in g] for g in f.grids]
    feat = tr.hexplane_features(p, spec(shape)[2], f.aabb.detach().to(dtype), planes)
    (feat * w.to(dtype)).sum().backward()
    return feat.detach().numpy(), p.grad.numpy(), [[q.grad.numpy() for q in g] for g in planes]


@functools.lru_cache(maxsize=None)
def oracle32(channels, shape, P):
    """The reference's fp32 sequence (the project's yardstick) for cloud(P), computed once and shared; read-only."""
    if P == hb.P and shape in hb.SHAPES:
        return hb.oracle(channels, BOX, shape)
    return freeze(oracle_for(channels, shape, cloud(P)))


@functools.lru_cache(maxsize=None)
def oracle64(channels, shape, P):
    """The same function on float64 inputs: a reference for the PLANE GRADIENTS only (sums of many terms).  Not for d xyz or the
    features: a point within rounding of a texel boundary falls into the other cell (tests/test_hexplane_orders_cpu.py)."""
    return freeze(oracle_for(channels, shape, cloud(P), torch.float64))


# the (shape, P) of the multi-chunk cases, for both channel counts
LARGE = (("small", 131072), ("small", 131109), ("small", 270001), ("mid", 270001))


def plane_error_ratio(got, ref):
    """max over the elements of |got - ref| / (atol + rtol |ref|) with the suite's gradient tolerance: <= 1 passes."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float((np.abs(got - ref) / (hb.grad_atol(ref) + hb.GRAD_RTOL * np.abs(ref))).max())
