"""What tests/test_eulerian_ordered_cpu.py and tests/test_eulerian_ordered_gpu.py share: the motions the ordered splat is tried on, the
documented order (include/mom4d.h, "ordered splat of the video generator's warp") restated in numpy with every float32 add done
on its own, and the host twins through ctypes.  The geometry, the chains and the bounds are eulerian_warp_cases'.  numpy and ctypes
only; nothing here touches a GPU."""
import functools
import importlib

import numpy as np

import eulerian_warp_cases as ec

pkg = "iclr2025_3d-mom_amd"
N = importlib.import_module(pkg + "._native")
F32 = np.float32
BLOCK = 64
MAX_COORD = 2.0 ** 30
MOTIONS = ("zero", "constant", "integer", "converge", "leave", "random", "nonfinite")
N_FRAMES = 5
IDX = (0, 2, 4)                                        # first, mid, last: at the ends one half has Z = 0


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def motion(kind, S):
    """[2,S,S] float32 (x then y)."""
    y, x = np.meshgrid(np.arange(S, dtype=np.float64), np.arange(S, dtype=np.float64), indexing="ij")
    c = S // 2
    if kind == "zero":                                 # one entry per half in every cell, weights (1, 0, 0, 0)
        m = np.zeros((2, S, S))
    elif kind == "constant":
        m = np.stack([np.full((S, S), 0.25), np.full((S, S), 0.5)])
    elif kind == "integer":
        m = np.stack([np.full((S, S), 2.0), np.full((S, S), -1.0)])
    elif kind == "converge":                           # every chain of the future half steps to (c + 1/4, c + 1/4) and rests there
        m = np.stack([c + 0.25 - x, c + 0.25 - y])
        m[:, c, c] = 0.0
    elif kind == "leave":                              # outwards on all four sides: the chains near the border leave the canvas
        m = np.stack([0.6 * (x - c + 0.5), 0.6 * (y - c + 0.5)])
    elif kind in ("random", "nonfinite"):
        m = np.random.default_rng(S).uniform(-3.0, 3.0, (2, S, S))
        if kind == "nonfinite":
            for (py, px), v in {(1, 2): np.nan, (S // 2, S // 3): np.inf, (S - 2, 3): -np.inf, (S // 3, S - 1): np.nan}.items():
                m[(py + px) % 2, py, px] = v
    else:
        raise ValueError(kind)
    return m.astype(F32)


def features(C, S):
    return ec.features(C, S, seed=24)


# ------------------------------------------------------------------------------------------------ the documented order, in numpy
def ordered_sum(values, ox, oy, H, W):
    """values [n, K] float32 (what an entry's term is before the weight), targets ox, oy [n] float32, entries in ascending e.
    Returns (T [H, W, K] float32, any [H, W] bool, longest cell): every texel's four classes, blocks of 64, each add on its own."""
    f = lambda a: np.asarray(a).astype(F32)
    with np.errstate(invalid="ignore"):
        kept = (np.abs(ox) < MAX_COORD) & (np.abs(oy) < MAX_COORD)             # NaN: False
    x0 = np.where(kept, np.floor(np.where(kept, ox, 0)), 0).astype(np.int64)
    y0 = np.where(kept, np.floor(np.where(kept, oy, 0)), 0).astype(np.int64)
    kept &= (x0 >= -1) & (x0 <= W - 1) & (y0 >= -1) & (y0 <= H - 1)
    oxk, oyk = np.where(kept, ox, 0).astype(F32), np.where(kept, oy, 0).astype(F32)
    wx1, wx0 = f(f(x0 + 1) - oxk), f(oxk - f(x0))
    wy1, wy0 = f(f(y0 + 1) - oyk), f(oyk - f(y0))
    w = (f(wx1 * wy1), f(wx0 * wy1), f(wx1 * wy0), f(wx0 * wy0))               # nw ne sw se (softmax_splatting.py:32-35)
    terms = [f(values * wk[:, None]) for wk in w]                              # one fp32 multiply per term
    cells = {}
    for e in np.flatnonzero(kept):                                             # ascending e inside every cell
        cells.setdefault((int(y0[e]), int(x0[e])), []).append(e)
    K = values.shape[1]
    T, any_term = np.zeros((H, W, K), F32), np.zeros((H, W), bool)
    for y in range(H):
        for x in range(W):
            s = []
            for k in range(4):
                es = cells.get((y - (k >> 1), x - (k & 1)), ())
                any_term[y, x] |= len(es) > 0
                sk = np.zeros(K, F32)
                for j in range(0, len(es), BLOCK):
                    b = np.zeros(K, F32)
                    for e in es[j:j + BLOCK]:
                        b = b + terms[k][e]
                    sk = sk + b
                s.append(sk)
            T[y, x] = (s[0] + s[1]) + (s[2] + s[3])
    return T, any_term, max((len(v) for v in cells.values()), default=0)


def finite_for_chains(m):
    """The kernels end a chain at non-finite motion (displacement 0 from that step on; include/mom4d.h).  ec.euler indexes with what it
    integrated, so it is handed a value that sends such a chain out of bounds at the same step -- with either sign, for either half."""
    return np.where(np.isfinite(m), m, F32(1e30)).astype(F32)


def blend_targets(mot, S, idx, n_frames):
    """(ox, oy, src) of the blend's entries in ascending e: the future half, then the past half; chains from ec.euler."""
    cut, pad, P, _ = ec.geometry(S)
    index = np.arange(S * S).reshape(S, S)
    m = finite_for_chains(mot)
    if cut:
        m, index = m[:, cut:-cut, cut:-cut], index[cut:-cut, cut:-cut]
    mpad = np.pad(m, ((0, 0), (pad, pad), (pad, pad)), mode="reflect")
    src = np.pad(index, pad, mode="reflect").ravel()
    future, past = ec.euler(mpad, idx), ec.euler(-mpad, n_frames - idx - 1)
    yy, xx = np.meshgrid(np.arange(P), np.arange(P), indexing="ij")
    f = lambda a: np.asarray(a).astype(F32)
    ox = np.concatenate([f(f(xx) + future[0]).ravel(), f(f(xx + P) + f(past[0] - F32(P))).ravel()])
    oy = np.concatenate([f(f(yy) + future[1]).ravel(), f(f(yy) + past[1]).ravel()])
    return ox, oy, np.concatenate([src, src]), P


def blend_numpy(feature, mot, idx, n_frames):
    """acc [P,P,C+1] of the ordered blend in the documented order, and the longest cell."""
    C, S, _ = feature.shape
    ox, oy, src, P = blend_targets(mot, S, idx, n_frames)
    alpha = idx / (n_frames - 1)
    z = np.concatenate([np.full(P * P, F32(1 - alpha)), np.full(P * P, F32(alpha))]).astype(F32)
    vals = np.concatenate([feature.reshape(C, -1)[:, src].T, np.ones((2 * P * P, 1), F32)], 1).astype(F32)
    vals = (vals * z[:, None]).astype(F32)                                       # (feature Z) and (1 Z)
    T, _, longest = ordered_sum(vals, ox, oy, P, P)
    return T, longest


def splat_numpy(inp, flw, out_in):
    """out_in + T per image, a texel without a term left as it is."""
    n, C, H, W = inp.shape
    out = out_in.copy()
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    for i in range(n):
        ox = (xx.astype(F32) + flw[i, 0]).astype(F32).ravel()
        oy = (yy.astype(F32) + flw[i, 1]).astype(F32).ravel()
        T, any_term, _ = ordered_sum(np.ascontiguousarray(inp[i].reshape(C, -1).T), ox, oy, H, W)
        with np.errstate(invalid="ignore", over="ignore"):
            out[i] = np.where(any_term[None], (out_in[i] + T.transpose(2, 0, 1)).astype(F32), out_in[i])
    return out


def splat_reached(flw, H, W):
    """[N,H,W] bool: the texels that have a term (of any weight, zero included) in some class."""
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    one = np.ones((H * W, 1), F32)
    return np.stack([ordered_sum(one, (xx.astype(F32) + f[0]).astype(F32).ravel(), (yy.astype(F32) + f[1]).astype(F32).ravel(), H, W)[1]
                     for f in flw])


# ------------------------------------------------------------------------------------------------ the host twins
def blend_host(feature, mot, idx, n_frames):
    C, S, _ = feature.shape
    P = ec.geometry(S)[2]
    feature, mot = np.ascontiguousarray(feature, F32), np.ascontiguousarray(mot, F32)
    acc = np.full((P, P, C + 1), np.nan, F32)
    rc = N.lib().mom_eulerian_blend_ordered_host(C, S, S, idx, n_frames, feature.ctypes.data, mot.ctypes.data, acc.ctypes.data)
    assert rc == N.MOM_OK, rc
    return acc


def splat_host(inp, flw, out_in):
    n, C, H, W = inp.shape
    inp, flw, out = np.ascontiguousarray(inp, F32), np.ascontiguousarray(flw, F32), np.ascontiguousarray(out_in, F32).copy()
    rc = N.lib().mom_softsplat_sum_ordered_host(n, C, H, W, inp.ctypes.data, flw.ctypes.data, out.ctypes.data)
    assert rc == N.MOM_OK, rc
    return out


@functools.lru_cache(maxsize=None)
def blend_case(kind, S, C, idx):
    """(feature, motion, the host twin's acc) of one case, computed once per process; not to be written to."""
    f, m = features(C, S), motion(kind, S)
    acc = blend_host(f, m, idx, N_FRAMES)
    for a in (f, m, acc):
        a.setflags(write=False)
    return f, m, acc


def splat_inputs(n, C, H, W):
    """input, flow and a non-zero output to add onto.  The flow leaves the canvas on all four sides; image 0 also has targets on the
    cell row and column -1, exactly on the last row, non-finite and huge ones (dropped), and a texel nothing reaches that holds -0.0."""
    rng = np.random.default_rng(1000 * n + 100 * C + H)
    inp = rng.standard_normal((n, C, H, W)).astype(F32)
    flw = rng.uniform(-2.5, 2.5, (n, 2, H, W)).astype(F32)
    out = rng.standard_normal((n, C, H, W)).astype(F32)
    flw[0, :, 0, 0] = (-0.5, -0.25)                    # cell (-1, -1): only its se corner is a texel
    flw[0, :, H - 1, W - 1] = (0.0, 0.0)               # cell (H-1, W-1): only its nw corner
    flw[0, 0, 1, 1], flw[0, 1, 2, 2], flw[0, 0, 3, 3], flw[0, 1, 4, 4] = np.nan, np.inf, 3e30, -2.0 ** 31
    return inp, flw, out
