"""Inputs, a float64 restatement and derived bounds for the fused deformation MLP (csrc/deform_mlp.hip, csrc/deform_bwd_b3.hip and
the MLP half of csrc/deform_field.hip / deform_field16.hip): shared by tests/test_deform_mlp_ref_cpu.py and _gpu.py.  numpy only.

What is restated (reference scene/deformation.py:53-65,97-153 as include/mom4d.h states it), parameters W0 b0 and, per head k in
{pos, scales, rotations}, W1_k b1_k W2_k b2_k (nn.Linear layout [out,in]; in_features 64 or 32, heads 3 / 3 / 4):
    z0 = W0 f + b0,  a0 = relu(z0),  z1_k = W1_k a0 + b1_k,  a1_k = relu(z1_k),  o_k = W2_k a1_k + b2_k
    pts = xyz + (o_pos + c flow),  scales = s + o_scales,  rots = r + o_rot
and, for upstream gradients d_k of the three outputs,
    dW2_k = d_k^T a1_k, db2_k = sum_g d_k,  dH1_k = [z1_k > 0] (d_k W2_k),  dW1_k = dH1_k^T a0, db1_k = sum_g dH1_k,
    dH0 = [a0 > 0] sum_k dH1_k W1_k,  dW0 = dH0^T f, db0 = sum_g dH0,  dfeat = dH0 W0            (relu'(0) = 0, as torch).
The backward takes a0 as an INPUT, as the kernels do (mom_deform_backward*): the GPU tests hand them fp32(reference a0), one known
rounding, so that the backward is tested on its own; `e_a0` carries an inherited error of that input for the composed
(forward + backward through ops.deform_mlp) cases.

Bounds.  eps = 2^-24, gamma(n, u) = n u / (1 - n u).  Every bound is a second float64 pass over absolute values; none of the
constants below was chosen by looking at what a kernel returns.

 (1) fp32 dot product of n terms plus a bias, in any order, fused or not: each term passes through at most n + 1 roundings, so
     |fl(w.x + b) - (w.x + b)| <= gamma(n + 1) S with S = sum |w||x| + |b|   [Higham, Accuracy and Stability, (3.5)].
 (2) The bf16 forms (deform_b3_dev.h: split_pair by masks, mfma6).  An operand is cut into three pieces by TRUNCATION to eight
     significant bits: x = x1 + x2 + x3 exactly, |x2| < 2^-7 |x|, |x3| < 2^-14 |x|.  Six of the nine piece products are kept;
     the dropped x2 y3 + x3 y2 + x3 y3 is below KAPPA |x||y|, KAPPA = 2^-21 + 2^-21 + 2^-28.  (The sources' comments say "2^-23":
     that is the figure for a split by rounding; with masks the pieces are one bit larger each.)  Every kept piece product is
     exact in fp32 (8 x 8 bits), so what remains is an fp32 sum of 6 n + 1 terms whose absolute values add up to at most
     PIECES S, PIECES = (1 + 2^-7 + 2^-14)^2.  The matrix instruction's internal additions are not documented to round to
     nearest: unit roundoff U_BF = 2^-23 covers truncation as well.  Bound: gamma(6 n + 1, U_BF) PIECES S + KAPPA S.
 (3) Inherited error propagates linearly, |W| e, and the magnitudes a later rounding acts on are those of the COMPUTED operand,
     |x| + e.  ReLU is 1-Lipschitz: e(a) = e(z) -- and 0 where z < -e(z), since then the computed value is 0 as well.
 (4) Residual adds: c flow one rounding, (o + c flow) one, xyz + (.) one; each bounded by eps times the sum of the absolute
     values (and errors) it adds, which covers a fused multiply-add too.
 (5) relu'.  Where |z| > e(z) the computed sign is the exact one and dH inherits only the rounding of the value that passes.
     Where it is not (an AMBIGUOUS unit), the bound is the whole magnitude |v| + e: such rows are not excluded, they are simply
     not there -- see the builder.
 (6) Sums over Gaussians (dW*, db*), in any order, with float atomics or not: a term that is exactly zero adds exactly, so with
     n the number of Gaussians whose upstream gradient row is not zero, gamma(n) S for fp32 (product + at most n - 1 additions)
     and form (2) with 6 n terms for the bf16 weight gradients, S the sum of |dH||x| over computed magnitudes, plus the operand
     terms  sum e(dH) (|x| + e(x)) + sum |dH| e(x).  dH1 = d W2 is a four-term fp32 dot product: gamma(4).  The three heads'
     dA0 meet in one fp32 chain (split form) or in two more additions (b3): one sum of 3 x 64 (x 6) + 2 terms.
 (7) += into a prefilled buffer: one more rounding, eps (|prefill| + |gradient| + e).

Membership at large P.  With dense upstream gradients the order-independent bound (6) grows like n eps sum |terms|: at 8 k
Gaussians it is wider than one Gaussian's contribution, so a dropped, duplicated or misattributed Gaussian would pass it.  The
NEEDLE cases guard that: d_k is zero except at a handful of Gaussians (0 and P - 1, the last of a dW range and the first of the
next, both sides of a 32-tile edge, tile 32 + {7, 8, 15, 16}: the b3 K-step halves).  n is then that handful whatever P is, the
bound is a few eps of each outer product, and a Gaussian lost or counted twice is an error of 100 %.

Inputs with no ambiguous ReLU.  Rows are drawn from a seeded generator; all 256 pre-activations of a Gaussian are evaluated in
float64 (z1 from fp32(a0), the array the backward receives) and a row is redrawn -- its feature VALUES only, never an index, and
a wide-range row keeps its scale -- while any |z| is below MARGIN = 16 times that pre-activation's bound (and twice the composed
bound that includes a0's own error, for the cases that run forward and backward together).  Rounds are bounded and the builder
asserts that no ambiguous row is left: backward comparisons then exclude ZERO rows, which is a condition on the inputs and not a
measurement.  Forward comparisons need none of this: every output is continuous across a flip.

Structural units are exempt from the margin rule and asserted exactly (STRUCT): an exactly-zero unit in the trunk and in head 0
(zero weight row, zero bias: z is 0 in any order; a0 / a1 column 0, its dW row and db entry exactly 0, the downstream weight
column's gradient exactly 0: relu'(0) = 0), an always-dead unit in the trunk and in head 1 (bias -1e3: the same exact zeros) and an
always-live unit in head 2 (bias +1e3; its W2 column is scaled by 1e-3 so that the head's output keeps its size)."""
import functools

import numpy as np

EPS = 2.0 ** -24
U_BF = 2.0 ** -23
KAPPA = 2.0 ** -21 + 2.0 ** -21 + 2.0 ** -28
PIECES = (1.0 + 2.0 ** -7 + 2.0 ** -14) ** 2
MARGIN = 16.0
FLOW_COEF = float(np.float32(0.7))
NOUT = (3, 3, 4)
HID = 64
# (layer, unit): layer 0 = trunk, 1 + k = head k
STRUCT = {"zero": ((0, 5), (1, 11)), "dead": ((0, 37), (2, 50)), "live": ((3, 23),)}
OUT_NAMES = ("pts", "scales", "rots", "a0")
GRAD_NAMES = ("dW0", "db0") + tuple(n + str(k) for k in range(3) for n in ("dW1_", "db1_", "dW2_", "db2_"))


def gamma(n, u=EPS):
    return n * u / (1.0 - n * u)


def dot_bound(S, n, bf16):
    """(1) / (2): S = sum |w||x| + |b| over computed magnitudes, n terms."""
    return (gamma(6 * n + 1, U_BF) * PIECES + KAPPA) * S if bf16 else gamma(n + 1) * S


def sum_bound(S, n, bf16):
    """(6): a sum of n products over the Gaussians."""
    return (gamma(6 * n, U_BF) * PIECES + KAPPA) * S if bf16 else gamma(n) * S


def _f64(params):
    return [np.asarray(p, np.float64) for p in params]


BLOCK = 4096          # rows per pass: the temporaries of a pass stay in the cache, and the cost is linear in P


def _blocks(P):
    return [slice(i, min(P, i + BLOCK)) for i in range(0, P, BLOCK)]


def _forward_rows(p, f, xyz, scal, rot, flow, bf16, a0_in):
    n_in = f.shape[1]
    W0, b0 = p[0], p[1]
    z0 = f @ W0.T + b0
    e_z0 = dot_bound(np.abs(f) @ np.abs(W0).T + np.abs(b0), n_in, bf16)
    if a0_in is None:
        a0, e_a0 = np.maximum(z0, 0.0), np.where(z0 < -e_z0, 0.0, e_z0)
    else:
        a0, e_a0 = np.asarray(a0_in, np.float64), np.zeros_like(z0)
    v, e = {"z0": z0, "a0": a0}, {"z0": e_z0, "a0": e_a0}
    for k in range(3):
        W1, b1, W2, b2 = p[2 + 4 * k:6 + 4 * k]
        z1 = a0 @ W1.T + b1
        e_z1 = e_a0 @ np.abs(W1).T + dot_bound((a0 + e_a0) @ np.abs(W1).T + np.abs(b1), HID, bf16)
        a1, e_a1 = np.maximum(z1, 0.0), np.where(z1 < -e_z1, 0.0, e_z1)
        o = a1 @ W2.T + b2
        S_o = (a1 + e_a1) @ np.abs(W2).T + np.abs(b2)
        e_o = e_a1 @ np.abs(W2).T + gamma(HID + 1) * S_o
        v["z1_%d" % k], e["z1_%d" % k] = z1, e_z1
        base = np.asarray((xyz, scal, rot)[k], np.float64)
        if k == 0:
            cf = FLOW_COEF * np.asarray(flow, np.float64)
            e1 = EPS * np.abs(cf)
            e2 = e_o + e1 + EPS * (S_o + e_o + np.abs(cf) + e1)
            v["pts"] = base + (o + cf)
            e["pts"] = e2 + EPS * (np.abs(base) + S_o + np.abs(cf) + e2)
        else:
            v[OUT_NAMES[k]] = base + o
            e[OUT_NAMES[k]] = e_o + EPS * (np.abs(base) + S_o + e_o)
    return v, e


def forward(params, feat, xyz, scal, rot, flow, bf16=False, a0_in=None, keep=OUT_NAMES):
    """The forward in float64 and its bounds, two dicts with the keys "pts", "scales", "rots", "a0" (and, on request through
    `keep`, the pre-activations "z0", "z1_0", "z1_1", "z1_2").
    bf16: the 64 x 64 layers (and the trunk) in form (2) -- deform_field.hip; the thin output layers are fp32 in every kernel.
    a0_in: evaluate the heads on this a0 (taken as exact) instead of relu(z0)."""
    p = _f64(params)
    f = np.asarray(feat, np.float64)
    vs, es = [], []
    for b in _blocks(len(f)):
        v, e = _forward_rows(p, f[b], xyz[b], scal[b], rot[b], flow[b], bf16, None if a0_in is None else a0_in[b])
        vs.append({k: v[k] for k in keep})
        es.append({k: e[k] for k in keep})
    return ({k: np.concatenate([v[k] for v in vs]) for k in keep}, {k: np.concatenate([e[k] for e in es]) for k in keep})


def _backward_rows(p, f, a0, douts, bf16, e0, acc):
    """One block of rows: returns (dfeat, its bound) and adds the block's share of every sum over Gaussians to acc[name] =
    [value, S (the sum of computed magnitudes the rounding bound multiplies), operand terms]; acc["n"]: the rows counted."""
    W0 = p[0]
    dA0, e_in, S_dA0 = 0.0, 0.0, 0.0

    def add(name, val, S, extra=0.0):
        t = acc.setdefault(name, [0.0, 0.0, 0.0])
        t[0], t[1], t[2] = t[0] + val, t[1] + S, t[2] + extra
    for k in range(3):
        W1, b1, W2, b2 = p[2 + 4 * k:6 + 4 * k]
        d = douts[k]
        z1 = a0 @ W1.T + b1
        e_z1 = e0 @ np.abs(W1).T + dot_bound((a0 + e0) @ np.abs(W1).T + np.abs(b1), HID, bf16)
        a1, e_a1 = np.maximum(z1, 0.0), np.where(z1 < -e_z1, 0.0, e_z1)
        acc["n"]["n2_%d" % k] += int(np.any(d != 0, axis=1).sum())
        add("db2_%d" % k, d.sum(0), np.abs(d).sum(0))
        add("dW2_%d" % k, d.T @ a1, np.abs(d).T @ (a1 + e_a1), np.abs(d).T @ e_a1)
        G, e_G = d @ W2, gamma(4) * (np.abs(d) @ np.abs(W2))
        dH1 = np.where(z1 > 0, G, 0.0)
        e_dH1 = np.where(np.abs(z1) <= e_z1, np.abs(G) + e_G, np.where(z1 > 0, e_G, 0.0))
        cH = np.abs(dH1) + e_dH1                                         # computed magnitude
        acc["n"]["n1_%d" % k] += int(np.any(cH != 0, axis=1).sum())
        add("dW1_%d" % k, dH1.T @ a0, cH.T @ (a0 + e0), e_dH1.T @ (a0 + e0) + np.abs(dH1).T @ e0)
        add("db1_%d" % k, dH1.sum(0), cH.sum(0), e_dH1.sum(0))
        dA0 = dA0 + dH1 @ W1
        e_in = e_in + e_dH1 @ np.abs(W1)
        S_dA0 = S_dA0 + cH @ np.abs(W1)
    e_dA0 = e_in + ((gamma(6 * 3 * HID + 3, U_BF) * PIECES + KAPPA) if bf16 else gamma(3 * HID + 2)) * S_dA0
    dH0 = np.where(a0 > 0, dA0, 0.0)
    e_dH0 = np.where(a0 <= e0, np.where(e0 > 0, np.abs(dA0) + e_dA0, 0.0), e_dA0)
    cH = np.abs(dH0) + e_dH0
    acc["n"]["n0"] += int(np.any(cH != 0, axis=1).sum())
    add("dW0", dH0.T @ f, cH.T @ np.abs(f), e_dH0.T @ np.abs(f))
    add("db0", dH0.sum(0), cH.sum(0), e_dH0.sum(0))
    return dH0 @ W0, e_dH0 @ np.abs(W0) + dot_bound(cH @ np.abs(W0), HID, bf16)


def backward(params, feat, a0, douts, bf16=False, e_a0=None):
    """The backward in float64 from a0 as the kernels receive it, and its bounds: {"dfeat"} + GRAD_NAMES in both dicts.
    bf16: the b3 form (z1 recomputed, dA0, dfeat, dW0 and dW1 in form (2); dW2, db*, dH1 in fp32).
    Only the Gaussians with a non-zero upstream gradient row are evaluated: every term of the others is exactly zero."""
    p = _f64(params)
    P, n_in = np.shape(feat)
    live = np.flatnonzero(np.any([np.any(np.asarray(d) != 0, axis=1) for d in douts], axis=0))
    f, a0l = np.asarray(feat, np.float64)[live], np.asarray(a0, np.float64)[live]
    e0 = np.zeros_like(a0l) if e_a0 is None else np.asarray(e_a0, np.float64)[live]
    dl = [np.asarray(d, np.float64)[live] for d in douts]
    acc = {"n": dict.fromkeys(["n0"] + ["n%d_%d" % (j, k) for j in (1, 2) for k in range(3)], 0)}
    v, e = {"dfeat": np.zeros((P, n_in))}, {"dfeat": np.zeros((P, n_in))}
    for b in _blocks(len(live)):
        v["dfeat"][live[b]], e["dfeat"][live[b]] = _backward_rows(p, f[b], a0l[b], [d[b] for d in dl], bf16, e0[b], acc)
    n = acc.pop("n")
    shapes = dict(dW0=(HID, n_in), db0=(HID,))
    for k in range(3):
        shapes.update({"dW1_%d" % k: (HID, HID), "db1_%d" % k: (HID,), "dW2_%d" % k: (NOUT[k], HID), "db2_%d" % k: (NOUT[k],)})
    for name in GRAD_NAMES:
        val, S, extra = acc.get(name, (0.0, 0.0, 0.0))
        cnt = n["n0"] if name in ("dW0", "db0") else n["n%s_%s" % (name[2], name[-1])]
        rounding = sum_bound(S, cnt, bf16) if name[:3] in ("dW0", "dW1") else gamma(cnt) * S
        v[name] = np.zeros(shapes[name]) + val
        e[name] = np.zeros(shapes[name]) + rounding + extra
    return v, e


def _exempt():
    m = np.zeros((4, HID), bool)
    for units in STRUCT.values():
        for layer, unit in units:
            m[layer, unit] = True
    return m


def ambiguous_rows(params, feat, bf16, margin=1.0, composed=0.0, exempt=None):
    """Rows with a pre-activation the float64 evaluation cannot sign for an fp32 (bf16: form (2)) evaluation: some |z0| below
    margin x its bound, or some |z1| (from fp32(a0), the array the backward receives) below margin x its own bound or below
    composed x the bound that includes a0's error.  margin = 1, composed = 1: the rows on which two such evaluations of forward +
    backward may take different ReLU branches.  exempt [4,64]: units left out (the structural ones)."""
    p = _f64(params)
    f = np.asarray(feat, np.float64)
    ex = np.zeros((4, HID), bool) if exempt is None else exempt
    W0, b0 = p[0], p[1]
    W1 = np.concatenate([p[2 + 4 * k] for k in range(3)])                # [192,64]: the three heads at once
    b1 = np.concatenate([p[3 + 4 * k] for k in range(3)])
    ex1 = ex[1:].reshape(-1)
    bad = np.zeros(len(f), bool)
    for b in _blocks(len(f)):
        z0 = f[b] @ W0.T + b0
        e_z0 = dot_bound(np.abs(f[b]) @ np.abs(W0).T + np.abs(b0), f.shape[1], bf16)
        bad[b] = ((np.abs(z0) < margin * e_z0) & ~ex[0]).any(1)
        a0 = np.maximum(z0, 0.0).astype(np.float32).astype(np.float64)
        z1 = a0 @ W1.T + b1
        thr = margin * dot_bound(a0 @ np.abs(W1).T + np.abs(b1), HID, bf16)
        if composed:
            e_a0 = np.where(z0 < -e_z0, 0.0, e_z0)
            thr = np.maximum(thr, composed * (e_a0 @ np.abs(W1).T + dot_bound((a0 + e_a0) @ np.abs(W1).T + np.abs(b1), HID, bf16)))
        bad[b] |= ((np.abs(z1) < thr) & ~ex1).any(1)
    return bad


def dw_chunk(P):
    """The f32 dW kernels' range of Gaussians per wave (deform_mlp.hip backward(): 1024 waves, even ranges)."""
    c = (P + 1023) // 1024
    return c + (c & 1)


def needle_rows(P):
    """The handful of Gaussians of a needle case (module docstring), sorted, inside [0, P)."""
    c, tiles = dw_chunk(P), (P + 31) // 32
    rows = {0, P - 1, 31, 32}
    r = max(1, (P // c) // 2)                       # a range boundary in the middle, and the last one
    last = ((P - 1) // c) * c
    rows |= {r * c - 1, r * c, last - 1, last}
    t = tiles // 2                                  # a tile in the middle: its edges and the b3 K-step halves
    rows |= {32 * t - 1, 32 * t, 32 * t + 7, 32 * t + 8, 32 * t + 15, 32 * t + 16}
    t = tiles - 1                                   # the last tile
    rows |= {32 * t - 1, 32 * t, 32 * t + 7, 32 * t + 8, 32 * t + 15, 32 * t + 16}
    return np.array(sorted(x for x in rows if 0 <= x < P), np.int64)


def _weights(rng, n_in):
    mk = lambda *s: (rng.standard_normal(s) * 0.3).astype(np.float32)
    params = [mk(HID, n_in), mk(HID)]
    for nout in NOUT:
        params += [mk(HID, HID), mk(HID), mk(nout, HID), mk(nout)]
    W = lambda layer: params[0] if layer == 0 else params[2 + 4 * (layer - 1)]
    b = lambda layer: params[1] if layer == 0 else params[3 + 4 * (layer - 1)]
    for layer, unit in STRUCT["zero"]:
        W(layer)[unit] = 0
        b(layer)[unit] = 0
    for layer, unit in STRUCT["dead"]:
        b(layer)[unit] = -1e3
    for layer, unit in STRUCT["live"]:
        b(layer)[unit] = 1e3
        params[4 + 4 * (layer - 1)][:, unit] *= np.float32(1e-3)
    return params


ROUNDS = 64


@functools.lru_cache(maxsize=None)
def case(P, n_in, kind="dense", redraw=True):
    """One input set (read-only: it is shared): kind "dense", "needle" (upstream gradients zero except at needle_rows(P)) or
    "wide" (feature rows scaled by 10^U(-3, 1), a few rows all zero).  redraw=False: forward-only use, no margin.
    Keys: params (14 fp32 arrays), feat, xyz, scal, rot, flow, douts (3), P, n_in, bf16, redrawn (share of rows redrawn),
    ambiguous (rows left below the margin: 0, asserted), and the float64 forward `fwd` = (values, bounds) in the width's widest
    form."""
    bf16 = n_in == 64                   # the bf16 forms exist at 64 features only; their bound is the wider one
    rng = np.random.default_rng([P, n_in, ("dense", "needle", "wide").index(kind)])
    exempt = _exempt()
    params = _weights(rng, n_in)
    if kind == "wide":                  # an all-zero feature row has z0 = b0 for every such row: a matter of the weights
        for _ in range(ROUNDS):
            if not ambiguous_rows(params, np.zeros((1, n_in), np.float32), bf16, MARGIN, 2.0, exempt)[0]:
                break
            params = _weights(rng, n_in)
    mk = lambda *s: (rng.standard_normal(s) * 0.3).astype(np.float32)
    scale = np.full((P, 1), 3.0, np.float32)
    if kind == "wide":
        scale = (3.0 * 10.0 ** rng.uniform(-3, 1, (P, 1))).astype(np.float32)
        scale[rng.choice(P, max(1, P // 50), replace=False)] = 0
    feat = mk(P, n_in) * scale
    xyz, scal, rot, flow = mk(P, 3), mk(P, 3), mk(P, 4), mk(P, 3)
    douts = [mk(P, n) for n in NOUT]
    if kind == "needle":
        keep = np.zeros((P, 1), np.float32)
        keep[needle_rows(P)] = 1
        douts = [d * keep for d in douts]
    touched = np.zeros(P, bool)
    left = 0
    if redraw:
        idx = np.arange(P)
        for _ in range(ROUNDS):
            bad = ambiguous_rows(params, feat[idx], bf16, MARGIN, 2.0, exempt)
            idx = idx[bad]
            if idx.size == 0:
                break
            touched[idx] = True
            feat[idx] = mk(idx.size, n_in) * scale[idx]
        left = int(idx.size)
        assert left == 0, ("ambiguous rows left after %d rounds" % ROUNDS, P, n_in, kind, left)
    c = dict(P=P, n_in=n_in, kind=kind, bf16=bf16, params=params, feat=feat, xyz=xyz, scal=scal, rot=rot, flow=flow, douts=douts,
             redrawn=float(touched.mean()), ambiguous=left)
    c["fwd"] = forward(params, feat, xyz, scal, rot, flow, bf16)
    for a in params + [feat, xyz, scal, rot, flow] + douts:
        a.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def forward_ref(P, n_in, kind, redraw, bf16):
    c = case(P, n_in, kind, redraw)
    if bf16 == c["bf16"]:
        return c["fwd"]
    return forward(c["params"], c["feat"], c["xyz"], c["scal"], c["rot"], c["flow"], bf16)


@functools.lru_cache(maxsize=None)
def backward_ref(P, n_in, kind, bf16):
    """(a0 as fp32, values, bounds) of the backward on fp32(reference a0)."""
    c = case(P, n_in, kind)
    a0 = c["fwd"][0]["a0"].astype(np.float32)
    return (a0,) + backward(c["params"], c["feat"], a0, c["douts"], bf16)


def share(got, want, bound):
    """Largest |got - want| / bound over the elements; an element whose bound is 0 must be met exactly (share inf if not)."""
    d = np.abs(np.asarray(got, np.float64) - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where(bound > 0, d / bound, np.where(d == 0, 0.0, np.inf))
    return float(s.max()) if s.size else 0.0


def struct_zero_checks(n_in):
    """(gradient name, index) pairs that must be exactly zero: rows / entries of the zero and dead units and the downstream weight
    columns that multiply their (exactly zero) activation."""
    out = []
    for layer, unit in STRUCT["zero"] + STRUCT["dead"]:
        if layer == 0:
            out += [("dW0", (unit,)), ("db0", (unit,))] + [("dW1_%d" % k, (slice(None), unit)) for k in range(3)]
        else:
            k = layer - 1
            out += [("dW1_%d" % k, (unit,)), ("db1_%d" % k, (unit,)), ("dW2_%d" % k, (slice(None), unit))]
    return out


def grads_as_list(v):
    """GRAD_NAMES order = the parameter order of ops.deform_mlp: W0 b0 then W1 b1 W2 b2 per head."""
    return [v[n] for n in GRAD_NAMES]


# The sizes of the GPU tests (tests/test_deform_mlp_ref_gpu.py has the table of what each one reaches) and their cases: the CPU
# test checks the builder's condition for every one of them.
SIZES_BACKWARD = (1, 2, 3, 31, 32, 33, 65, 2047, 2049, 8193, 16387, 65569)
SIZE_FORWARD_ONLY = 131105
WIDE_SIZES = (33, 2049)


def all_cases():
    """(P, n_in, kind, redraw) of every case the GPU tests run."""
    out = []
    for n_in in (64, 32):
        for P in SIZES_BACKWARD:
            out += [(P, n_in, "dense", True), (P, n_in, "needle", True)]
        out += [(P, n_in, "wide", True) for P in WIDE_SIZES]
        out.append((SIZE_FORWARD_ONLY, n_in, "dense", False))
    return out
