"""Yardstick and inputs of the scene-flow fit's tests (test_sceneflow_cpu.py, test_sceneflow_gpu.py).

`restate` is the reference's loop (train_motion.py:125-207) written out once more as torch operations with autograd, SGD and
ExponentialLR, in float32 (what the reference computes) or float64 (what it means):

    q = p + f;  c = R_j q + T_j;  h = K c;  (u, v) = h[:2] / h[2] at the view's valid points
    d = ((u, v) - pix0) - gt;  loss = (sum_j mean |d|) / divisor;  one SGD step per epoch, lr = 0.5 * 0.97^e

Both precisions get the SAME numbers as inputs -- the float32 values the kernel is given -- so the float64 run differs from the
float32 one by the arithmetic alone.  Results are computed once per case and shared (functools.lru_cache); callers do not modify
them."""
import functools
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G15 = os.path.join(ROOT, "tests", "golden", "g15_scene_flow_fit.npz")


def restate(points, K, R, T, valid, pix0, gt, epochs, divisor, dtype, lr=0.5, gamma=0.97):
    """Returns (flow [3,P], loss [E] (float64 numpy), flow2d_last: per view [2, n_j]) in `dtype`."""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        tt = lambda a: torch.tensor(np.asarray(a), dtype=dtype)
        p, Kt = tt(points), tt(K)
        Rt, Tt = [tt(r) for r in R], [tt(t).reshape(3, 1) for t in T]
        idx = [torch.as_tensor(np.asarray(v), dtype=torch.long) for v in valid]
        px, g = [tt(a) for a in pix0], [tt(a) for a in gt]
        f = torch.zeros_like(p, requires_grad=True)
        opt = torch.optim.SGD([f], lr=lr)
        sched = torch.optim.lr_scheduler.ExponentialLR(opt, gamma=gamma)
        losses, last = [], None
        for e in range(epochs):
            total, last = 0, []
            for j in range(len(idx)):
                h = torch.matmul(Kt, torch.matmul(Rt[j], p + f) + Tt[j])
                new = h[:2, idx[j]] / h[-1:, idx[j]] - px[j]
                total = total + torch.abs(new - g[j]).mean()
                last.append(new.detach())
            loss = total / divisor
            opt.zero_grad()
            loss.backward()
            opt.step()
            sched.step()
            losses.append(float(loss.detach()))
        return f.detach(), np.asarray(losses, np.float64), last
    finally:
        torch.set_num_threads(threads)


def loss_of(points, K, R, T, valid, pix0, gt, divisor, flow):
    """The loss of a given flow, float64."""
    tt = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)
    q = tt(points) + tt(flow)
    total = 0.0
    for j in range(len(valid)):
        h = torch.matmul(tt(K), torch.matmul(tt(R[j]), q) + tt(T[j]).reshape(3, 1))
        i = torch.as_tensor(np.asarray(valid[j]), dtype=torch.long)
        total = total + float(torch.abs(h[:2, i] / h[-1:, i] - tt(pix0[j]) - tt(gt[j])).mean())
    return total / divisor


# ------------------------------------------------------------------------------------------------ inputs
def _rot(ax, ay, az):
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    return (np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
            @ np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]))


def intrinsics(H, W):
    return np.array([[1.25 * W, 0, W / 2], [0, 1.25 * W, H / 2], [0, 0, 1]], np.float32)


def poses(V, seed):
    """V world-to-camera poses (R float64 [3,3], T float64 [3,1]); view 0 is the identity, the others turn by up to 0.04 rad and
    move by up to 0.08: at the test sizes (W <= 32, focal 1.25 W, depths >= 2.5) a projection moves by about 3 px at the most, so
    nearly every point 3 px inside the identity view's image is inside every view's, and a few near the border are not."""
    rng = np.random.default_rng(seed)
    out = [(np.eye(3), np.zeros((3, 1)))]
    for _ in range(V - 1):
        a = rng.uniform(-0.04, 0.04, 2)
        out.append((_rot(a[0], a[1], rng.uniform(-0.02, 0.02)), rng.uniform(-0.08, 0.08, (3, 1)) * np.array([[1], [1], [0.5]])))
    return out


def cloud(P, H, W, seed):
    """[3,P] float32.  P == 1: one point in the middle of the image.  P >= 4: point 0 lies outside every view, points 1 and 2
    1.2 px beyond the right edge of view 0 (outside it, inside whichever view looks a little further right), the rest at least
    3 px inside the identity view's image."""
    rng = np.random.default_rng(seed)
    K = intrinsics(H, W)
    z = rng.uniform(2.5, 4.0, P)
    u, v = rng.uniform(3.0, W - 4.0, P), rng.uniform(3.0, H - 4.0, P)
    if P == 1:
        u[0], v[0] = W / 2 + 0.3, H / 2 - 0.2
    if P >= 4:
        u[0], v[0] = 3.0 * W, -2.0 * H
        u[1:3] = W - 1 + 1.2
    return np.stack([(u - K[0, 2]) / K[0, 0] * z, (v - K[1, 2]) / K[1, 1] * z, z]).astype(np.float32)


class Case:
    """One fit: the inputs as the kernel's callers and `restate` take them."""
    def __init__(self, points, K, w2c, H, W, gt_maker, epochs, divisor=None):
        import importlib
        motion = importlib.import_module("iclr2025_3d-mom_amd.motion")
        self.points, self.K, self.H, self.W, self.epochs = points, K, H, W, epochs
        self.views = motion.prepare_views(points, K, w2c, H, W)
        self.gt = [np.asarray(gt_maker(j, self.views.valid[j], self.views.pix0[j]), np.float32) for j in range(self.views.V)]
        self.divisor = self.views.V if divisor is None else divisor

    def args(self):
        v = self.views
        return (self.points, self.K, v.R, v.T, v.valid, v.pix0, self.gt, self.epochs, self.divisor)

    @functools.lru_cache(maxsize=None)
    def ref(self, dtype):
        return restate(*self.args(), dtype)

    def loss_of(self, flow):
        v = self.views
        return loss_of(self.points, self.K, v.R, v.T, v.valid, v.pix0, self.gt, self.divisor, flow)


def _tiefree(seed):
    def make(j, idx, pix0):
        rng = np.random.default_rng(seed * 1000 + j)
        n = rng.standard_normal((2, len(idx)))
        return np.where(rng.random((2, len(idx))) < 0.5, -1.0, 1.0) * (0.5 + np.abs(n))
    return make


def _noise(seed, px=3.0):
    def make(j, idx, pix0):
        return np.random.default_rng(seed * 1000 + j).standard_normal((2, len(idx))) * px
    return make


@functools.lru_cache(maxsize=None)
def one_epoch_case(P, V):
    """Targets sign * (0.5 + |n|) px given directly at the points: after one epoch from a zero flow d = -gt, no sign near a tie."""
    return Case(cloud(P, 24, 24, seed=P), intrinsics(24, 24), poses(V, seed=V), 24, 24, _tiefree(P + V), epochs=1)


@functools.lru_cache(maxsize=None)
def noise_case(P, V):
    return Case(cloud(P, 24, 24, seed=P), intrinsics(24, 24), poses(V, seed=V), 24, 24, _noise(P + V), epochs=12)


def _compose(render, internal):
    out = []
    for Ri, Ti in render:
        for Rj, Tj in internal:
            out.append((Rj @ Ri, Rj @ Ti + Tj))                   # train_motion.py:152-153
    return out


@functools.lru_cache(maxsize=None)
def convergence_case(P, nr, ni, size, zero_half=False):
    """Targets: the exact float64 projection of a known flow 0.05 * N(0,1) minus the unflowed float64 pixel.  zero_half: the
    targets of every second point are exactly 0 (a static region)."""
    H = W = size
    K = intrinsics(H, W)
    w2c = _compose(poses(nr, seed=nr + 7), poses(ni, seed=ni + 11))
    pts = cloud(P, H, W, seed=P + 1)
    truth = np.random.default_rng(P).standard_normal((3, P)) * 0.05
    Kd = K.astype(np.float64)

    def make(j, idx, pix0):
        R, T = w2c[j]
        h0 = Kd @ (R @ pts.astype(np.float64) + T)
        h1 = Kd @ (R @ (pts.astype(np.float64) + truth) + T)
        g = (h1[:2] / h1[2:] - h0[:2] / h0[2:])[:, idx]
        if zero_half:
            g[:, idx % 2 == 1] = 0.0
        return g
    return Case(pts, K, w2c, H, W, make, epochs=200)


@functools.lru_cache(maxsize=None)
def g15():
    """The fixture written by tools/gen_sceneflow_golden.py from the reference's own optimize_motion."""
    d = np.load(G15)
    return {k: d[k] for k in d.files}


@functools.lru_cache(maxsize=None)
def g15_case():
    """g15's inputs as a Case: the poses composed as train_motion.py:147-153 does, the recorded sampled targets."""
    d = g15()
    w2c = _compose([(p[:3, :3], p[:3, 3:4]) for p in d["render_poses"]], [(p[:3, :3], p[:3, 3:4]) for p in d["internal_poses"]])
    return Case(d["points"], d["K"], w2c, int(d["H"]), int(d["W"]), lambda j, idx, pix0: d[f"gt_{j}"], epochs=int(d["epochs"]))


def g15_train_data():
    """A fresh train_data dict of g15's inputs, as optimize_motion takes it."""
    d = g15()
    frames = [{"T2C_flow": [torch.from_numpy(d["t2c_flow"][k].copy())], "our_flow": []} for k in range(len(d["t2c_flow"]))]
    return {"pcd_points": d["points"].copy(), "frames": frames}


def check_g15_mirror(train_data, scene_flow, bound=2e-6):
    """optimize_motion's two results on g15's inputs against the reference's: the scene flow within `bound` of its largest
    magnitude, every frame's our_flow image within `bound` of the pixel coordinates' magnitude (it interpolates differences of
    pixel coordinates; the triangulation is of the same float64 pixels).  Returns the two distances for printing."""
    d = g15()
    ref = d["scene_flow"]
    a = float(np.abs(np.asarray(scene_flow) - ref).max()) / scale(ref)
    assert a <= bound, a
    pixels = float(max(int(d["W"]), int(d["H"])) - 1)
    b = 0.0
    for k, fr in enumerate(train_data["frames"]):
        assert len(fr["our_flow"]) == 1 and tuple(fr["our_flow"][0].shape) == (1, 2, int(d["H"]), int(d["W"]))
        b = max(b, float(np.abs(fr["our_flow"][0].numpy() - d["our_flow"][k]).max()) / pixels)
    assert b <= bound, b
    return a, b


def scale(t):
    return float(np.abs(np.asarray(t)).max())
