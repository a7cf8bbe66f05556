"""Seeded synthetic inputs shared by the parity tests (numpy only, no torch needed)."""
import math
import os

import numpy as np


def projection_matrix(znear, zfar, fovx, fovy):
    """Row-major P of utils/graphics_utils.py:51-71 (reference), as float32."""
    ty, tx = math.tan(fovy / 2), math.tan(fovx / 2)
    top, right = ty * znear, tx * znear
    P = np.zeros((4, 4), np.float32)
    P[0, 0] = 2.0 * znear / (2 * right)
    P[1, 1] = 2.0 * znear / (2 * top)
    P[3, 2] = 1.0
    P[2, 2] = zfar / (zfar - znear)
    P[2, 3] = -(zfar * znear) / (zfar - znear)
    return P


def camera(W, H, R=None, T=None, focal=None, fovx=None, fovy=None, dtype=np.float32):
    """Returns dict(viewmatrix, projmatrix (both transposed, as the rasterizer wants), campos, tanfovx, tanfovy).  R is
    camera-to-world and T the world-to-camera translation (w2c = [R^T | T], the reference's getWorld2View2).  fovx / fovy
    (radians) replace the fields of view derived from `focal`; dtype=np.float64 keeps the matrices unrounded (for the fp64
    oracle builds: a float32 rotation is orthogonal only to 6e-8)."""
    R = np.eye(3) if R is None else np.asarray(R, np.float64)
    T = np.zeros(3) if T is None else np.asarray(T, np.float64)
    focal = 582.69 if focal is None else focal  # train_motion.py:52-56 style intrinsics
    fovx = 2 * math.atan(W / (2 * focal)) if fovx is None else fovx
    fovy = 2 * math.atan(H / (2 * focal)) if fovy is None else fovy
    Rt = np.zeros((4, 4))
    Rt[:3, :3] = R.T
    Rt[:3, 3] = T
    Rt[3, 3] = 1.0
    w2c = Rt.astype(dtype)
    view = w2c.T.copy()
    proj = projection_matrix(0.01, 100.0, fovx, fovy).T.copy()
    full = (view @ proj).astype(dtype)
    campos = np.linalg.inv(view.astype(np.float64))[3, :3].astype(dtype)
    return dict(viewmatrix=view, projmatrix=full, campos=campos, tanfovx=math.tan(fovx * 0.5),
                tanfovy=math.tan(fovy * 0.5), W=W, H=H)


def _rot(axis, degrees):
    c, s = math.cos(math.radians(degrees)), math.sin(math.radians(degrees))
    i, j = {"x": (1, 2), "y": (2, 0), "z": (0, 1)}[axis]
    M = np.eye(3)
    M[i, i], M[i, j], M[j, i], M[j, j] = c, -s, s, c
    return M


def _golden(name):
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name))


def pose(name):
    """The named camera poses of the posed parity tests, as keyword arguments of camera() / random_gaussians():
      identity  today's camera: view = I, campos = 0
      yaw90     a quarter turn about y: R's exact zeros and ones sit elsewhere than the identity's, nothing rounds
      general   yaw 37, pitch -21, roll 13 degrees, T = (0.4, -0.3, 2.5): no zero in R, the camera centre far from the origin
      slide     pose 0 of the reference's `side` render trajectory (golden/g9_side_trajectory.npz): translation only
      ref17     R17 / T17 / fov of golden/g5_cameras.npz: the reference's own camera 17 (R17 is the identity, as all of the
                reference's cameras here are; `general` carries the rotation), fovx == fovy whatever W / H is"""
    if name == "identity":
        return {}
    if name == "yaw90":
        return dict(R=np.array([[0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [-1.0, 0.0, 0.0]]), T=np.zeros(3))
    if name == "general":
        return dict(R=_rot("y", 37.0) @ _rot("x", -21.0) @ _rot("z", 13.0), T=np.array([0.4, -0.3, 2.5]))
    if name == "slide":
        d = _golden("g9_side_trajectory.npz")
        return dict(R=d["R"][0].astype(np.float64), T=d["t"][0].astype(np.float64))
    if name == "ref17":
        d = _golden("g5_cameras.npz")
        return dict(R=d["R17"], T=d["T17"], fovx=float(d["fov"][0]), fovy=float(d["fov"][1]))
    raise KeyError(name)


POSES = ("yaw90", "general", "slide", "ref17")


def view_space(means3D, viewmatrix):
    """float64 view-space coordinates of `means3D` under a (transposed) view matrix."""
    v = np.asarray(viewmatrix, np.float64).reshape(4, 4)
    return np.asarray(means3D, np.float64) @ v[:3, :3] + v[3, :3]


def to_world(p_cam, R=None, T=None, **_):
    """float64 world coordinates of view-space points under camera(R=R, T=T): p_world = R (p_cam - T)."""
    R = np.eye(3) if R is None else np.asarray(R, np.float64)
    T = np.zeros(3) if T is None else np.asarray(T, np.float64)
    return (np.asarray(p_cam, np.float64) - T) @ R.T


def quat_of(R):
    """(r, x, y, z) of a rotation matrix whose angle is well below 180 degrees (all named poses)."""
    R = np.asarray(R, np.float64)
    r = 0.5 * math.sqrt(1.0 + R[0, 0] + R[1, 1] + R[2, 2])
    assert r > 0.1
    return np.array([r, (R[2, 1] - R[1, 2]) / (4 * r), (R[0, 2] - R[2, 0]) / (4 * r), (R[1, 0] - R[0, 1]) / (4 * r)])


def quat_left(a):
    """L(a) with a (x) q = L(a) q for quaternions (r, x, y, z)."""
    ar, ax, ay, az = a
    return np.array([[ar, -ax, -ay, -az], [ax, ar, -az, ay], [ay, az, ar, -ax], [az, -ay, ax, ar]])


def rigid_move(s, R, T, dtype=np.float32, **intrinsics):
    """The scene `s` (posed for the identity camera) and its camera both moved by the rigid motion G = (R, T): the means to
    R (p - T), every quaternion left-multiplied by the quaternion of R (the world covariance becomes R Sigma R^T), the camera to
    camera(R, T).  View-space positions and covariances are those of `s`, so at SH degree 0 (a colour that does not depend on the
    view direction) the frame is the same frame."""
    out = dict(s)
    out.update(camera(s["W"], s["H"], R=R, T=T, dtype=dtype, **intrinsics))
    out["means3D"] = to_world(s["means3D"], R, T).astype(dtype)
    out["rotations"] = (np.asarray(s["rotations"], np.float64) @ quat_left(quat_of(R)).T).astype(dtype)
    return out


def random_gaussians(P, seed=0, W=128, H=96, zrange=(1.0, 6.0), scale=(-4.5, -2.0), sh_coeffs=16, focal=None, R=None, T=None,
                     fovx=None, fovy=None, spread=1.3):
    """Random Gaussians spread over (and slightly beyond) the frustum of camera(W, H, R, T): drawn in camera space, laterally
    within `spread` x tan(fov/2) x z, and taken to world space with the inverse pose in float64, p_world = R (p_cam - T).
    With the default pose the arrays are those of every earlier version of this function, bit for bit."""
    rng = np.random.default_rng(seed)
    cam = camera(W, H, R=R, T=T, focal=focal, fovx=fovx, fovy=fovy)
    z = rng.uniform(*zrange, P)
    # a few behind / at the near plane to exercise the cull (auxiliary.h:154)
    n_near = max(1, P // 50)
    z[:n_near] = rng.uniform(-1.0, 0.25, n_near)
    x = rng.uniform(-spread, spread, P) * cam["tanfovx"] * z
    y = rng.uniform(-spread, spread, P) * cam["tanfovy"] * z
    means = np.stack([x, y, z], 1)
    if R is not None or T is not None:
        means = to_world(means, R, T)
    means = means.astype(np.float32)
    scales = np.exp(rng.uniform(scale[0], scale[1], (P, 3))).astype(np.float32)
    rots = rng.normal(size=(P, 4)).astype(np.float32)
    rots /= np.linalg.norm(rots, axis=1, keepdims=True)
    opac = (1 / (1 + np.exp(-rng.normal(0, 2, (P, 1))))).astype(np.float32)
    shs = (rng.normal(0, 0.3, (P, sh_coeffs, 3))).astype(np.float32)
    shs[:, 0, :] += rng.uniform(0, 2.0, (P, 3)).astype(np.float32)
    bg = np.array([0.1, 0.2, 0.3], np.float32)
    return dict(means3D=means, scales=scales, rotations=rots, opacities=opac, shs=shs, bg=bg, **cam)


def posed_gaussians(P, pose_name, W=128, H=96, scale=(-4.5, -2.0), **kw):
    """random_gaussians() under a named pose.  A pose with fields of view of its own (ref17's are twice the default camera's at
    W = 256) keeps the splats' size in PIXELS: the log-scale range moves by log(tan(fov/2) / the default camera's), which is 0
    for every pose that keeps the default intrinsics."""
    kp = pose(pose_name)
    if "fovx" in kp:
        shift = math.log(math.tan(kp["fovx"] * 0.5) / camera(W, H, focal=kw.get("focal"))["tanfovx"])
        scale = (scale[0] + shift, scale[1] + shift)
    return random_gaussians(P, W=W, H=H, scale=scale, **kw, **kp)


def near_plane_scene(P, pose_name, seed):
    """Means for the visibility tests: random_gaussians under the pose, a quarter of them moved to a view-space depth just either
    side of the 0.2 cull (1e-4 .. 1e-2 away), none left within 1e-5 of it (float32 evaluation of the depth is good to ~1e-6
    here, so the float64 answer is the answer).  Returns the scene and the float64 expectation z_view > 0.2."""
    s = posed_gaussians(P, pose_name, seed=seed)
    rng = np.random.default_rng(seed + 1)
    pv = view_space(s["means3D"], s["viewmatrix"])
    sel = np.arange(P) % 4 == 1
    pv[sel, 2] = 0.2 + rng.choice([-1.0, 1.0], sel.sum()) * 10.0 ** rng.uniform(-4, -2, sel.sum())
    s["means3D"] = to_world(pv, **pose(pose_name)).astype(np.float32)
    z = view_space(s["means3D"], s["viewmatrix"])[:, 2]
    keep = np.abs(z - 0.2) > 1e-5
    assert keep.sum() >= P - 2
    z = np.where(keep, z, 1.0)
    s["means3D"][~keep] = to_world(np.array([[0.0, 0.0, 1.0]]), **pose(pose_name)).astype(np.float32)
    return s, z > 0.2


def clamp_some_channels(s, seed=0, frac=0.3):
    """Give a fraction of the Gaussians a strongly negative DC term in one channel (in place): their colour from SH falls below
    zero there, so the rasterizer clamps it and its backward masks that channel's colour gradient."""
    rng = np.random.default_rng(seed)
    P = s["shs"].shape[0]
    sel = np.nonzero(rng.random(P) < frac)[0]
    ch = rng.integers(0, 3, len(sel))
    s["shs"][sel, 0, ch] = rng.uniform(-4.0, -1.5, len(sel)).astype(np.float32)
    return s
