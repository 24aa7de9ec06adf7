"""Shared by tests/test_eval_render.py (GPU), tests/test_eval_render_host.py (CPU) and
tools/time_eval_render.py: the render / visibility contract of include/apd_eval.h restated literally
in float32 numpy (which does not contract), and the scenes the tests draw."""
import numpy as np

import apd_abi as A

f32 = np.float32
INT32_MIN = -(2 ** 31)
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)


def make_cam(K, R, t, width, height):
    """ApdCamera from float matrices (rounded to float32, as the library sees them)."""
    return A.camera_from_values(dict(K=np.asarray(K, f32), R=np.asarray(R, f32), t=np.asarray(t, f32),
                                     width=width, height=height))


def cam_arrays(cam):
    return np.array(cam.K[:], f32), np.array(cam.R[:], f32), np.array(cam.t[:], f32), int(cam.width), int(cam.height)


def trunc_x86(v):
    """int(v) as cvttss2si: truncation; INT32_MIN for NaN and out-of-range values (the guard comes
    before the integer conversion)."""
    v = np.asarray(v, f32)
    ok = (v >= f32(-2147483648.0)) & (v < f32(2147483648.0))
    out = np.full(v.shape, INT32_MIN, np.int64)
    out[ok] = np.trunc(v[ok]).astype(np.int64)
    return out


def project_ref(xyz, cam):
    """(kept, d, u, v): elementwise float32, every sum left to right."""
    K, R, t, _, _ = cam_arrays(cam)
    p = np.ascontiguousarray(xyz, f32).reshape(-1, 3)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        tx = R[0] * x + R[1] * y + R[2] * z + t[0]
        ty = R[3] * x + R[4] * y + R[5] * z + t[1]
        tz = R[6] * x + R[7] * y + R[8] * z + t[2]
        d = K[6] * tx + K[7] * ty + K[8] * tz
        px = (K[0] * tx + K[1] * ty + K[2] * tz) / d
        py = (K[3] * tx + K[4] * ty + K[5] * tz) / d
        assert d.dtype == f32 and px.dtype == f32
        kept = np.isfinite(p).all(axis=1) & (d > 0) & (d < f32(np.inf))
        u = trunc_x86(px + f32(0.5))
        v = trunc_x86(py + f32(0.5))
    return kept, d, u, v


def render_ref(xyz, cam, splat=0):
    """(depth (H, W) float32, index (H, W) int32): minimum of (bits(d) << 32) | i over the clipped
    footprint of every kept point."""
    _, _, _, W, H = cam_arrays(cam)
    kept, d, u, v = project_ref(xyz, cam)
    i = np.flatnonzero(kept)
    key = (d[i].view(np.uint32).astype(np.uint64) << np.uint64(32)) | i.astype(np.uint64)
    plane = np.full(W * H, EMPTY, np.uint64)
    for db in range(-splat, splat + 1):
        for da in range(-splat, splat + 1):
            a, b = u[i] + da, v[i] + db  # int64: no overflow, INT32_MIN stays far outside
            m = (a >= 0) & (a < W) & (b >= 0) & (b < H)
            np.minimum.at(plane, b[m] * W + a[m], key[m])
    hit = plane != EMPTY
    depth = np.where(hit, (plane >> np.uint64(32)).astype(np.uint32).view(f32), f32(0)).astype(f32)
    index = np.where(hit, (plane & np.uint64(0xFFFFFFFF)).astype(np.int64), -1).astype(np.int32)
    return depth.reshape(H, W), index.reshape(H, W)


def visible_ref(xyz, cam, depth, rel_tol):
    """bool[n]: the z-buffer test of one view (centre pixel only)."""
    _, _, _, W, H = cam_arrays(cam)
    kept, d, u, v = project_ref(xyz, cam)
    depth = np.ascontiguousarray(depth, f32).reshape(H, W)
    inb = kept & (u >= 0) & (u < W) & (v >= 0) & (v < H)
    factor = f32(1.0) + f32(rel_tol)
    out = np.zeros(len(d), bool)
    j = np.flatnonzero(inb)
    with np.errstate(all="ignore"):
        z = depth[v[j], u[j]]
        out[j] = (z > 0) & (d[j] <= z * factor)
    return out


def seen_ref(xyz, cams, depths, rel_tol):
    n = len(np.asarray(xyz).reshape(-1, 3))
    seen = np.zeros(n, np.int32)
    for cam, dep in zip(cams, depths):
        seen += visible_ref(xyz, cam, dep, rel_tol)
    return seen


# ---- scenes ---------------------------------------------------------------------------------------

def two_wall_camera(width=67, height=49):
    """A small rotation about y and a non-zero translation."""
    a = 0.05
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    K = np.array([[60.0, 0, width / 2 - 0.3], [0, 60.0, height / 2 + 0.2], [0, 0, 1]])
    return make_cam(K, R, [0.05, -0.02, 0.1], width, height)


def two_wall_cloud(seed=5):
    """About 900 points on a front wall (z about 2, the left half of the image), about 2 600 on a back
    wall (z about 4) that extends beyond all four image borders, 100 points behind the camera, the
    first 50 points again as exact duplicates, and rows with NaN, +inf and -inf.
    Returns (cloud, slices by name)."""
    rng = np.random.default_rng(seed)
    front = np.column_stack([rng.uniform(-1.15, 0.0, 900), rng.uniform(-0.85, 0.85, 900),
                             2.0 + rng.normal(0, 0.01, 900)])
    back = np.column_stack([rng.uniform(-2.9, 2.9, 2600), rng.uniform(-2.2, 2.2, 2600),
                            4.0 + rng.normal(0, 0.01, 2600)])
    behind = np.column_stack([rng.uniform(-1, 1, (100, 2)), rng.uniform(-3, -0.5, 100)])
    bad = np.array([[np.nan, 0, 2], [0, np.inf, 2], [0, 0, -np.inf], [np.inf, -np.inf, np.nan], [0.1, 0.1, np.inf]])
    pts = np.concatenate([front, back, behind]).astype(f32)
    cloud = np.concatenate([pts, pts[:50], bad.astype(f32)]).astype(f32)
    parts = {"front": slice(0, 900), "back": slice(900, 3500), "behind": slice(3500, 3600),
             "dup": slice(3600, 3650), "bad": slice(3650, 3655)}
    return cloud, parts


def sheet(rng, n, noise=0.001, side=10.0):
    """The wavy sheet of tools/time_eval.py."""
    xy = rng.uniform(-side / 2, side / 2, (n, 2))
    z = 6.0 + 0.3 * np.sin(xy[:, 0]) * np.cos(0.7 * xy[:, 1]) + rng.normal(0, noise, n)
    return np.column_stack([xy, z]).astype(f32)
