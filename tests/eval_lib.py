"""Shared by tests/test_eval.py (GPU) and tests/test_eval_host.py (CPU): the brute-force reference of
include/apd_eval.h's distance contract, PLY writers in the layouts the reader must accept, and the
path of the `apd_eval` binary."""
import os

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(REPO, "apde-mvs_amd", "host")
APD_EVAL = os.path.join(HOST, "build", "apd_eval")
f32 = np.float32
INF = f32(np.inf)


def brute(q, t, max_dist):
    """The contract restated literally in float32 numpy (which does not contract): per pair dx*dx,
    dy*dy, dz*dz, (a + b) + c, min over the finite targets, sqrt, then the cut."""
    q = np.asarray(q, f32).reshape(-1, 3)
    t = np.asarray(t, f32).reshape(-1, 3)
    t = t[np.isfinite(t).all(axis=1)]
    out = np.full(len(q), INF, f32)
    if len(t) == 0:
        return out
    md = f32(max_dist)
    with np.errstate(all="ignore"):
        for s in range(0, len(q), 256):
            c = q[s:s + 256]
            dx = c[:, None, 0] - t[None, :, 0]
            dy = c[:, None, 1] - t[None, :, 1]
            dz = c[:, None, 2] - t[None, :, 2]
            d2 = (dx * dx + dy * dy) + dz * dz
            assert d2.dtype == f32
            m = np.sqrt(d2.min(axis=1))
            out[s:s + 256] = np.where(m <= md, m, INF)
    out[~np.isfinite(q).all(axis=1)] = INF
    return out


def same_bits(a, b):
    a = np.ascontiguousarray(a, f32)
    b = np.ascontiguousarray(b, f32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def voxel_ref(x, v):
    x = np.asarray(x, f32).reshape(-1, 3)
    fin = np.flatnonzero(np.isfinite(x).all(axis=1))
    if len(fin) == 0:
        return np.zeros(0, np.int32)
    keys = np.floor(x[fin] / f32(v)).astype(np.int64)
    first = np.unique(keys, axis=0, return_index=True)[1]
    return np.sort(fin[first]).astype(np.int32)


def ply_apd_layout(xyz, rng=None):
    """APD.ply's 15-byte records: float x, y, z + uchar blue, green, red."""
    xyz = np.ascontiguousarray(xyz, "<f4").reshape(-1, 3)
    rec = np.zeros(len(xyz), np.dtype([("p", "<f4", 3), ("c", "u1", 3)]))
    rec["p"] = xyz
    rec["c"] = 200 if rng is None else rng.integers(0, 256, (len(xyz), 3))
    assert rec.dtype.itemsize == 15
    hdr = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\n"
           "property float z\nproperty uchar blue\nproperty uchar green\nproperty uchar red\nend_header\n" % len(xyz))
    return hdr.encode() + rec.tobytes()


def ply_gt_layout(xyz):
    """Comments, obj_info, an extra double in front, an extra float between the coordinates (which
    are not in x, y, z order in the record), and a later face element that must be ignored."""
    xyz = np.ascontiguousarray(xyz, "<f4").reshape(-1, 3)
    rec = np.zeros(len(xyz), np.dtype([("t", "<f8"), ("z", "<f4"), ("s", "<f4"), ("x", "<f4"), ("y", "<f4"),
                                       ("l", "<u2")]))
    rec["t"], rec["s"], rec["l"] = 1.5, -7.0, 9
    rec["x"], rec["y"], rec["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    hdr = ("ply\nformat binary_little_endian 1.0\ncomment made by tests/eval_lib.py\nobj_info scanner 1\n"
           "element vertex %d\nproperty double time\nproperty float z\ncomment between properties\n"
           "property float32 scalar_intensity\nproperty float x\nproperty float y\nproperty ushort label\n"
           "element face 1\nproperty list uchar int vertex_indices\nend_header\n" % len(xyz))
    return hdr.encode() + rec.tobytes() + bytes([3]) + np.array([0, 1, 2], "<i4").tobytes()


def plane_pair(rng, n=4000):
    """A reconstruction and a ground truth of about n points each: two noisy samplings of the plane
    z = 0.1 x + 2 (different noise levels), plus outliers far from it in the reconstruction and a
    patch the reconstruction misses in the ground truth."""
    def plane(m, noise):
        xy = rng.uniform(-1, 1, (m, 2))
        z = 0.1 * xy[:, 0] + 2.0 + rng.normal(0, noise, m)
        return np.column_stack([xy, z])
    rec = np.concatenate([plane(n - 150, 0.02), rng.uniform(-3, 3, (150, 3)) + [0, 0, 6]]).astype(f32)
    gt = np.concatenate([plane(n - 300, 0.002), plane(300, 0.002) + [3.0, 0, 0]]).astype(f32)
    return rec, gt
