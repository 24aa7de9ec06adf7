"""Literal numpy restatement of the contract in include/apd_prep.h (pair counts, score, depth ranks,
selection), written from the contract and not from the reference's script, plus writers of COLMAP
models (text and binary) and small synthetic models for the tests. Everything is IEEE double,
element-wise (numpy fuses nothing), sums left to right as the contract writes them."""
import os
import struct

import numpy as np

f64 = np.float64


# ---- model ---------------------------------------------------------------------------------------------

def rotation_ref(q):
    w, x, y, z = (f64(v) for v in q)
    return np.array([[(1 - 2 * (y * y)) - 2 * (z * z), (2 * x) * y - (2 * w) * z, (2 * z) * x + (2 * w) * y],
                     [(2 * x) * y + (2 * w) * z, (1 - 2 * (x * x)) - 2 * (z * z), (2 * y) * z - (2 * w) * x],
                     [(2 * z) * x - (2 * w) * y, (2 * y) * z + (2 * w) * x, (1 - 2 * (x * x)) - 2 * (y * y)]], f64)


def centre_ref(R, t):
    return np.array([-((R[0][k] * t[0] + R[1][k] * t[1]) + R[2][k] * t[2]) for k in range(3)], f64)


def model_ref(images, point_ids, xyz):
    """images (dicts: id, qvec, tvec, point_ids) in any order -> renumbered in ascending id:
    rot (n,3,3), trans (n,3), centres (n,3), obs: per image the list of point INDICES (ids -1 dropped,
    duplicates kept). A point id missing from point_ids raises KeyError."""
    index = {int(p): k for k, p in enumerate(np.asarray(point_ids).tolist())}
    ims = sorted(images, key=lambda im: int(im["id"]))
    rot = np.array([rotation_ref(im["qvec"]) for im in ims], f64).reshape(-1, 3, 3)
    trans = np.array([im["tvec"] for im in ims], f64).reshape(-1, 3)
    cen = np.array([centre_ref(R, t) for R, t in zip(rot, trans)], f64).reshape(-1, 3)
    obs = [np.array([index[int(p)] for p in np.asarray(im["point_ids"]).tolist() if int(p) != -1], np.int64)
           for im in ims]
    return {"rot": rot, "trans": trans, "centres": cen, "xyz": np.asarray(xyz, f64).reshape(-1, 3), "obs": obs}


def csr(obs):
    off = np.zeros(len(obs) + 1, np.int64)
    off[1:] = np.cumsum([len(o) for o in obs])
    pts = np.concatenate(obs).astype(np.int32) if len(obs) and off[-1] else np.zeros(0, np.int32)
    return off, pts


# ---- pair counts ---------------------------------------------------------------------------------------

def cos_ref(ca, cb, p):
    """q of the contract for arrays of centres and points (m, 3)."""
    u, v = ca - p, cb - p
    with np.errstate(invalid="ignore", divide="ignore"):
        return (((u[:, 0] * v[:, 0] + u[:, 1] * v[:, 1]) + u[:, 2] * v[:, 2]) /
                np.sqrt((u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1]) + u[:, 2] * u[:, 2])) / \
            np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])


def pair_records_ref(obs):
    """(point, a, b) of every record: per point the unordered pairs a < b of the distinct images that see it."""
    n = len(obs)
    pt = np.concatenate([np.asarray(o, np.int64) for o in obs]) if n else np.zeros(0, np.int64)
    im = np.concatenate([np.full(len(o), i, np.int64) for i, o in enumerate(obs)]) if n else np.zeros(0, np.int64)
    key = np.unique(pt * n + im)  # duplicates within an image collapse; sorted by (point, image)
    pt, im = key // n, key % n
    P, A, B = [], [], []
    if len(pt):
        starts = np.flatnonzero(np.r_[True, pt[1:] != pt[:-1]])
        ends = np.r_[starts[1:], len(pt)]
        for s, e in zip(starts.tolist(), ends.tolist()):
            L = e - s
            if L < 2:
                continue
            a, b = np.triu_indices(L, 1)
            P.append(np.full(len(a), pt[s], np.int64))
            A.append(im[s + a])
            B.append(im[s + b])
    if not P:
        z = np.zeros(0, np.int64)
        return z, z, z
    return np.concatenate(P), np.concatenate(A), np.concatenate(B)


def pair_counts_ref(centres, xyz, obs, q_gate):
    n = len(obs)
    P, A, B = pair_records_ref(obs)
    q = cos_ref(centres[A], centres[B], xyz[P]) if len(P) else np.zeros(0, f64)
    with np.errstate(invalid="ignore"):
        nar = q >= q_gate
    up_s = np.bincount(A * n + B, minlength=n * n).reshape(n, n)
    up_n = np.bincount((A * n + B)[nar], minlength=n * n).reshape(n, n)
    return (up_s + up_s.T).astype(np.uint32), (up_n + up_n.T).astype(np.uint32), len(P)


def score_ref(shared, narrow):
    s = shared.astype(np.int64)
    out = s.copy()
    out[narrow.astype(np.int64) >= (3 * s) // 4 + 1] = 0
    return out


def select_ref(score, max_views=20):
    n = len(score)
    sel = []
    for i in range(n):
        cand = [j for j in range(n) if j != i]
        cand.sort(key=lambda j: (-int(score[i, j]), j))
        sel.append([(j, int(score[i, j])) for j in cand[:min(max_views, n - 1)]])
    return sel


def sequential_ref(n, k):
    """Window of +-k: score k + 1 - offset, ordered by (score descending, distance ascending) with the
    lower neighbour first among equals (a stable sort of the offsets visited -1 before +1)."""
    sel = []
    for i in range(n):
        nb = []
        for off in range(1, k + 1):
            for j in (i - off, i + off):
                if 0 <= j < n:
                    nb.append((j, k + 1 - off))
        sel.append(nb[:min(n - 1, 2 * k)])
    return sel


# ---- depth ranks ---------------------------------------------------------------------------------------

def _enc(z):
    u = np.asarray(z, f64).view(np.uint64)
    return np.where(u >> np.uint64(63), ~u, u | np.uint64(1 << 63))


def _dec(e):
    u = np.where(e >> np.uint64(63), e & np.uint64((1 << 63) - 1), ~e)
    return u.astype(np.uint64).view(f64)


def depth_ranks_ref(rot, trans, xyz, obs, fractions):
    n = len(obs)
    z_at = np.zeros((n, len(fractions)), f64)
    cnt = np.zeros(n, np.int64)
    for i, o in enumerate(obs):
        cnt[i] = len(o)
        if not len(o):
            continue
        p = xyz[np.asarray(o, np.int64)]
        R = rot[i]
        z = ((R[2, 0] * p[:, 0] + R[2, 1] * p[:, 1]) + R[2, 2] * p[:, 2]) + trans[i, 2]
        s = _dec(np.sort(_enc(z)))
        for k, f in enumerate(fractions):
            z_at[i, k] = s[min(int(float(len(o)) * float(f)), len(o) - 1)]
    return z_at, cnt


def depth_range_ref(z01, z99, n_obs, max_d, interval_scale, fx):
    """(depth_min, interval, depth_num, depth_max) of one image (doubles, the contract's host part)."""
    dmin, dmax = (f64(z01) * 0.75, f64(z99) * 1.25) if n_obs else (f64(0), f64(0))
    with np.errstate(all="ignore"):
        if max_d == 0:
            num = (1 / dmin - 1 / dmax) / (1 / dmin - 1 / (dmin + dmin / f64(fx)))
        else:
            num = f64(max_d)
        return dmin, (dmax - dmin) / (num - 1) / f64(interval_scale), num, dmax


def same_bits64(a, b):
    a, b = np.ascontiguousarray(a, f64), np.ascontiguousarray(b, f64)
    return a.shape == b.shape and bool(np.all(a.view(np.uint64) == b.view(np.uint64)))


# ---- synthetic models ----------------------------------------------------------------------------------

def random_quat(rng):
    q = rng.normal(size=4)
    return q / np.linalg.norm(q)


def ring_model(n_images, n_points, rng, mean_track=8.0, first_id=1, id_step=1, point_id=lambda k: k + 1):
    """Cameras on a ring looking at a blob of points; every point is seen by a random window of
    neighbouring images. Returns (images, point_ids, xyz)."""
    xyz = rng.normal(scale=0.5, size=(n_points, 3))
    ids = np.array([point_id(k) for k in range(n_points)], np.int64)
    images = []
    seen = [[] for _ in range(n_images)]
    for k in range(n_points):
        L = min(n_images, max(0, int(rng.poisson(mean_track))))
        s = int(rng.integers(0, n_images))
        for d in range(L):
            seen[(s + d) % n_images].append(int(ids[k]))
    for i in range(n_images):
        a = 2 * np.pi * i / max(n_images, 1)
        c = np.array([4 * np.cos(a), 4 * np.sin(a), 0.3 * np.sin(3 * a)])
        fwd = -c / np.linalg.norm(c)
        right = np.cross(fwd, [0, 0, 1.0])
        right /= np.linalg.norm(right)
        down = np.cross(fwd, right)
        R = np.stack([right, down, fwd])
        w = np.sqrt(max(1e-12, 1 + R[0, 0] + R[1, 1] + R[2, 2])) / 2
        q = np.array([w, (R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w)])
        t = -R @ c
        p = np.array(seen[i], np.int64)
        rng.shuffle(p)
        images.append({"id": first_id + id_step * i, "qvec": q, "tvec": t, "point_ids": p, "camera_id": 1,
                       "name": "img%04d.png" % i})
    return images, ids, xyz


# ---- COLMAP files --------------------------------------------------------------------------------------

MODEL_IDS = {"SIMPLE_PINHOLE": 0, "PINHOLE": 1, "SIMPLE_RADIAL": 2}


def write_colmap_text(d, cameras, images, point_ids, xyz):
    """cameras: dicts id, model, width, height, params. images as above (+ camera_id, name; xys optional)."""
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "cameras.txt"), "w") as f:
        f.write("# Camera list with one line of data per camera:\n#   CAMERA_ID, MODEL, WIDTH, HEIGHT, PARAMS[]\n")
        for c in cameras:
            f.write("%d %s %d %d %s\n" % (c["id"], c["model"], c["width"], c["height"],
                                          " ".join(repr(float(p)) for p in c["params"])))
    with open(os.path.join(d, "images.txt"), "w") as f:
        f.write("# Image list with two lines of data per image:\n")
        for im in images:
            f.write("%d %s %s %d %s\n" % (im["id"], " ".join(repr(float(v)) for v in im["qvec"]),
                                          " ".join(repr(float(v)) for v in im["tvec"]), im["camera_id"], im["name"]))
            xys = im.get("xys")
            f.write(" ".join("%s %s %d" % (repr(float(xys[k][0])) if xys is not None else "1.5",
                                           repr(float(xys[k][1])) if xys is not None else "2.5", int(p))
                             for k, p in enumerate(np.asarray(im["point_ids"]).tolist())) + "\n")
    with open(os.path.join(d, "points3D.txt"), "w") as f:
        f.write("# 3D point list with one line of data per point:\n")
        for p, x in zip(np.asarray(point_ids).tolist(), np.asarray(xyz, f64).reshape(-1, 3)):
            f.write("%d %s 10 20 30 0.5 1 0\n" % (p, " ".join(repr(float(v)) for v in x)))


def write_colmap_bin(d, cameras, images, point_ids, xyz):
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "cameras.bin"), "wb") as f:
        f.write(struct.pack("<Q", len(cameras)))
        for c in cameras:
            f.write(struct.pack("<iiQQ", c["id"], MODEL_IDS[c["model"]], c["width"], c["height"]))
            f.write(struct.pack("<%dd" % len(c["params"]), *[float(p) for p in c["params"]]))
    with open(os.path.join(d, "images.bin"), "wb") as f:
        f.write(struct.pack("<Q", len(images)))
        for im in images:
            f.write(struct.pack("<i4d3di", im["id"], *[float(v) for v in im["qvec"]], *[float(v) for v in im["tvec"]],
                                im["camera_id"]))
            f.write(im["name"].encode() + b"\0")
            pids = np.asarray(im["point_ids"]).tolist()
            xys = im.get("xys")
            f.write(struct.pack("<Q", len(pids)))
            for k, p in enumerate(pids):
                f.write(struct.pack("<ddq", float(xys[k][0]) if xys is not None else 1.5,
                                    float(xys[k][1]) if xys is not None else 2.5, int(p)))
    with open(os.path.join(d, "points3D.bin"), "wb") as f:
        f.write(struct.pack("<Q", len(point_ids)))
        for p, x in zip(np.asarray(point_ids).tolist(), np.asarray(xyz, f64).reshape(-1, 3)):
            f.write(struct.pack("<Q3d3BdQ", p, *[float(v) for v in x], 10, 20, 30, 0.5, 1))
            f.write(struct.pack("<ii", 1, 0))


# ---- scans for the binary ------------------------------------------------------------------------------

def quat_from_R(R):
    """(w, x, y, z) of a proper rotation matrix (largest-component branch)."""
    R = np.asarray(R, f64)
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    if tr > 0:
        s = np.sqrt(tr + 1.0) * 2
        q = [0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s]
    elif R[0, 0] > R[1, 1] and R[0, 0] > R[2, 2]:
        s = np.sqrt(1.0 + R[0, 0] - R[1, 1] - R[2, 2]) * 2
        q = [(R[2, 1] - R[1, 2]) / s, 0.25 * s, (R[0, 1] + R[1, 0]) / s, (R[0, 2] + R[2, 0]) / s]
    elif R[1, 1] > R[2, 2]:
        s = np.sqrt(1.0 + R[1, 1] - R[0, 0] - R[2, 2]) * 2
        q = [(R[0, 2] - R[2, 0]) / s, (R[0, 1] + R[1, 0]) / s, 0.25 * s, (R[1, 2] + R[2, 1]) / s]
    else:
        s = np.sqrt(1.0 + R[2, 2] - R[0, 0] - R[1, 1]) * 2
        q = [(R[1, 0] - R[0, 1]) / s, (R[0, 2] + R[2, 0]) / s, (R[1, 2] + R[2, 1]) / s, 0.25 * s]
    return np.array(q, f64)


def write_png(path, bgr):
    """8-bit colour PNG of a (h, w, 3) BGR array, by PIL."""
    from PIL import Image
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(np.ascontiguousarray(bgr[:, :, ::-1], np.uint8), mode="RGB").save(path)


def scene_to_colmap(scene, rng, n_points=400):
    """A synth.Scene as a COLMAP model: PINHOLE camera, images with their poses, and a sample of the
    ground-truth surface as points, observed wherever they project inside an image."""
    import synth
    cloud = synth.gt_cloud(scene).astype(f64)
    xyz = cloud[rng.choice(len(cloud), min(n_points, len(cloud)), replace=False)]
    pids = np.arange(1, len(xyz) + 1, dtype=np.int64)
    K = scene.cameras[0].K
    cams = [{"id": 1, "model": "PINHOLE", "width": scene.width, "height": scene.height,
             "params": [K[0, 0], K[1, 1], K[0, 2], K[1, 2]]}]
    images = []
    for i, cam in enumerate(scene.cameras):
        p = xyz @ cam.R.T + cam.t
        uv = p @ cam.K.T
        u, v = uv[:, 0] / uv[:, 2], uv[:, 1] / uv[:, 2]
        ok = (p[:, 2] > 0) & (u >= 0) & (u <= scene.width - 1) & (v >= 0) & (v <= scene.height - 1)
        images.append({"id": i + 1, "qvec": quat_from_R(cam.R), "tvec": np.asarray(cam.t, f64), "camera_id": 1,
                       "name": "view%02d.png" % i, "point_ids": pids[ok], "xys": np.column_stack([u[ok], v[ok]])})
    return cams, images, pids, xyz
