"""Constructed fusion problems for the float64 known answers (tests/test_oracle_kat_fusion.py) and the
GPU edge tests (tests/test_gpu_fusion_edges.py).

A problem is a list of view dicts as tests/fusion_lib.py uses them. The scene is a plane or two
planes; cameras differ by non-symmetric rotations about two axes, non-zero t, fx != fy, cx != cy (one
problem has K[1] != 0). Column blocks of source depth, source normal, weak state and confidence bytes
put each rule on both sides of its cut. After construction the builder runs the float64 restatement
(tests/fusion_ref.py) and nudges the depth of any pixel that takes part in an unguarded decision
until none is left; it never looks at the oracle or the kernels.
"""
import functools
import os
import pickle

import numpy as np
from PIL import Image

import apd_abi as A
import fusion_ref as FR
import synth


def rot_xy(rx, ry):
    cx, sx, cy, sy = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    return Rx @ Ry  # not symmetric: R != R^T in every off-diagonal pair


def make_cam(W, H, fx, fy, cx, cy, skew, rx, ry, centre):
    cam = A.ApdCamera()
    K = np.array([fx, skew, cx, 0, fy, cy, 0, 0, 1], np.float32)
    R = rot_xy(rx, ry).astype(np.float32)
    t = (-(R.astype(np.float64) @ np.asarray(centre, np.float64))).astype(np.float32)
    c = (-(R.astype(np.float64).T @ t.astype(np.float64))).astype(np.float32)
    for k in range(9):
        cam.K[k] = float(K[k])
        cam.R[k] = float(R.reshape(-1)[k])
    for k in range(3):
        cam.t[k] = float(t[k])
        cam.c[k] = float(c[k])
    cam.width, cam.height = W, H
    cam.depth_min, cam.depth_max, cam.interval, cam.depth_num = 1.0, 20.0, 0.1, 192.0
    return cam


def plane_depth(cam, W, H, n, d0):
    """z-depth of the plane n.X = d0 along every pixel's ray, and the plane's normal in the camera
    frame (the reference compares normals in their own camera frames)."""
    K = np.array(list(cam.K), np.float64).reshape(3, 3)
    R = np.array(list(cam.R), np.float64).reshape(3, 3)
    t = np.array(list(cam.t), np.float64)
    C = -R.T @ t
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    rays = np.stack([xs, ys, np.ones_like(xs)], -1) @ np.linalg.inv(K).T  # camera frame, z = 1
    rw = rays @ R  # R^T ray
    s = (d0 - n @ C) / (rw @ n)
    nc = R @ n
    return s, np.broadcast_to(nc, (H, W, 3)).copy()


def blocks(W, values, width):
    """Per-column value: values[(c // width) % len(values)]."""
    return np.asarray(values, np.float64)[(np.arange(W) // width) % len(values)]


def rotate_normals(nrm, angle):
    """Tilt every normal by `angle` (per column) about the camera's x axis."""
    ca, sa = np.cos(angle)[None, :], np.sin(angle)[None, :]
    out = nrm.copy()
    out[..., 1] = ca * nrm[..., 1] - sa * nrm[..., 2]
    out[..., 2] = sa * nrm[..., 1] + ca * nrm[..., 2]
    return out


def _view(ref, srcs, cam, depth, normal, weak, conf, bgr):
    return dict(ref=ref, srcs=list(srcs), cam=cam, depth=np.ascontiguousarray(depth, np.float32),
                normal=np.ascontiguousarray(normal, np.float32), weak=np.ascontiguousarray(weak, np.uint8),
                conf=np.ascontiguousarray(conf, np.uint8), bgr=np.ascontiguousarray(bgr, np.uint8))


PLANE_N = np.array([0.10, -0.07, -1.0]) / np.linalg.norm([0.10, -0.07, -1.0])


def _std_views(W, H, nv, rng, focal, skew=0.0, rot=0.05, depth_err=(0.0,), tilt=(0.0,), block=4, two_planes=False,
               centres=None, sizes=None, baseline=0.22, aim=1.0):
    views = []
    for i in range(nv):
        w, h = (W, H) if sizes is None else sizes[i]
        centre = centres[i] if centres is not None else (baseline * (i - 0.5 * (nv - 1)), 0.4 * baseline * ((i % 3) - 0.9), 0.2 * baseline * i)
        f = focal[i % len(focal)] * w / W
        rx = rot * (((i * 7) % 5) - 2) * 0.6 + 0.01
        ry = aim * np.arctan2(centre[0], 5.0) + rot * (((i * 3) % 4) - 1.5)
        cam = make_cam(w, h, f, f * 1.1 + 2.0, w / 2 + 1.3, h / 2 - 0.7, skew, rx, ry, centre)
        d, nrm = plane_depth(cam, w, h, PLANE_N, PLANE_N @ np.array([0, 0, 5.0]))
        if two_planes:  # a nearer plane over the right part of the world: occlusions between views
            d2, _ = plane_depth(cam, w, h, PLANE_N, PLANE_N @ np.array([0, 0, 4.4]))
            K = np.array(list(cam.K)).reshape(3, 3)
            R = np.array(list(cam.R)).reshape(3, 3)
            ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
            Xw = (np.stack([xs, ys, np.ones_like(xs)], -1) @ np.linalg.inv(K).T * d2[..., None] -
                  np.array(list(cam.t))) @ R
            d = np.where(Xw[..., 0] > 0.35, d2, d)
        if i > 0:  # the perturbations live in the sources; each view shifts the pattern
            e = blocks(w, np.roll(np.asarray(depth_err), i), block)
            d = d * (1.0 + e)[None, :]
            nrm = rotate_normals(nrm, blocks(w, np.roll(np.asarray(tilt), 2 * i), block + 1))
        weak = rng.choice(np.array([0, 1, 2], np.uint8), size=(h, w), p=[0.45, 0.45, 0.10])
        conf = rng.integers(0x30, 0x50, (h, w)).astype(np.uint8)  # every 4-byte window is a positive finite float
        conf[:, (np.arange(w) // 5) % 3 == 0] = 0
        bgr = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
        views.append(_view(i, [j for j in range(nv) if j != i], cam, d, nrm, weak, conf, bgr))
    return views


def build_geom():
    """RunFusion's cuts: 32x24, 4 views, K[1] != 0, one source with a third of the reference's focal
    length (reprojection errors up to ~2.1 px), source depth off by 0 .. 3 %, normals tilted by
    0 .. 0.25 rad. Holes: depth 0, negative, NaN in the reference view."""
    rng = np.random.default_rng(101)
    v = _std_views(32, 24, 4, rng, focal=(96.0, 31.0, 80.0, 90.0), skew=0.8, rot=0.02, aim=0.0,
                   depth_err=(0.0, 0.0005, 0.004, 0.0088, 0.0112, 0.001, 0.03, 0.0),
                   tilt=(0.0, 0.02, 0.16, 0.0, 0.19, 0.04, 0.25), block=3)
    v[0]["depth"][3, 5] = np.nan
    v[0]["depth"][4, 7] = 0.0
    v[0]["depth"][5, 9] = -1.0
    v[1]["depth"][10:12, 12:16] = 0.0
    v[2]["depth"][6, 10:20] = -2.0
    v[1]["weak"][:, :] = 1
    v[2]["normal"][8:10, 5:9] = 0.0  # acosf of 0/0 is NaN: GetAngle then returns 0
    return v


def _pull_and_states(v, nmain, W, H, rng):
    """Reference depths pulled in front of the surface by 0 .. 3 % in column blocks (the 1 % margin).
    Sources are WEAK with STRONG and state-2 column bands; the middle third of the rows is mostly
    STRONG; in the top and bottom thirds all but the last two views are WEAK throughout, so the last
    view's WEAK pixels count three of them plus a banded fourth. Confidence bytes rise with the view
    index in overlapping ranges, with zero bands; reads from the last rows run past the buffer."""
    pull = blocks(W, (0.03, 0.006, 0.014, 0.03, 0.0094, 0.02), 2)
    cols = np.arange(W)
    for i in range(nmain):
        v[i]["depth"] = (v[i]["depth"] * (1.0 - np.roll(pull, 3 * i))[None, :]).astype(np.float32)
        st = np.zeros((H, W), np.uint8)
        st[:, (cols + 3 * i) % 8 == 0] = 1
        st[:, (cols + 3 * i) % 8 == 1] = 2
        st[H // 3:2 * H // 3, (cols + i) % 3 != 0] = 1
        if i < nmain - 2:
            st[: H // 3] = 0
            st[2 * H // 3:] = 0
        v[i]["weak"] = st
        conf = (0x30 + 6 * i + rng.integers(0, 12, (H, W))).astype(np.uint8)
        conf[:, (cols // 3 + i) % 7 == 0] = 0
        v[i]["conf"] = conf


def build_filter():
    """WeakVisFilter: 24x18, 6 views of two planes. Views 0-4 look at the scene; view 5 stands far to
    the side (view angles around 80 degrees)."""
    rng = np.random.default_rng(202)
    centres = [(-0.5, -0.08, 0.0), (-0.25, 0.01, 0.04), (0.0, 0.1, 0.08), (0.25, -0.08, 0.12), (0.5, 0.01, 0.16)]
    v = _std_views(24, 18, 5, rng, focal=(40.0, 43.0, 38.0), rot=0.04, two_planes=True, centres=centres)
    W, H = 24, 18
    _pull_and_states(v, 5, W, H, rng)
    side = make_cam(W, H, 20.0, 23.0, W / 2 + 0.4, H / 2 - 0.3, 0.0, 0.02, -1.25, (4.55, 0.3, 4.1))
    d, nrm = plane_depth(side, W, H, PLANE_N, PLANE_N @ np.array([0, 0, 5.0]))
    d = np.where(np.isfinite(d) & (d > 0) & (d < 50), d * 0.95, 0.0)
    v.append(_view(5, [0, 1], side, d, nrm, rng.choice(np.array([0, 1], np.uint8), size=(H, W)),
                   rng.integers(0x30, 0x50, (H, W)), rng.integers(0, 256, (H, W, 3))))
    for i in range(5):
        v[i]["srcs"] = [j for j in range(5) if j != i]
    return v


def build_counts():
    """WeakVisFilter's counters by design: 26x18, 6 views of one plane. Views 0-3 stand close together
    and carry per-column-block states; view 4 stands far to the side, all STRONG with a far depth, so
    it counts one STRONG occlusion wherever its view angle is <= 80 degrees (the angle crosses 80 near
    the middle column); view 5 is the WEAK reference, pulled 3 % in front of the surface (0.6 / 0.94 /
    1.4 % in some columns) and with its principal point 4 rows lower, so its last rows, whose
    confidence read runs past the buffer, meet source rows that read inside theirs. The sources'
    confidence bytes are lower than view 5's; their rows 9.. are zero, equal to view 5's zero tail."""
    rng = np.random.default_rng(606)
    W, H = 26, 18
    v = _std_views(W, H, 6, rng, focal=(40.0,), rot=0.01, baseline=0.03, aim=0.0)
    cols = np.arange(W)
    table = ["WWWW", "WWW2", "SSWW", "SWWW", "S2W2", "SWWW", "WWW2", "WWWW", "2222"]
    code = {"W": 0, "S": 1, "2": 2}
    for i in range(4):
        v[i]["weak"] = np.ascontiguousarray(np.broadcast_to(
            np.array([code[table[c // 3][i]] for c in cols], np.uint8)[None, :], (H, W))).copy()
        conf = rng.integers(0x30, 0x3c, (H, W)).astype(np.uint8)
        conf[9:] = 0
        v[i]["conf"] = conf
    side = make_cam(W, H, 10.0, 11.0, W / 2 + 0.4, H / 2 - 0.3, 0.0, 0.01, 1.397, (2.84, 0.05, 4.5))
    v[4] = _view(4, [0], side, np.full((H, W), 50.0), np.broadcast_to(np.array([0, 0, -1.0]), (H, W, 3)),
                 np.ones((H, W), np.uint8), np.zeros((H, W)), rng.integers(0, 256, (H, W, 3)))
    cam5 = v[5]["cam"]
    cam5.K[5] = float(np.float32(cam5.K[5] + 4.0))
    d, nrm = plane_depth(cam5, W, H, PLANE_N, PLANE_N @ np.array([0, 0, 5.0]))
    pull = blocks(W, (0.03, 0.03, 0.014, 0.03, 0.006, 0.03, 0.0094, 0.03), 2)
    st = np.zeros((H, W), np.uint8)
    st[:, cols % 7 == 3] = 1
    st[:, cols % 7 == 5] = 2
    v[5] = _view(5, [0, 1, 2, 3], cam5, d * (1.0 - pull)[None, :], nrm, st, rng.integers(0x44, 0x50, (H, W)),
                 v[5]["bgr"])
    for i in range(4):
        v[i]["srcs"] = [j for j in (0, 1, 2, 3, 5) if j != i]
    return v


def build_behind():
    """`proj_depth <= 0` is skipped in the filter only: 24x18, 3 views; view 2 stands between the
    cameras and the scene and looks back at them, so scene points project into its bounds with a
    negative depth, under a view angle far below 80 degrees."""
    rng = np.random.default_rng(505)
    v = _std_views(24, 18, 2, rng, focal=(40.0, 43.0), rot=0.02, two_planes=True, baseline=0.5, aim=0.0)
    W, H = 24, 18
    _pull_and_states(v, 2, W, H, rng)
    for i in range(2):
        v[i]["weak"][: H // 2] = np.where(v[i]["weak"][: H // 2] == 0, 1, 0)  # STRONG sources for WEAK pixels
    back = make_cam(W, H, 30.0, 33.0, W / 2 - 0.6, H / 2 + 0.2, 0.0, 0.03, np.pi + 0.04, (0.05, 0.02, 2.0))
    v.append(_view(2, [0], back, np.full((H, W), 3.0), np.broadcast_to(np.array([0, 0, -1.0]), (H, W, 3)),
                   np.ones((H, W), np.uint8), np.zeros((H, W)), rng.integers(0, 256, (H, W, 3))))
    v[0]["srcs"], v[1]["srcs"] = [1, 2], [0, 2]
    return v


def build_tat():
    """The TAT levels: 32x24, 5 views with long focal lengths (pixel rounding then moves the relative
    depth by ~1e-4, below the level spacing 1/3500), source depth off by 0 .. 0.2 % and normals tilted
    by 0 .. 0.35 rad in column blocks, holes that make the cost cache carry, also across row ends."""
    rng = np.random.default_rng(303)
    v = _std_views(32, 24, 5, rng, focal=(300.0, 280.0, 320.0, 150.0, 310.0), rot=0.02, baseline=0.04, aim=0.0,
                   depth_err=(0.0, 0.0002, 0.0007, 0.0, 0.0004, 0.001, 0.0001, 0.0013, 0.0, 0.0018, 0.00005),
                   tilt=(0.0, 0.10, 0.0, 0.16, 0.05, 0.21, 0.0, 0.27, 0.35), block=2)
    for i in range(1, 5):
        v[i]["depth"][:, 28 - i:] = 0.0          # holes up to the row end: the cache crosses rows
        v[i]["depth"][(3 * i) % 24, :] = -1.0
        v[i]["depth"][5 + i:9 + i, 8:11] = 0.0
    for r, c in ((7, 3), (9, 21), (13, 14), (15, 8), (18, 20), (20, 5), (11, 17), (16, 25)):
        v[0]["depth"][r, c] = np.nan  # processed (`NaN <= 0.0` is false): decided by the carried cache
    return v


def build_index():
    """imageIdToindexMap's quirks: 16x12, ids 10, 20, 30 and a second problem with id 20; view 0 lists
    an id that no problem has (reads as view 0: itself); view 1 lists itself and one id twice."""
    rng = np.random.default_rng(404)
    v = _std_views(16, 12, 4, rng, focal=(40.0, 44.0), rot=0.04, depth_err=(0.0, 0.003, 0.012), tilt=(0.0, 0.1, 0.2),
                   block=3)
    ids = [10, 20, 30, 20]
    for i, x in enumerate(ids):
        v[i]["ref"] = x
    v[0]["srcs"] = [20, 99, 30]
    v[1]["srcs"] = [20, 10, 10, 30]
    v[2]["srcs"] = [10, 20]
    v[3]["srcs"] = [30, 10]
    return v


# name -> (builder, [(variant, weak_filter)])
PROBLEMS = {
    "geom": (build_geom, [(0, False), (0, True)]),
    "filter": (build_filter, [(0, True), (1, True), (2, True)]),
    "counts": (build_counts, [(0, True), (2, True)]),
    "behind": (build_behind, [(0, True)]),
    "tat": (build_tat, [(1, False), (2, False)]),
    "index": (build_index, [(0, False), (1, False), (2, False)]),
}


def run_ref(views, runs, device=True):
    """The restatement's results for every (variant, weak_filter) of a problem, one shared scene.
    device: also take (and guard) every decision that the candidate and device tests compare."""
    sc = FR.Scene(views)
    g = FR.Guards()
    res = {run: FR.fuse(views, run[0], run[1], scene=sc, guards=g) for run in runs}
    for ref in range(len(views) if device else 0):  # every pair of views, itself included: the candidate tests use them all
        FR.candidates(sc, ref, list(range(len(views))), g)
        # and the mask-free decisions of the device entry points, over the view's own source list
        FR.decisions(sc, ref, [sc.index_of(s) for s in sc.srcs[ref]], g)
    return res, g


def repair(views, runs, rounds=40, device=True):
    """Nudges the depth of every pixel that takes part in an unguarded decision (the reference pixel;
    for a reprojection error, which does not depend on it, the source pixel), until the restatement
    reports none. Returns the number of rounds used."""
    for it in range(rounds):
        _res, g = run_ref(views, runs, device)
        if not g.bad:
            return it
        seen = set()
        for name, where, _val, _cut, _bound in g.bad:
            key = where[:3]
            if name.startswith("dist"):
                sv, sp = where[3], where[4]
                key = (sv,) + divmod(sp, views[sv]["depth"].shape[1])
            if key in seen:
                continue
            seen.add(key)
            vi, r, c = key
            d = views[vi]["depth"]
            if name.startswith("dist") and it >= 8:  # a short baseline: depth hardly moves the reprojection; make a hole
                d[r, c] = 0.0
                views[vi]["weak"][r, c] = 1
                continue
            d[r, c] = np.float32(np.float64(d[r, c]) * (1.0 + 2.3e-5 * (1 + it)))
    raise AssertionError(f"construction still has {len(g.bad)} unguarded decisions: {g.bad[:5]}")


@functools.lru_cache(maxsize=None)
def problem(name):
    build, runs = PROBLEMS[name]
    # APD_FUSION_KAT_CACHE: a folder in which tools/mutate_oracle.py keeps the constructed views between
    # its many pytest runs (construction is the restatement's alone, so mutants cannot change it)
    cache = os.environ.get("APD_FUSION_KAT_CACHE")
    path = os.path.join(cache, name + ".pkl") if cache else None
    if path and os.path.exists(path):
        with open(path, "rb") as fh:
            views = pickle.load(fh)
        res, g = run_ref(views, runs)
        assert not g.bad, g.bad[:5]
        return views, res, g
    views = build()
    for v in views:  # WeakVisFilter does not test the reference depth: at depth 0 the point is the camera
        v["weak"][v["depth"] == 0] = 1  # centre and the view angle is 0/0, so no WEAK pixel may be a hole
    repair(views, runs)
    res, g = run_ref(views, runs)
    assert not g.bad, g.bad[:5]
    if path:
        os.makedirs(cache, exist_ok=True)
        tmp = f"{path}.{os.getpid()}"
        with open(tmp, "wb") as fh:
            pickle.dump(views, fh)
        os.replace(tmp, path)
    return views, res, g


DATASETS = {0: "ETH3D", 1: "TaT_i", 2: "TaT_a"}


def close(got, ref, bound):
    """got (float32 result) within bound of ref (float64), NaN and infinities in the same places."""
    got = np.asarray(got, np.float64)
    fin = np.isfinite(ref)
    same = np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(got[~fin & ~np.isnan(ref)],
                                                                           ref[~fin & ~np.isnan(ref)])
    return same and bool(np.all(np.abs(got[fin] - ref[fin]) <= bound[fin]))


def check_oracle_fusion(views, variant, weak_filter, res):
    """oracle_fusion against the restatement's result `res`: accepted set and order (same count, every
    point within the bound of the restatement's point at the same position), float colours within
    the bound, PLY bytes where the float64 colour decides them, skip maps and TAT_A counts exactly."""
    import fusion_lib as FL
    xyz, col, skips, counts = FL.run_oracle(views, DATASETS[variant], weak_filter)
    assert len(xyz) == len(res["order"]), f"{len(xyz)} points, restatement {len(res['order'])}"
    if len(xyz):
        bad = [i for i in range(len(xyz)) if not close(xyz[i], res["xyz"][i], res["e_xyz"][i])]
        assert not bad, f"point {bad[0]} = {xyz[bad[0]]}, restatement {res['xyz'][bad[0]]} at {res['order'][bad[0]]}"
        assert close(col, res["col"], res["e_col"]), "float colours"
        byt, decided = FR.ply_colour_bytes(res["col"], res["e_col"])
        assert np.array_equal(col.astype(np.uint8)[decided], byt[decided]), "PLY colour bytes"
    for i, v in enumerate(views):
        assert np.array_equal(skips[i].reshape(-1), np.array(res["skips"][i], np.uint8)), f"skip map of view {i}"
    if variant == 2:
        assert list(counts) == res["skip_weak"]
    return xyz, col


# ------------------------------------------------------------------------------------------------
# a scan folder from views (for `apd --only_fuse`)
# ------------------------------------------------------------------------------------------------
def write_scan(folder, views, image_size=None):
    """images/, cams/, pair.txt and APD/<id>/*.bin for the given views. image_size (W, H): every
    colour image is stored at that one size (the tool refuses images of different sizes, like the
    reference's CheckImages) with the intrinsics scaled to it; loading then resizes image and camera
    to each view's own depth-map size (RescaleImageAndCamera)."""
    os.makedirs(os.path.join(folder, "images"), exist_ok=True)
    os.makedirs(os.path.join(folder, "cams"), exist_ok=True)
    for v in views:
        name = f"{v['ref']:08d}"
        img = Image.fromarray(np.ascontiguousarray(v["bgr"][..., ::-1]), "RGB")
        h, w = v["depth"].shape
        sx, sy = (1.0, 1.0) if image_size is None else (image_size[0] / w, image_size[1] / h)
        if image_size is not None:
            img = img.resize(image_size, Image.NEAREST)
        img.save(os.path.join(folder, "images", name + ".png"))
        cam = v["cam"]
        with open(os.path.join(folder, "cams", name + "_cam.txt"), "w") as fh:
            fh.write("extrinsic\n")
            for r in range(3):
                fh.write(" ".join(repr(float(cam.R[3 * r + k])) for k in range(3)) + " " + repr(float(cam.t[r])) + "\n")
            fh.write("0.0 0.0 0.0 1.0\n\nintrinsic\n")
            for r in range(3):
                fh.write(" ".join(repr(float(cam.K[3 * r + k]) * (sx, sy, 1.0)[r]) for k in range(3)) + "\n")
            fh.write(f"\n{float(cam.depth_min)!r} {float(cam.interval)!r} {float(cam.depth_num)!r} {float(cam.depth_max)!r}\n")
        d = os.path.join(folder, "APD", name)
        os.makedirs(d, exist_ok=True)
        synth.write_bin_mat(os.path.join(d, "depths.bin"), v["depth"])
        synth.write_bin_mat(os.path.join(d, "normals.bin"), v["normal"])
        synth.write_bin_mat(os.path.join(d, "weak.bin"), v["weak"])
        synth.write_bin_mat(os.path.join(d, "confidence.bin"), v["conf"])
    with open(os.path.join(folder, "pair.txt"), "w") as fh:
        fh.write(f"{len(views)}\n")
        for v in views:
            fh.write(f"{v['ref']}\n{len(v['srcs'])} " + " ".join(f"{s} 1.0" for s in v["srcs"]) + "\n")


# ------------------------------------------------------------------------------------------------
# small scans for the branches of the host commit that the random scans never reach
# (tests/test_gpu_fusion_edges.py). RUNS: the (variant, weak_filter) pairs for which the scan is
# repaired to zero unguarded decisions, so that the oracle can also be held to the restatement.
# ------------------------------------------------------------------------------------------------
def _edge_views(W, H, nv, seed, sizes=None, focal=(120.0, 110.0, 126.0), baseline=0.04):
    rng = np.random.default_rng(seed)
    v = _std_views(W, H, nv, rng, focal=focal, rot=0.01, baseline=baseline, aim=0.0,
                   depth_err=(0.0, 0.0003, 0.004, 0.0, 0.012, 0.0001), tilt=(0.0, 0.05, 0.0, 0.12, 0.2), block=3,
                   sizes=sizes)
    for i, x in enumerate(v):
        h, w = x["depth"].shape
        x["depth"][rng.random((h, w)) < 0.04] = 0.0
        x["depth"][rng.random((h, w)) < 0.01] = -1.0
    return v


def scan_self_source():
    v = _edge_views(32, 24, 3, 11)
    v[1]["srcs"] = [0, 1, 2]
    return v


def scan_missing_id():
    """Id 7 is in no problem: it reads as view 0, a self-source for view 0 and a plain one for view 2."""
    v = _edge_views(32, 24, 3, 12)
    v[0]["srcs"] = [1, 7]
    v[2]["srcs"] = [1, 7]
    return v


def scan_duplicate_source():
    v = _edge_views(32, 24, 3, 13)
    v[1]["srcs"] = [0, 2, 2, 0]
    v[0]["srcs"] = [1, 1, 2]
    return v


def scan_three_sizes():
    return _edge_views(48, 36, 3, 14, sizes=[(48, 36), (40, 30), (33, 25)])


def scan_tiny():
    """A 15x9 image (under one 256-lane block), a 64x1 image (one row) and a 20x12 one."""
    return _edge_views(20, 12, 3, 15, sizes=[(15, 9), (64, 1), (20, 12)], focal=(60.0,), baseline=0.02)


def scan_one_source():
    v = _edge_views(32, 24, 2, 16)
    return v


def scan_max_sources():
    """33 views of 16x12; view 0 lists all 32 others (APD_MAX_IMAGES sources), the rest two each."""
    v = _edge_views(16, 12, 33, 17, focal=(60.0, 64.0), baseline=0.004)
    for i in range(1, 33):
        v[i]["srcs"] = [(i + 1) % 33, (i + 7) % 33]
    return v


def scan_carry():
    """64x96 (96 rows: 64 row chunks of the host commit); view 2 has depth only in its top fifth, so
    for every later pixel of view 0 its cost comes from the carried cache."""
    v = _edge_views(64, 96, 3, 18, focal=(400.0, 380.0, 410.0), baseline=0.02)
    v[2]["depth"][19:] = 0.0
    v[2]["depth"][18, 40:] = np.float32(v[2]["depth"][18, 39])  # the last usable pixels agree with the surface
    return v


def scan_nonfinite():
    v = _edge_views(40, 30, 4, 19)
    rng = np.random.default_rng(20)
    for x in v:
        h, w = x["depth"].shape
        m = rng.random((h, w))
        x["depth"][m < 0.03] = np.nan
        x["depth"][(m >= 0.03) & (m < 0.05)] = np.inf
        x["depth"][(m >= 0.05) & (m < 0.07)] = -np.inf
        x["normal"][rng.random((h, w)) < 0.1] = 0.0
    v[3]["normal"][:] = 0.0
    return v


ALL3 = [(0, True), (1, True), (2, True)]
EDGE_SCANS = {
    "self_source": (scan_self_source, ALL3),
    "missing_id": (scan_missing_id, ALL3),
    "duplicate_source": (scan_duplicate_source, ALL3),
    "three_sizes": (scan_three_sizes, None, (96, 72)),
    "tiny": (scan_tiny, None, (64, 36)),
    "one_source": (scan_one_source, None),
    "max_sources": (scan_max_sources, None),
    "carry": (scan_carry, [(1, False), (2, False)]),
    "nonfinite": (scan_nonfinite, None),
}


def prepare_scan(folder, name, hl):
    """Writes edge scan `name`, loads it back as the tool does (tests/fusion_lib.load_views) and, for a
    scan with RUNS, repairs the loaded depths until the restatement has no unguarded decision and
    writes them again. Returns (loaded views, restatement results or None)."""
    import fusion_lib as FL
    build, runs = EDGE_SCANS[name][:2]
    views = build()
    if runs:
        for v in views:
            v["weak"][v["depth"] == 0] = 1
    write_scan(folder, views, *EDGE_SCANS[name][2:])
    loaded = FL.load_views(folder, hl)
    if not runs:
        return loaded, None
    for v in loaded:
        v["depth"] = np.ascontiguousarray(v["depth"], np.float32).copy()
        v["weak"] = np.ascontiguousarray(v["weak"], np.uint8).copy()
    repair(loaded, runs, device=False)
    for v in loaded:
        synth.write_bin_mat(os.path.join(folder, "APD", f"{v['ref']:08d}", "depths.bin"), v["depth"])
        synth.write_bin_mat(os.path.join(folder, "APD", f"{v['ref']:08d}", "weak.bin"), v["weak"])
    res, g = run_ref(loaded, runs, device=False)
    assert not g.bad, g.bad[:5]
    return loaded, res
