"""apd_eval_free_gap / apd_eval_voxel_scores / apd_eval_cube_cameras, cloud_metrics_scanners and
`apd_eval --gt_mlp` on the GPU against the literal numpy restatement of the contract in
tests/protocol_lib.py: floats bit for bit, integers equal, no tolerances anywhere. The counts quoted
in the assertions come from that numpy reference on the draws below."""
import ctypes as C
import json
import subprocess

import numpy as np
import pytest

import apd_abi as A
from eval_lib import APD_EVAL, brute, f32, ply_apd_layout, ply_gt_layout, same_bits
from protocol_lib import (NEG_INF, ROOM_ORIGINS, classes_ref, colours_ref, cube_cameras_ref, free_gap_ref, in_view_ref,
                          mlp_text, protocol_ref, read_ply_xyz_rgb, room_scene, score_of, scores_equal, to_world_ref,
                          voxel_scores_ref)
from render_lib import make_cam, render_ref, two_wall_camera, two_wall_cloud

pytestmark = pytest.mark.gpu

TOLS = A.ETH3D_TOLERANCES
ROOM = dict(voxel=0.25, cube_size=48, max_dist=0.5)
EINVAL = -1


@pytest.fixture(scope="module")
def lib():
    return A.load_library()


@pytest.fixture(scope="module")
def eng(lib):
    e = A.EvalEngine(0, lib)
    yield e
    e.close()


@pytest.fixture(scope="module")
def room():
    """The room scene with its reference results at splat 0 and 1 (computed once, never modified)."""
    rec, scans, parts = room_scene()
    ref = {s: protocol_ref(rec, scans, TOLS, ROOM["voxel"], ROOM["cube_size"], s, ROOM["max_dist"], brute)
           for s in (0, 1)}
    return rec, scans, parts, ref


def simple_cam(W, H, f=None, t=(0, 0, 0)):
    f = 0.8 * max(W, H) if f is None else f
    return make_cam([[f, 0, W / 2 - 0.5], [0, f, H / 2 - 0.5], [0, 0, 1]], np.eye(3), t, W, H)


def box_cloud(rng, n):
    return np.column_stack([rng.uniform(-1.5, 1.5, (n, 2)), rng.uniform(1, 4, n)]).astype(f32)


def check_gap(eng, cloud, cams, maps):
    got = eng.free_gap(cloud, cams, maps)
    want = free_gap_ref(cloud, cams, maps)
    assert got.dtype == f32 and got.shape == want.shape
    assert same_bits(got, want), int((got.view(np.uint32) != want.view(np.uint32)).sum())
    return want


def check_scores(eng, xyz, voxel, dist, gap, tols):
    got = eng.voxel_scores(xyz, voxel, dist, gap, tols)
    want = voxel_scores_ref(xyz, voxel, dist, gap, tols)
    assert all(got[k].dtype == np.int64 and len(got[k]) == len(np.atleast_1d(tols)) for k in want)
    assert scores_equal(got, want), (got, want)
    assert got["score"] == score_of(want["ratio_sum"], want["voxels"])
    return want


# ---- 1. the room ------------------------------------------------------------------------------------

def test_room_is_not_vacuous(room):
    rec, scans, parts, ref = room
    a = ref[1]["accuracy"]
    n = len(ref[1]["R"])
    assert n == 5800 and len(ref[1]["G"]) == 13500
    k = TOLS.index(0.1)
    assert (a["good"][k], a["bad"][k], n - a["good"][k] - a["bad"][k]) == (3160, 1382, 1258)
    for k in (TOLS.index(0.05), TOLS.index(0.1), TOLS.index(0.2)):  # the middle tolerances
        g, b = a["good"][k], a["bad"][k]
        assert min(g, b, n - g - b) >= 0.1 * n
        assert abs(score_of(a["ratio_sum"], a["voxels"])[k] - g / (g + b)) >= 0.01  # voxel-averaged != plain
    # the parts behave as built: walls good, floaters in observed free space, the shell behind the walls
    good, bad = classes_ref(ref[1]["accuracy_dist"], ref[1]["gap"], 0.1)
    count = lambda s: (int(good[s].sum()), int(bad[s].sum()), int((~good[s] & ~bad[s]).sum()))
    assert count(parts["wall"]) == (2950, 1, 49) and count(parts["floater"]) == (12, 1179, 9)
    assert count(parts["shell"]) == (0, 0, 1200) and count(parts["box"]) == (198, 202, 0)
    assert ref[0]["accuracy"]["bad"] != ref[1]["accuracy"]["bad"]  # the footprint matters
    assert len(set(a["voxels"])) > 1  # voxels whose points are all unobserved drop out per tolerance


@pytest.mark.parametrize("splat", [0, 1])
def test_room_scene(eng, room, splat):
    rec, scans, parts, ref = room
    r = ref[splat]
    cams, maps = [], []
    for pts, origin in scans:
        faces = A.cube_cameras(origin, ROOM["cube_size"])
        got = eng.render_depth(pts, faces, splat)
        assert all(same_bits(m, render_ref(pts, c, splat)[0]) for m, c in zip(got, faces))
        cams += faces
        maps += got
    gap = eng.free_gap(rec, cams, maps)  # all twelve faces at once: crosses the chunk of 8
    assert same_bits(gap, r["gap"])
    assert scores_equal(eng.voxel_scores(rec, ROOM["voxel"], r["accuracy_dist"], gap, TOLS), r["accuracy"])
    assert scores_equal(eng.voxel_scores(r["G"], ROOM["voxel"], r["completeness_dist"], None, TOLS), r["completeness"])
    m = A.cloud_metrics_scanners(rec, scans, TOLS, ROOM["voxel"], ROOM["cube_size"], splat, engine=eng)
    assert m["max_dist"] == 0.5 and m["rec"]["points"] == 5800 and m["gt"]["points"] == 13500
    assert same_bits(m["accuracy_gap"], r["gap"]) and same_bits(m["accuracy_dist"], r["accuracy_dist"])
    assert same_bits(m["completeness_dist"], r["completeness_dist"])
    for side in ("accuracy", "completeness"):
        want = r[side]
        assert all(m[side][k] == want[k] for k in want), side
        assert m[side]["score"] == score_of(want["ratio_sum"], want["voxels"])
        assert m[side]["unobserved"] == [m[side]["points"] - g - b for g, b in zip(want["good"], want["bad"])]
    assert m["completeness"]["unobserved"] == [0] * len(TOLS)
    a, c = m["accuracy"]["score"], m["completeness"]["score"]
    assert m["f1"] == [2 * x * y / (x + y) if x + y > 0 else 0.0 for x, y in zip(a, c)] and 0 < m["f1"][3] < 1


# ---- 2. free_gap ------------------------------------------------------------------------------------

def test_free_gap_map_entries_and_dropped_points(eng):
    cam = two_wall_camera()
    cloud, parts = two_wall_cloud()  # points behind the camera, outside the image, non-finite rows
    dep = render_ref(cloud, cam, 2)[0].copy()
    dep[::3, ::2] = 0
    dep[1::3, 1::2] = np.nan
    dep[2::3, ::5] = f32(-4.0)
    dep[::7, 1::4] = np.inf
    dep[6, 8] = -np.inf
    want = check_gap(eng, cloud, [cam], [dep])
    assert (want[parts["behind"]] == NEG_INF).all() and (want[parts["bad"]] == NEG_INF).all()
    assert (want == np.inf).sum() > 50 and (want == NEG_INF).sum() > 1000 and np.isfinite(want).sum() > 500
    assert (want[np.isfinite(want)] < 0).any() and (want[np.isfinite(want)] >= 0).any()


def test_free_gap_against_the_own_map_is_not_positive(eng):
    """A map rendered from the cloud itself holds, at a point's own pixel, the depth of that point or
    of a nearer one: gap = zb - d is finite and <= 0 for every covered point, and +0 for the points
    that won their pixel. (No point of a cloud lies in the free space its own z-buffer proves.)"""
    cam = two_wall_camera()
    cloud, parts = two_wall_cloud()
    for splat in (0, 2):
        dep, idx = eng.render_depth(cloud, [cam], splat, want_index=True)[0]
        want = check_gap(eng, cloud, [cam], [dep])
        inb, _, u, v = in_view_ref(cloud, cam)
        assert np.isfinite(want[inb]).all() and (want[inb] <= 0).all() and (want[~inb] == NEG_INF).all()
        assert (want[inb] < 0).any()
        j = np.flatnonzero(inb)
        winners = j[idx[v[j], u[j]] == j]  # the points that hold their own centre pixel
        assert len(winners) > 50 and (want[winners] == 0).all()
        assert not np.signbit(want[winners]).any()  # equal operands give +0


def test_free_gap_on_the_face_seams(eng):
    """Points within an ulp of a seam of the cube map: the faces each lands in are the reference's."""
    origin = np.array([0.5, 0.3, -0.4], f32)
    rng = np.random.default_rng(2)
    base = rng.uniform(0.5, 3, 400).astype(f32)
    other = rng.uniform(-0.4, 0.4, 400).astype(f32) * base
    pts = []
    for step in (-1, 0, 1):  # |a| = |b| exactly, one ulp below, one ulp above
        b = base.copy()
        for _ in range(abs(step)):
            b = np.nextafter(b, f32(np.inf) if step > 0 else f32(0))
        for sa in (1, -1):
            for sb in (1, -1):
                for axes in ((0, 1, 2), (0, 2, 1), (1, 2, 0)):
                    p = np.zeros((400, 3), f32)
                    p[:, axes[0]], p[:, axes[1]], p[:, axes[2]] = sa * base, sb * b, other
                    pts.append(p)
    rel = np.concatenate(pts)
    for size in (8, 48):
        for centre in (np.zeros(3, f32), origin):
            cloud = (rel + centre).astype(f32)
            cams = A.cube_cameras(centre, size)
            ones = np.full((size, size), 100, f32)
            landed = np.stack([np.isfinite(check_gap(eng, cloud, [c], [ones])) for c in cams])
            assert np.array_equal(landed, np.stack([in_view_ref(cloud, c)[0] for c in cams]))
            hits = landed.sum(axis=0)
            # a point exactly on a seam projects to -0.5 in one face (kept: pixel 0) and to size - 0.5 in
            # the other (pixel `size`: outside), so besides one and two faces some seam points land in none
            assert (hits == 0).sum() > 500 and (hits == 2).sum() > 1000 and (hits == 1).sum() > 1000
            check_gap(eng, cloud, cams, [ones] * 6)


@pytest.mark.parametrize("views", [0, 1, 6, 19])
def test_free_gap_view_counts(eng, views):
    rng = np.random.default_rng(views)
    cloud = box_cloud(rng, 1500)
    cams = [simple_cam(20 + 3 * v, 31 - v, t=(0.1 * (v % 5) - 0.2, 0.05 * (v % 3), 0.02 * v)) for v in range(views)]
    maps = [np.where(rng.uniform(size=(c.height, c.width)) < 0.2, 0, rng.uniform(1, 4, (c.height, c.width))).astype(f32)
            for c in cams]
    want = check_gap(eng, cloud, cams, maps)
    if views == 0:
        assert (want == NEG_INF).all()
    else:
        assert np.isfinite(want).sum() > 300 and (want == NEG_INF).sum() > 30
    if views == 19:  # the maximum really comes from views of every chunk
        best = np.argmax(np.stack([free_gap_ref(cloud, [c], [m]) for c, m in zip(cams, maps)]), axis=0)
        assert (best[np.isfinite(want)] < 8).any() and (best[np.isfinite(want)] >= 16).any()


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257])
def test_free_gap_sizes(eng, n):
    rng = np.random.default_rng(100 + n)
    cloud = box_cloud(rng, n)
    cams = [simple_cam(33, 21), simple_cam(16, 40, t=(0.2, 0, 0.3))]
    maps = [rng.uniform(1, 4, (c.height, c.width)).astype(f32) for c in cams]
    want = check_gap(eng, cloud, cams, maps)
    assert want.shape == (n,)
    perm = rng.permutation(n)
    assert same_bits(eng.free_gap(cloud[perm], cams, maps), want[perm])


def test_free_gap_device_pointers(eng, room):
    import torch
    rec, scans, parts, ref = room
    cams = A.cube_cameras(scans[0][1], 48) + A.cube_cameras(scans[1][1], 48)
    maps = [render_ref(scans[i // 6][0], c, 1)[0] for i, c in enumerate(cams)]
    got = eng.free_gap(torch.from_numpy(rec).cuda(), cams, [torch.from_numpy(m).cuda() for m in maps])
    assert got.is_cuda and same_bits(got.cpu().numpy(), ref[1]["gap"])
    mixed = eng.free_gap(rec, cams, [torch.from_numpy(m).cuda() if i % 2 else m for i, m in enumerate(maps)])
    assert same_bits(mixed, ref[1]["gap"])


# ---- 3. cube cameras ----------------------------------------------------------------------------------

@pytest.mark.parametrize("size,two", [(8, 2326), (48, 456)])
def test_cube_faces_on_the_device(eng, size, two):
    rng = np.random.default_rng(size)
    origin = np.array([0.5, 0.3, -0.4], f32)
    pts = (origin + rng.normal(0, 1, (20000, 3)) * rng.uniform(0.5, 3, (20000, 1))).astype(f32)
    cams = A.cube_cameras(origin, size)
    assert all(bytes(c) == bytes(r) for c, r in zip(cams, cube_cameras_ref(origin, size)))
    ones = np.full((size, size), 100, f32)
    landed = np.stack([np.isfinite(eng.free_gap(pts, [c], [ones])) for c in cams])
    assert np.array_equal(landed, np.stack([in_view_ref(pts, c)[0] for c in cams]))
    hits = landed.sum(axis=0)
    assert hits.min() >= 1 and int((hits > 1).sum()) == two
    # the cloud against its own cube map: every point is covered, by itself or by something nearer
    for splat in (0, 1):
        gap = check_gap(eng, pts, cams, eng.render_depth(pts, cams, splat))
        assert np.isfinite(gap).all() and (gap <= 0).all() and (gap == 0).any() and (gap < 0).any()


# ---- 4. voxel_scores ------------------------------------------------------------------------------------

def draw_dist_gap(rng, n):
    dist = rng.uniform(0, 0.3, n).astype(f32)
    gap = rng.uniform(-0.3, 0.3, n).astype(f32)
    return dist, gap


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_scores_one_voxel(eng, n):
    rng = np.random.default_rng(n)
    xyz = rng.uniform(0.1, 0.9, (n, 3)).astype(f32)
    dist, gap = draw_dist_gap(rng, n)
    want = check_scores(eng, xyz, 1.0, dist, gap, TOLS)
    assert max(want["voxels"]) == 1
    check_scores(eng, xyz, 1.0, dist, None, TOLS)


def runs_cloud(rng, where):
    """2000 single-point voxels on the x axis with three long runs (300, 64 and 129 points) whose
    voxels sort first / in the middle / last (the key's major axis is x)."""
    x0 = {"first": (-5, -4, -3), "middle": (700, 900, 1100), "last": (2100, 2200, 2300), "mixed": (-5, 900, 2300)}[where]
    single = np.column_stack([np.arange(2000) + 0.5, rng.uniform(0, 1, (2000, 2))])
    runs = [np.column_stack([rng.uniform(x + 0.1, x + 0.9, m), rng.uniform(0, 1, (m, 2))])
            for x, m in zip(x0, (300, 64, 129))]
    xyz = np.concatenate([single] + runs).astype(f32)
    return xyz[rng.permutation(len(xyz))]


@pytest.mark.parametrize("where", ["first", "middle", "last", "mixed"])
def test_scores_long_and_short_runs(eng, where):
    rng = np.random.default_rng(7)
    xyz = runs_cloud(rng, where)
    dist, gap = draw_dist_gap(rng, len(xyz))
    want = check_scores(eng, xyz, 1.0, dist, gap, TOLS)
    assert 1500 < max(want["voxels"]) <= 2003 and len(set(want["voxels"])) > 1
    perm = rng.permutation(len(xyz))
    assert scores_equal(eng.voxel_scores(xyz[perm], 1.0, dist[perm], gap[perm], TOLS), want)


def test_scores_single_point_voxels(eng):
    rng = np.random.default_rng(8)
    g = np.stack(np.meshgrid(np.arange(20), np.arange(25), np.arange(10), indexing="ij"), -1).reshape(-1, 3)
    xyz = ((g - [10, 12, 5]) * 0.5 + rng.uniform(0.05, 0.45, (5000, 3))).astype(f32)  # negative coordinates too
    dist, gap = draw_dist_gap(rng, 5000)
    want = check_scores(eng, xyz, 0.5, dist, gap, TOLS)
    k = TOLS.index(0.1)
    assert want["voxels"][k] == want["good"][k] + want["bad"][k] < 5000
    assert want["ratio_sum"][k] == want["good"][k] << 32


def test_scores_exact_ratios(eng):
    """a = b gives exactly 2^31; a = 1, b = 2 gives 1431655765 (rounded down); all-unobserved voxels
    do not count."""
    xyz = np.array([[0.5, 0, 0]] * 6 + [[1.5, 0, 0]] * 3 + [[2.5, 0, 0]] * 4 + [[3.5, 0, 0]] * 2, f32)
    dist = np.array([0.01] * 3 + [1.0] * 3 + [0.01, 1, 1] + [1.0] * 4 + [0.01, 0.01], f32)
    gap = np.array([1.0] * 6 + [1.0] * 3 + [-np.inf, 0.0, 0.05, -1.0] + [1.0, 1.0], f32)
    want = check_scores(eng, xyz, 1.0, dist, gap, [0.05])
    assert want == {"good": [6], "bad": [5], "ratio_sum": [(1 << 31) + 1431655765 + (1 << 32)], "voxels": [3]}
    got = eng.voxel_scores(xyz[6:9], 1.0, dist[6:9], gap[6:9], [0.05])
    assert int(got["ratio_sum"][0]) == 1431655765 == (1 << 32) // 3 and got["score"] == [1431655765 / 2 ** 32]
    # at tolerance 2 everything is good; at 0.02 the third voxel's gap 0.05 counts as bad
    want = check_scores(eng, xyz, 1.0, dist, gap, [2.0, 0.02, 0.05])
    assert want["voxels"] == [4, 4, 3] and want["bad"] == [0, 6, 5]


def test_scores_voxel_faces_and_signs(eng):
    """Coordinates exactly on voxel faces, on both sides of zero, and -0.0: floorf(x / voxel)."""
    v = np.array([-0.75, -0.5, -0.25, -0.0, 0.0, 0.25, 0.5], f32)
    near = np.concatenate([v, np.nextafter(v, f32(-np.inf)), np.nextafter(v, f32(np.inf))])
    rng = np.random.default_rng(9)
    xyz = np.stack([rng.choice(near, 3000), rng.choice(near, 3000), rng.choice(near[:7], 3000)], 1).astype(f32)
    dist, gap = draw_dist_gap(rng, 3000)
    for voxel in (0.25, 0.1):
        want = check_scores(eng, xyz, voxel, dist, gap, TOLS)
        assert 30 < max(want["voxels"]) < 3000


def test_scores_non_finite_inputs(eng):
    rng = np.random.default_rng(10)
    xyz = rng.uniform(-1, 1, (4000, 3)).astype(f32)
    xyz[::17, 0], xyz[5::29, 1], xyz[7::31, 2] = np.nan, np.inf, -np.inf
    dist, gap = draw_dist_gap(rng, 4000)
    dist[::5], dist[1::7] = np.inf, np.nan
    gap[::3], gap[1::11], gap[2::13] = -np.inf, np.inf, np.nan
    fin = int(np.isfinite(xyz).all(axis=1).sum())
    for g in (gap, None):
        want = check_scores(eng, xyz, 0.2, dist, g, TOLS)
        assert all(a + b <= fin for a, b in zip(want["good"], want["bad"]))
    assert [a + b for a, b in zip(want["good"], want["bad"])] == [fin] * len(TOLS)  # gap = None: good or bad
    none = np.full((50, 3), np.nan, f32)
    assert check_scores(eng, none, 0.2, dist[:50], gap[:50], TOLS)["voxels"] == [0] * len(TOLS)


@pytest.mark.parametrize("num_tol", [0, 1, 6, 40])
def test_scores_tolerance_counts(eng, num_tol):
    rng = np.random.default_rng(num_tol)
    xyz = rng.uniform(-1, 1, (3000, 3)).astype(f32)
    dist, gap = draw_dist_gap(rng, 3000)
    tols = rng.uniform(0, 0.3, num_tol).astype(f32)  # unsorted
    if num_tol >= 6:
        tols[3], tols[-1] = tols[0], 0.0  # repeated, and zero
    want = check_scores(eng, xyz, 0.2, dist, gap, tols)
    if num_tol >= 6:
        assert all(want[k][3] == want[k][0] for k in want) and want["good"][-1] == 0


def test_scores_empty_cloud(eng):
    got = eng.voxel_scores(np.zeros((0, 3), f32), 0.1, np.zeros(0, f32), None, TOLS)
    assert all(got[k].tolist() == [0] * len(TOLS) for k in ("good", "bad", "ratio_sum", "voxels"))
    assert got["score"] == [0.0] * len(TOLS)
    assert eng.free_gap(np.zeros((0, 3), f32), [], []).shape == (0,)


def test_scores_do_not_disturb_the_other_calls(eng):
    rng = np.random.default_rng(12)
    target = rng.uniform(-1, 1, (3000, 3)).astype(f32)
    query = rng.uniform(-1, 1, (2500, 3)).astype(f32)
    xyz = rng.uniform(-1, 1, (3500, 3)).astype(f32)
    dist, gap = draw_dist_gap(rng, 3500)
    cam = simple_cam(40, 30)
    want_d = brute(query, target, 0.2)
    eng.set_target(target)
    first = check_scores(eng, xyz, 0.2, dist, gap, TOLS)
    assert same_bits(eng.distances(query, 0.2)[0], want_d)  # the target survived voxel_scores
    keep = eng.voxel_downsample(xyz, 0.2)
    dep = eng.render_depth(xyz + [0, 0, 3], [cam], 1)[0]
    g1 = check_gap(eng, xyz + [0, 0, 3.5], [cam], [dep])
    assert scores_equal(eng.voxel_scores(xyz, 0.2, dist, gap, TOLS), first)
    assert same_bits(eng.distances(query, 0.2)[0], want_d) and np.array_equal(eng.voxel_downsample(xyz, 0.2), keep)
    assert same_bits(eng.free_gap(xyz + [0, 0, 3.5], [cam], [dep]), g1)
    t = eng.protocol_timing()
    assert t["free_gap_ms"] > 0 and t["scores_ms"] > 0


def test_scores_device_pointers(eng):
    import torch
    rng = np.random.default_rng(13)
    xyz = rng.uniform(-1, 1, (3000, 3)).astype(f32)
    dist, gap = draw_dist_gap(rng, 3000)
    want = voxel_scores_ref(xyz, 0.2, dist, gap, TOLS)
    dev = lambda a: torch.from_numpy(a).cuda()
    got = eng.voxel_scores(dev(xyz), 0.2, dev(dist), dev(gap), TOLS)
    assert all(got[k].is_cuda and got[k].dtype == torch.int64 for k in want)
    assert scores_equal({k: got[k].cpu().numpy() for k in want}, want) and got["score"] == score_of(want["ratio_sum"], want["voxels"])
    assert scores_equal(eng.voxel_scores(xyz, 0.2, dev(dist), gap, TOLS), want)  # mixed host and device
    got = eng.voxel_scores(dev(xyz), 0.2, dev(dist), None, TOLS)
    assert scores_equal({k: got[k].cpu().numpy() for k in want}, voxel_scores_ref(xyz, 0.2, dist, None, TOLS))


def test_scores_agree_with_distances_within(eng):
    rng = np.random.default_rng(14)
    target = rng.uniform(1, 3, (3000, 3)).astype(f32)
    query = rng.uniform(1, 3, (2777, 3)).astype(f32)
    query[::50] = np.nan
    eng.set_target(target)
    dist, within = eng.distances(query, 0.5, TOLS)
    got = eng.voxel_scores(query, 1000.0, dist, None, TOLS)
    fin = int(np.isfinite(query).all(axis=1).sum())
    assert got["good"].tolist() == within.tolist() and got["voxels"].tolist() == [1] * len(TOLS)
    assert got["bad"].tolist() == [fin - int(w) for w in within]
    assert got["ratio_sum"].tolist() == [(int(w) << 32) // fin for w in within]


# ---- 5. status codes ------------------------------------------------------------------------------------

def test_status_codes(lib):
    e = A.EvalEngine(0, lib)  # a fresh context: neither call needs a target
    try:
        ctx = e.ctx
        xyz = np.random.default_rng(0).uniform(-1, 1, (10, 3)).astype(f32)
        xyz[:, 2] += 3
        cam = simple_cam(8, 6)
        cams = (A.ApdCamera * 2)(cam, cam)
        dep = np.ones((6, 8), f32)
        maps = (C.c_void_p * 2)(dep.ctypes.data, dep.ctypes.data)
        gap = np.zeros(10, f32)
        X, G = xyz.ctypes.data, gap.ctypes.data
        gapf = lib.apd_eval_free_gap
        assert gapf(ctx, 10, X, 2, cams, maps, G) == 0 and np.isfinite(gap).any()
        assert gapf(ctx, 0, None, 0, None, None, None) == 0
        assert gapf(ctx, -1, X, 2, cams, maps, G) == EINVAL and gapf(ctx, 2 ** 31, X, 2, cams, maps, G) == EINVAL
        assert gapf(ctx, 10, None, 2, cams, maps, G) == EINVAL
        assert gapf(ctx, 10, X, -1, cams, maps, G) == EINVAL and gapf(ctx, 10, X, 2, None, maps, G) == EINVAL
        assert gapf(ctx, 10, X, 2, cams, None, G) == EINVAL
        assert gapf(ctx, 10, X, 2, cams, (C.c_void_p * 2)(dep.ctypes.data, None), G) == EINVAL
        assert gapf(ctx, 10, X, 2, cams, maps, None) == EINVAL
        for w, h in ((0, 6), (8, 0), (-1, 6), (2 ** 15, 2 ** 14)):
            bad = (A.ApdCamera * 2)(cam, simple_cam(8, 6))
            bad[1].width, bad[1].height = w, h
            assert gapf(ctx, 10, X, 2, bad, maps, G) == EINVAL
        assert b"apd_eval_free_gap" in lib.apd_eval_last_error(ctx)

        dist = np.full(10, 0.01, f32)
        tol = np.array([0.1, 0.2], f32)
        outs = [np.zeros(2, np.int64) for _ in range(4)]
        D, T, O = dist.ctypes.data, tol.ctypes.data, [o.ctypes.data for o in outs]
        sc = lib.apd_eval_voxel_scores
        assert sc(ctx, 10, X, 0.5, D, None, 2, T, *O) == 0 and outs[0].tolist() == [10, 10]
        assert sc(ctx, 10, X, 0.5, D, G, 2, T, *O) == 0
        assert sc(ctx, 0, None, 0.5, None, None, 0, None, None, None, None, None) == 0
        assert sc(ctx, 10, X, 0.5, D, None, 0, None, None, None, None, None) == 0
        assert sc(ctx, -1, X, 0.5, D, None, 2, T, *O) == EINVAL and sc(ctx, 2 ** 31, X, 0.5, D, None, 2, T, *O) == EINVAL
        assert sc(ctx, 10, None, 0.5, D, None, 2, T, *O) == EINVAL and sc(ctx, 10, X, 0.5, None, None, 2, T, *O) == EINVAL
        for voxel in (0.0, -0.5, np.nan, np.inf):
            assert sc(ctx, 10, X, voxel, D, None, 2, T, *O) == EINVAL
        assert sc(ctx, 10, X, 0.5, D, None, -1, T, *O) == EINVAL and sc(ctx, 10, X, 0.5, D, None, 2, None, *O) == EINVAL
        for bad in (-0.1, np.nan):
            assert sc(ctx, 10, X, 0.5, D, None, 2, np.array([0.1, bad], f32).ctypes.data, *O) == EINVAL
        for q in range(4):
            assert sc(ctx, 10, X, 0.5, D, None, 2, T, *[None if i == q else o for i, o in enumerate(O)]) == EINVAL
        wide = np.array([[0, 0, 0], [0, 3e6, 0]], f32)  # 3e6 voxels of size 1 along y: more than 2^21
        assert sc(ctx, 2, wide.ctypes.data, 1.0, D, None, 2, T, *O) == EINVAL
        assert b"2^21" in lib.apd_eval_last_error(ctx)
        assert sc(ctx, 2, wide.ctypes.data, 2.0, D, None, 2, T, *O) == 0 and outs[3].tolist() == [2, 2]
        assert sc(ctx, 10, X, 0.5, D, None, 2, T, *O) == 0 and outs[0].tolist() == [10, 10]  # still usable

        cube, faces, o = lib.apd_eval_cube_cameras, (A.ApdCamera * 6)(), np.zeros(3, f32)
        assert cube(o.ctypes.data, 2, faces) == 0 and cube(o.ctypes.data, 16384, faces) == 0
        assert cube(o.ctypes.data, 1, faces) == EINVAL and cube(o.ctypes.data, 16385, faces) == EINVAL
        assert cube(None, 8, faces) == EINVAL and cube(o.ctypes.data, 8, None) == EINVAL
        for bad in (np.nan, np.inf, -np.inf):
            assert cube(np.array([0, bad, 0], f32).ctypes.data, 8, faces) == EINVAL
    finally:
        e.close()


# ---- 6. command line -----------------------------------------------------------------------------------

def parse_result_lines(text):
    """The string handling of the evaluation script this mode stands in for, restated: a line is
    found by its first word, the numbers follow the last colon, separated by single spaces."""
    result = {}
    for line in text.splitlines():
        line = line.strip()
        for word, key in (("Completenesses", "completeness"), ("Accuracies", "accuracy"), ("F1-scores", "f1")):
            if line.startswith(word):
                values = [float(x) for x in line.split(":")[-1].strip().split(" ")]
                result[key] = {name: values[i] for i, name in enumerate(("0.01", "0.02", "0.05", "0.1", "0.2", "0.5"))}
    return result


def test_command_line(eng, room, tmp_path):
    rec, scans, parts, _ = room
    a = 0.4
    poses = [np.array([[1, 0, 0, ROOM_ORIGINS[0][0]], [0, 1, 0, ROOM_ORIGINS[0][1]], [0, 0, 1, ROOM_ORIGINS[0][2]],
                       [0, 0, 0, 1]], np.float64),
             np.array([[np.cos(a), -np.sin(a), 0, ROOM_ORIGINS[1][0]], [np.sin(a), np.cos(a), 0, ROOM_ORIGINS[1][1]],
                       [0, 0, 1, ROOM_ORIGINS[1][2]], [0, 0, 0, 1]], np.float64)]
    # the files hold scanner-local points; what the tool sees is their double-then-float32 transform
    local = [((pts.astype(np.float64) - M[:3, 3]) @ M[:3, :3]).astype(f32) for (pts, _), M in zip(scans, poses)]
    local[1] = np.concatenate([local[1], [[np.nan, 0, 0]]]).astype(f32)  # a non-finite scan point is dropped
    world = [to_world_ref(p, M) for p, M in zip(local, poses)]
    assert not same_bits(world[1][0][:-1], scans[1][0]) and np.abs(world[1][0][:-1] - scans[1][0]).max() < 1e-5
    rec_in = np.concatenate([rec[:100], [[0, np.inf, 0]], rec[100:]]).astype(f32)
    rng = np.random.default_rng(1)
    (tmp_path / "scans").mkdir()
    (tmp_path / "rec.ply").write_bytes(ply_apd_layout(rec_in, rng))
    (tmp_path / "scans" / "s0.ply").write_bytes(ply_gt_layout(local[0]))
    (tmp_path / "scans" / "s1.ply").write_bytes(ply_apd_layout(local[1], rng))
    (tmp_path / "room.mlp").write_text(mlp_text([("scans/s0.ply", poses[0]), ("scans/s1.ply", poses[1])]))
    ref = protocol_ref(rec_in, world, TOLS, 0.25, 48, 1, 0.5, brute)
    out = tmp_path / "o.json"
    p = subprocess.run([APD_EVAL, "--cloud", tmp_path / "rec.ply", "--gt_mlp", tmp_path / "room.mlp", "--cube_size", "48",
                        "--voxel", "0.25", "--json", out, "--accuracy_cloud_out", tmp_path / "acc",
                        "--completeness_cloud_out", tmp_path / "comp"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.stdout, p.stderr)
    j = json.loads(out.read_text())["scanners"]
    m = A.cloud_metrics_scanners(rec_in, world, engine=eng, voxel=0.25, cube_size=48)
    assert j["splat"] == m["splat"] == 1 and j["cube_size"] == 48 and j["voxel"] == 0.25 and j["max_dist"] == 0.5
    assert j["tolerances"] == list(TOLS) and [float(f32(t)) for t in TOLS] == m["tolerances"] and j["rec"]["points_in"] == 5801 and j["rec"]["points"] == 5800
    assert j["gt"]["points"] == 13500 and [s["points_in"] for s in j["positions"]] == [7500, 6001]
    assert [s["origin"] for s in j["positions"]] == [[float(v) for v in o] for _, o in world]
    for side in ("accuracy", "completeness"):
        for k in ("good", "bad", "ratio_sum", "voxels"):
            assert j[side][k] == m[side][k] == ref[side][k], (side, k)
        for k in ("points", "unobserved", "score", "plain", "plain_of_all"):
            assert j[side][k] == m[side][k], (side, k)
    assert j["f1"] == m["f1"]
    # the result lines, as the evaluation script reads them
    got = parse_result_lines(p.stdout)
    lines = p.stdout.splitlines()
    assert "Tolerances: 0.01 0.02 0.05 0.1 0.2 0.5" in lines
    for key, values in (("accuracy", m["accuracy"]["score"]), ("completeness", m["completeness"]["score"]), ("f1", m["f1"])):
        assert list(got[key].values()) == [float("%.6f" % v) for v in values]
        assert all(0 <= v <= 1 for v in values)
    # the coloured clouds: the finite input points in order, coloured by the reference's classes
    for name, pts, dist, gap in (("acc", ref["R"], ref["accuracy_dist"], ref["gap"]),
                                 ("comp", ref["G"], ref["completeness_dist"], None)):
        for t, label in zip(TOLS, ("0.01", "0.02", "0.05", "0.1", "0.2", "0.5")):
            xyz, rgb = read_ply_xyz_rgb(tmp_path / name / ("tolerance_%s.ply" % label))
            assert same_bits(xyz, pts) and np.array_equal(rgb, colours_ref(dist, gap, t))
        if gap is None:
            assert not rgb[:, 2].any()
        else:
            assert len(set(map(tuple, colours_ref(dist, gap, 0.1)))) == 3
