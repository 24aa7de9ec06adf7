"""apd_eval_render_depth / apd_eval_visibility on the GPU against the literal float32 numpy restatement
of the contract in tests/render_lib.py, bit for bit: no tolerances anywhere. The counts quoted in the
assertions come from that numpy reference on the draws below."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import apd_abi as A
import synth
from eval_lib import APD_EVAL, REPO, brute, f32, plane_pair, same_bits
from render_lib import (make_cam, project_ref, render_ref, seen_ref, two_wall_camera, two_wall_cloud, visible_ref)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    return A.load_library()


@pytest.fixture(scope="module")
def eng(lib):
    e = A.EvalEngine(0, lib)
    yield e
    e.close()


@pytest.fixture(scope="module")
def walls():
    """Case 1's scene with its reference maps at splat 0, 1, 2 (computed once, never modified)."""
    cam = two_wall_camera()
    cloud, parts = two_wall_cloud()
    ref = {s: render_ref(cloud, cam, s) for s in (0, 1, 2)}
    return cam, cloud, parts, ref


def simple_cam(W, H, f=None, cx=None, cy=None):
    f = 0.8 * max(W, H) if f is None else f
    K = [[f, 0, W / 2 if cx is None else cx], [0, f, H / 2 if cy is None else cy], [0, 0, 1]]
    return make_cam(K, np.eye(3), [0, 0, 0], W, H)


def box_cloud(rng, n):
    return np.column_stack([rng.uniform(-1, 1, (n, 2)), rng.uniform(2, 4, n)]).astype(f32)


def check_render(eng, cloud, cams, splat):
    got = eng.render_depth(cloud, cams, splat, want_index=True)
    assert len(got) == len(cams)
    for (dep, idx), cam in zip(got, cams):
        rd, ri = render_ref(cloud, cam, splat)
        assert dep.shape == rd.shape and dep.dtype == f32 and idx.dtype == np.int32
        assert same_bits(dep, rd), int((dep.view(np.uint32) != rd.view(np.uint32)).sum())
        assert np.array_equal(idx, ri)
    return got


# ---- 1. two walls -----------------------------------------------------------------------------------

def test_two_wall_inputs_are_not_vacuous(walls):
    cam, cloud, parts, ref = walls
    kept, d, u, v = project_ref(cloud, cam)
    inb = kept & (u >= 0) & (u < 67) & (v >= 0) & (v < 49)
    assert int(np.isfinite(cloud).all(axis=1).sum()) == 3650 and int(kept.sum()) == 3550
    assert 0.05 * 3550 <= int(inb.sum()) <= 0.95 * 3550 and int(inb.sum()) == 2582
    assert not kept[parts["behind"]].any() and not kept[parts["bad"]].any()
    assert [int((ref[s][0] == 0).sum()) for s in (0, 1, 2)] == [1599, 30, 0]
    assert ref[0][0].size == 3283 and ((ref[0][1] >= 0) & (ref[0][1] < 900)).sum() == 688  # both walls win pixels


@pytest.mark.parametrize("splat", [0, 1, 2])
def test_two_wall_render(eng, walls, splat):
    cam, cloud, parts, ref = walls
    dep, idx = eng.render_depth(cloud, [cam], splat, want_index=True)[0]
    assert same_bits(dep, ref[splat][0]) and np.array_equal(idx, ref[splat][1])
    assert ((idx == -1) == (dep == 0)).all()
    assert not ((idx >= parts["dup"].start) & (idx < parts["dup"].stop)).any()  # ties go to the lowest index
    only = eng.render_depth(cloud, [cam], splat)  # without index maps
    assert len(only) == 1 and same_bits(only[0], ref[splat][0])


# ---- 2. visibility ----------------------------------------------------------------------------------

@pytest.mark.parametrize("splat,front,back", [(0, 864, 1303), (1, 690, 789), (2, 525, 695)])
def test_visibility_against_own_maps(eng, walls, splat, front, back):
    cam, cloud, parts, ref = walls
    want = visible_ref(cloud, cam, ref[splat][0], 0.01)
    # both outcomes are well represented among the in-bounds points of each wall (900 and 1 632)
    assert int(want[parts["front"]].sum()) == front and int(want[parts["back"]].sum()) == back
    seen, n_any = eng.visibility(cloud, [cam], [ref[splat][0]], 0.01, want_any=True)
    assert seen.dtype == np.int32 and np.array_equal(seen, want.astype(np.int32)) and n_any == int(want.sum())
    want0 = visible_ref(cloud, cam, ref[splat][0], 0.0)
    assert 0 < int(want0.sum()) < int(want.sum())
    assert np.array_equal(eng.visibility(cloud, [cam], [ref[splat][0]], 0.0), want0.astype(np.int32))


def test_visibility_against_a_map_with_holes(eng, walls):
    cam, cloud, parts, ref = walls
    dep = ref[2][0].copy()
    dep[::3, ::2] = 0
    dep[1::3, 1::2] = np.nan
    dep[2::3, ::5] = f32(-4.0)
    dep[5, 7], dep[6, 8] = np.inf, -np.inf
    want = seen_ref(cloud, [cam, cam], [dep, ref[0][0]], 0.01)
    assert set(np.unique(want)) == {0, 1, 2}
    seen, n_any = eng.visibility(cloud, [cam, cam], [dep, ref[0][0]], 0.01, want_any=True)
    assert np.array_equal(seen, want) and n_any == int((want > 0).sum())


# ---- 3. border rounding -----------------------------------------------------------------------------

def _near(t):
    """float32 values x with x + 0.5f at, just below and just above t"""
    t = f32(t)
    s = [np.nextafter(t, f32(-np.inf)), t, np.nextafter(t, f32(np.inf))]
    out = []
    for v in s:
        x = f32(v - f32(0.5))
        out += [np.nextafter(x, f32(-np.inf)), x, np.nextafter(x, f32(np.inf))]
    return out


@pytest.mark.parametrize("splat", [0, 3])
def test_border_rounding(eng, splat):
    W, H = 13, 9
    cam = make_cam([[1, 0, 0], [0, 1, 0], [0, 0, 1]], np.eye(3), [0, 0, 0], W, H)  # px = x / 1, py = y / 1
    xs = [x for t in (0, W, -splat, W + splat, -splat - 1, W + splat + 1) for x in _near(t)]
    ys = [y for t in (0, H, -splat, H + splat, -splat - 1, H + splat + 1) for y in _near(t)]
    pts = [(x, 4.0, 1.0) for x in xs] + [(6.0, y, 1.0) for y in ys] + [(x, y, 1.0) for x, y in zip(xs, ys)]
    cloud = np.array(pts, f32)
    kept, d, u, v = project_ref(cloud, cam)
    assert kept.all()
    centre_in = (u >= 0) & (u < W) & (v >= 0) & (v < H)
    # every depth is 1 and ties go to the lowest index: the points centred outside go first, so that
    # their footprints show in the maps
    cloud = np.concatenate([cloud[~centre_in], cloud[centre_in]])
    kept, d, u, v = project_ref(cloud, cam)
    centre_in = (u >= 0) & (u < W) & (v >= 0) & (v < H)
    rd, ri = render_ref(cloud, cam, splat)
    winners = np.unique(ri[ri >= 0])
    assert 0 < centre_in.sum() < len(cloud)
    if splat:
        # a centre outside the image whose footprint reaches inside wins pixels, and some footprints stay outside
        assert (~centre_in[winners]).any()
        reach = (u + splat >= 0) & (u - splat < W) & (v + splat >= 0) & (v - splat < H)
        assert (~reach).any() and (reach & ~centre_in).any()
    check_render(eng, cloud, [cam], splat)
    want = visible_ref(cloud, cam, rd, 0.0)
    assert np.array_equal(want, centre_in)  # every depth is 1: visible iff the centre is inside
    assert np.array_equal(eng.visibility(cloud, [cam], [rd], 0.0), want.astype(np.int32))


def test_huge_and_overflowing_projections(eng):
    """u or v at INT32_MIN, near INT32_MAX, px infinite or NaN: nothing is covered, nothing overflows."""
    W, H = 16, 16
    cam = simple_cam(W, H, f=1.0, cx=0.0, cy=0.0)
    cloud = np.array([(3.0, 3.0, 1.0), (2147483520.0, 3.0, 1.0), (-2147483648.0, 3.0, 1.0), (3e9, 3.0, 1.0),
                      (-3e9, 3.0, 1.0), (3.0, 2147483520.0, 1.0), (3e38, 3.0, 1e-38), (1e-30, 1e-30, 1e-45),
                      (5.0, 5.0, 2.0)], f32)
    kept, d, u, v = project_ref(cloud, cam)
    assert (u == -(2 ** 31)).any() and (u == 2147483520).any() and kept.sum() >= 8
    for splat in (0, 16):
        got = check_render(eng, cloud, [cam], splat)
        assert set(np.unique(got[0][1])) <= {-1, 0, 8}


# ---- 4. sizes ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_point_counts(eng, n):
    rng = np.random.default_rng(40 + n)
    cloud = box_cloud(rng, n)
    got = check_render(eng, cloud, [simple_cam(31, 17)], 1)
    if n == 0:
        assert (got[0][0] == 0).all() and (got[0][1] == -1).all()
    else:
        assert (got[0][1] >= 0).any()
    seen = eng.visibility(cloud, [simple_cam(31, 17)], [got[0][0]], 0.01)
    assert np.array_equal(seen, seen_ref(cloud, [simple_cam(31, 17)], [got[0][0]], 0.01)) and len(seen) == n


@pytest.mark.parametrize("W,H", [(1, 1), (1, 130), (130, 1)])
def test_thin_images(eng, W, H):
    rng = np.random.default_rng(W + 7 * H)
    cloud = box_cloud(rng, 300)
    for splat in (0, 2):
        got = check_render(eng, cloud, [simple_cam(W, H)], splat)
        assert (got[0][0] > 0).any()


def test_view_counts_and_null_index_maps(eng, lib):
    rng = np.random.default_rng(44)
    cloud = box_cloud(rng, 500)
    cams = [simple_cam(40, 30), simple_cam(17, 23), simple_cam(64, 5)]
    assert eng.render_depth(cloud, [], 0) == [] and eng.render_depth(cloud, [], 0, want_index=True) == []
    seen, n_any = eng.visibility(cloud, [], [], 0.01, want_any=True)
    assert (seen == 0).all() and len(seen) == 500 and n_any == 0
    check_render(eng, cloud, cams[:1], 0)
    got = check_render(eng, cloud, cams, 1)
    # index NULL, then only index[1] NULL
    arr = eng._cams(cams)
    dep = [np.full((c.height, c.width), -1, f32) for c in cams]
    idx = [np.full((c.height, c.width), -7, np.int32) for c in cams]
    eng.render_depth_ptr(500, cloud.ctypes.data, arr, 1, [d.ctypes.data for d in dep], None)
    assert all(same_bits(d, g[0]) for d, g in zip(dep, got))
    eng.render_depth_ptr(500, cloud.ctypes.data, arr, 1, [d.ctypes.data for d in dep],
                         [idx[0].ctypes.data, None, idx[2].ctypes.data])
    assert np.array_equal(idx[0], got[0][1]) and (idx[1] == -7).all() and np.array_equal(idx[2], got[2][1])
    want = seen_ref(cloud, cams, [g[0] for g in got], 0.01)
    assert set(np.unique(want)) >= {0, 3}
    seen, n_any = eng.visibility(cloud, cams, [g[0] for g in got], 0.01, want_any=True)
    assert np.array_equal(seen, want) and n_any == int((want > 0).sum())


def test_more_views_than_one_launch_takes(eng):
    """The visibility kernel takes the views in chunks: 19 views of different sizes."""
    rng = np.random.default_rng(45)
    cloud = box_cloud(rng, 400)
    cams = [simple_cam(20 + 3 * k, 35 - k, cx=10.0 + 2 * k) for k in range(19)]
    maps = eng.render_depth(cloud, cams, 0)
    for m, cam in zip(maps, cams):
        assert same_bits(m, render_ref(cloud, cam, 0)[0])
    want = seen_ref(cloud, cams, maps, 0.01)
    assert want.max() > 8
    assert np.array_equal(eng.visibility(cloud, cams, maps, 0.01), want)


def test_a_view_the_cloud_misses(eng):
    rng = np.random.default_rng(46)
    cloud = box_cloud(rng, 300)
    away = make_cam([[20, 0, 10], [0, 20, 8], [0, 0, 1]], np.diag([-1.0, 1.0, -1.0]), [0, 0, 0], 20, 16)  # looks along -z
    aside = simple_cam(20, 16, f=20.0, cx=-500.0)  # everything projects far to the left
    for cam in (away, aside):
        dep, idx = eng.render_depth(cloud, [cam], 2, want_index=True)[0]
        assert (dep == 0).all() and not np.signbit(dep).any() and (idx == -1).all()
        assert (eng.visibility(cloud, [cam], [np.ones((16, 20), f32)], 0.01) == 0).all()


# ---- 5. order independence --------------------------------------------------------------------------

def test_permuted_cloud(eng, walls):
    cam, cloud, parts, ref = walls
    perm = np.random.default_rng(50).permutation(len(cloud))
    for splat in (0, 2):
        dep, idx = eng.render_depth(cloud[perm], [cam], splat, want_index=True)[0]
        assert same_bits(dep, ref[splat][0])
        hit = idx >= 0
        back = perm[idx[hit]]  # a duplicate may stand in for its original: the coordinates are the same
        assert same_bits(cloud[back], cloud[ref[splat][1][hit]])


_CHILD = """
import sys
import numpy as np
import apd_abi as A
from render_lib import two_wall_camera, two_wall_cloud
eng = A.EvalEngine(0)
cloud, _ = two_wall_cloud()
out = {}
for s in (0, 1, 2):
    d, i = eng.render_depth(cloud, [two_wall_camera()], s, want_index=True)[0]
    out["d%d" % s], out["i%d" % s] = d, i
np.savez(sys.argv[1], **out)
"""


@pytest.mark.parametrize("order", ["input", "morton"])
def test_render_order_switch(walls, tmp_path, order):
    cam, cloud, parts, ref = walls
    env = dict(os.environ, APD_EVAL_RENDER_ORDER=order,
               PYTHONPATH=os.pathsep.join([os.path.join(REPO, "apde-mvs_amd"), os.path.join(REPO, "tests")]))
    out = tmp_path / (order + ".npz")
    p = subprocess.run([sys.executable, "-c", _CHILD, str(out)], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    got = np.load(out)
    for s in (0, 1, 2):
        assert same_bits(got["d%d" % s], ref[s][0]) and np.array_equal(got["i%d" % s], ref[s][1])


# ---- 6. device pointers, context reuse ----------------------------------------------------------------

def test_device_pointers_and_reuse(lib, walls):
    import torch
    cam, cloud, parts, ref = walls
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(60)
    eng = A.EvalEngine(0, lib)
    target, query = box_cloud(rng, 900), box_cloud(rng, 700)
    eng.set_target(target)
    want_dist = brute(query, target, 0.5)
    for cl in (box_cloud(rng, 5000), cloud, box_cloud(rng, 70)):  # clouds of different size, one context
        cams = [cam, simple_cam(33, 21)]
        got = eng.render_depth(torch.from_numpy(cl).to(dev), cams, 1, want_index=True)
        maps = []
        for (dep, idx), c in zip(got, cams):
            assert dep.is_cuda and idx.is_cuda and dep.dtype == torch.float32 and idx.dtype == torch.int32
            rd, ri = render_ref(cl, c, 1)
            assert same_bits(dep.cpu().numpy(), rd) and np.array_equal(idx.cpu().numpy(), ri)
            maps.append(dep)
        # the renderer did not disturb the target
        assert same_bits(eng.distances(query, 0.5)[0], want_dist)
        seen, n_any = eng.visibility(torch.from_numpy(cl).to(dev), cams, maps, 0.01, want_any=True)
        want = seen_ref(cl, cams, [m.cpu().numpy() for m in maps], 0.01)
        assert seen.is_cuda and np.array_equal(seen.cpu().numpy(), want) and n_any == int((want > 0).sum())
        # host maps against a device cloud
        seen2 = eng.visibility(torch.from_numpy(cl).to(dev), cams, [m.cpu().numpy() for m in maps], 0.01)
        assert np.array_equal(seen2.cpu().numpy(), want)
        assert same_bits(eng.distances(query, 0.5)[0], want_dist)
        # and a new target or a voxel pass in between does not disturb the renderer
        eng.set_target(target)
        eng.voxel_downsample(query, 0.1)
        assert same_bits(eng.render_depth(cl, cams[:1], 1)[0], render_ref(cl, cam, 1)[0])
    tm = eng.render_timing()
    assert tm["render_ms"] > 0 and tm["visibility_ms"] > 0
    eng.close()


# ---- 7. status codes --------------------------------------------------------------------------------

def test_status_codes(lib, walls):
    cam, cloud, parts, ref = walls
    eng = A.EvalEngine(0, lib)
    ctx, n, xp = eng.ctx, len(cloud), cloud.ctypes.data
    dep, idx, seen = np.zeros((49, 67), f32), np.zeros((49, 67), np.int32), np.zeros(n, np.int32)
    cams = (A.ApdCamera * 1)(cam)
    dp, ip = (C.c_void_p * 1)(dep.ctypes.data), (C.c_void_p * 1)(idx.ctypes.data)
    null1 = (C.c_void_p * 1)(None)

    def sized(w, h):
        c = (A.ApdCamera * 1)(cam)
        c[0].width, c[0].height = w, h
        return c

    def render(n_=n, x=xp, nv=1, c=cams, splat=0, d=dp, i=ip):
        return lib.apd_eval_render_depth(ctx, n_, x, nv, c, splat, d, i)

    def vis(n_=n, x=xp, nv=1, c=cams, d=dp, tol=0.01, s=seen.ctypes.data):
        return lib.apd_eval_visibility(ctx, n_, x, nv, c, d, tol, s, None)

    def still_works():
        assert render() == 0 and same_bits(dep, ref[0][0]) and np.array_equal(idx, ref[0][1])
        assert vis() == 0 and np.array_equal(seen, visible_ref(cloud, cam, ref[0][0], 0.01).astype(np.int32))

    still_works()
    bad_views = [sized(0, 49), sized(67, 0), sized(-3, 49), sized(1 << 14, (1 << 14) + 1), sized(1 << 30, 1 << 30)]
    for kw in ([dict(n_=-1), dict(n_=2 ** 31), dict(x=None), dict(nv=-1), dict(c=None), dict(d=None), dict(d=null1),
                dict(splat=-1), dict(splat=17)] + [dict(c=c) for c in bad_views]):
        assert render(**kw) == -1, kw
        assert lib.apd_eval_last_error(ctx)
        still_works()
    for kw in ([dict(n_=-1), dict(n_=2 ** 31), dict(x=None), dict(nv=-1), dict(c=None), dict(d=None), dict(d=null1),
                dict(s=None), dict(tol=-0.01), dict(tol=float("nan")), dict(tol=float("inf"))] +
               [dict(c=c) for c in bad_views]):
        assert vis(**kw) == -1, kw
        assert lib.apd_eval_last_error(ctx)
        still_works()
    # valid edges: no points, no views, a NULL index list, the largest splat
    assert render(n_=0, x=None) == 0 and (dep == 0).all() and (idx == -1).all()
    assert render(nv=0, c=None, d=None, i=None) == 0 and vis(nv=0, c=None, d=None) == 0 and (seen == 0).all()
    assert vis(n_=0, x=None, s=None) == 0
    assert render(splat=16, i=None) == 0 and same_bits(dep, render_ref(cloud, cam, 16)[0])
    assert lib.apd_eval_get_render_timing(ctx, None, None) == 0
    still_works()
    eng.close()


# ---- 8. against analytic depth ----------------------------------------------------------------------

@pytest.fixture(scope="module")
def scene():
    sc = synth.make_scene(160, 120, 4)
    cams = [A.camera_from_values(synth.camera_struct_values(c, sc.width, sc.height)) for c in sc.cameras]
    return sc, cams, synth.gt_cloud(sc)


def test_against_analytic_depth(eng, scene):
    sc, cams, cloud = scene
    assert cloud.shape == (95473, 3)
    got = eng.render_depth(cloud, [cams[0], cams[3]], 0, want_index=True)
    for (dep, idx), v, covered in zip(got, (0, 3), (19200, 18686)):
        rd, ri = render_ref(cloud, cams[v], 0)
        assert same_bits(dep, rd) and np.array_equal(idx, ri)
        gt = sc.gt_depth[v]
        assert int((gt > 0).sum()) == covered and np.array_equal(rd > 0, gt > 0)  # covered exactly where there is surface
        m = gt > 0
        close = np.abs(rd[m].astype(np.float64) - gt[m]) <= 1e-2 * gt[m]
        # a condition on the scene (the rest are foreground points at depth discontinuities), not a
        # tolerance on the kernel: the device equals the reference bit for bit
        assert close.mean() >= 0.99


# ---- 9. cloud_metrics(gt_cams=...) ------------------------------------------------------------------

def test_cloud_metrics_with_visibility(eng):
    rng = np.random.default_rng(21)
    rec, gt = plane_pair(rng)
    gt[9] = (0, np.inf, 0)
    wide = simple_cam(90, 40, f=20.0, cx=40.0, cy=20.0)    # sees the plane and the far patch
    narrow = simple_cam(60, 60, f=40.0, cx=30.0, cy=30.0)  # the far patch lies outside its image
    cams = [wide, narrow]
    tol = [0.01, 0.02, 0.05, 0.1, 0.2, 0.5]
    g = gt[np.isfinite(gt).all(axis=1)]
    far = g[:, 0] > 1.5
    assert far.sum() == 300
    seen = seen_ref(g, cams, [render_ref(g, c, 1)[0] for c in cams], 0.01)
    assert (seen[far] <= 1).all() and (seen[far] == 1).sum() > 200 and (seen[~far] == 2).sum() > 2000
    gv = g[seen >= 2]
    d_acc, d_comp = brute(rec, g, 0.5), brute(gv, rec, 0.5)

    m = A.cloud_metrics(rec, gt, tol, engine=eng, gt_cams=cams, min_views=2, splat=1, occlusion_tol=0.01)
    assert m["gt"] == {"points_in": len(gt), "points_finite": len(g), "points": len(g), "points_visible": len(gv)}
    assert m["accuracy"]["within"] == [int((d_acc <= f32(t)).sum()) for t in tol]
    assert m["completeness"]["within"] == [int((d_comp <= f32(t)).sum()) for t in tol]
    assert m["accuracy"]["ratio"] == [w / len(rec) for w in m["accuracy"]["within"]]
    assert m["completeness"]["ratio"] == [w / len(gv) for w in m["completeness"]["within"]]
    assert m["completeness"]["inf"] == int(np.isinf(d_comp).sum())
    f1 = [2 * a * c / (a + c) if a + c > 0 else 0.0 for a, c in zip(m["accuracy"]["ratio"], m["completeness"]["ratio"])]
    assert m["f1"] == f1

    one = A.cloud_metrics(rec, gt, tol, engine=eng, gt_cams=cams, min_views=1, splat=1)
    assert one["gt"]["points_visible"] == int((seen >= 1).sum()) > len(gv)

    # without gt_cams: today's dict, key for key, and the unfiltered completeness is lower
    plain = A.cloud_metrics(rec, gt, tol, engine=eng)
    assert set(plain) == {"tolerances", "max_dist", "voxel", "timing_ms", "rec", "gt", "accuracy", "completeness", "f1"}
    assert plain["gt"] == {"points_in": len(gt), "points_finite": len(g), "points": len(g)}
    assert set(plain["timing_ms"]) == {"accuracy", "completeness"}
    assert plain["accuracy"] == m["accuracy"]
    d_all = brute(g, rec, 0.5)
    assert plain["completeness"]["within"] == [int((d_all <= f32(t)).sum()) for t in tol]
    assert plain["completeness"]["ratio"][3] < m["completeness"]["ratio"][3]
    with pytest.raises(ValueError):
        A.cloud_metrics(rec, gt, tol, engine=eng, gt_cams=cams, min_views=0)


# ---- 10. command line -------------------------------------------------------------------------------

def _cli_camera(cam, src_w, src_h, W, H):
    """The camera as `apd_eval` sees it: cam.txt read as float32, rescaled as fusion's load_view does."""
    K = cam.K.astype(f32).copy()
    if (src_w, src_h) != (W, H):
        sx, sy = f32(W) / f32(src_w), f32(H) / f32(src_h)
        K[0, 0] *= sx
        K[0, 2] *= sx
        K[1, 1] *= sy
        K[1, 2] *= sy
    return make_cam(K, cam.R, cam.t, W, H)


@pytest.fixture(scope="module")
def scans(tmp_path_factory):
    root = tmp_path_factory.mktemp("render_cli")
    sc = synth.make_scene(64, 48, 2)
    rng = np.random.default_rng(70)
    cloud = synth.gt_cloud(sc)
    synth.write_ply(str(root / "gt.ply"), cloud)
    out = {"root": root, "scene": sc, "cloud": cloud}
    for name, step in (("full", 1), ("half", 2)):
        folder = root / name
        synth.write_scan(sc, str(folder), ext=".png")  # PGM bytes: the decoders go by content
        depths = []
        for i, g in enumerate(sc.gt_depth):
            d = (g * (1 + rng.normal(0, 3e-3, g.shape))).astype(f32)[::step, ::step].copy()
            d[rng.random(d.shape) < 0.05] = 0
            v = folder / "APD" / f"{i:08d}"
            os.makedirs(v)
            synth.write_bin_mat(str(v / "depths.bin"), d)
            synth.write_bin_mat(str(v / "weak.bin"), np.ones(d.shape, np.uint8))
            depths.append(d)
        out[name] = (folder, depths)
    synth.write_scan(sc, str(root / "bare"), ext=".png")  # no results: the view size is the image's
    return out


def run_eval(*args):
    return subprocess.run([APD_EVAL, *map(str, args)], capture_output=True, text=True, timeout=300)


@pytest.mark.parametrize("name,step,splat", [("full", 1, 0), ("half", 2, 1), ("bare", 1, 0)])
def test_cli_render_gt(scans, tmp_path, name, step, splat):
    sc, cloud = scans["scene"], scans["cloud"]
    folder = scans["root"] / name
    p = run_eval("--render_gt", scans["root"] / "gt.ply", "--scan", folder, "--out", tmp_path / "gtd", "--splat", splat,
                 "--json", tmp_path / "r.json")
    assert p.returncode == 0, (p.stdout, p.stderr)
    j = json.loads((tmp_path / "r.json").read_text())["render"]
    assert j["points"] == len(cloud) and j["splat"] == splat and len(j["views"]) == len(sc.cameras)
    W, H = sc.width // step, sc.height // step
    for i, cam in enumerate(sc.cameras):
        want = render_ref(cloud, _cli_camera(cam, sc.width, sc.height, W, H), splat)[0]
        got = synth.read_bin_mat(str(tmp_path / "gtd" / f"{i:08d}.bin"))
        assert got.dtype == f32 and same_bits(got, want)
        assert j["views"][i] == {"id": i, "width": W, "height": H, "covered": int((want > 0).sum())} and (want > 0).any()


@pytest.mark.parametrize("name", ["full", "half"])
def test_cli_gt_cloud_equals_render_then_gt_depth(scans, tmp_path, name):
    folder, depths = scans[name]
    ply = scans["root"] / "gt.ply"
    assert run_eval("--render_gt", ply, "--scan", folder, "--out", tmp_path / "gtd").returncode == 0
    a = run_eval("--dense_folder", folder, "--gt_depth", tmp_path / "gtd", "--json", tmp_path / "a.json")
    b = run_eval("--dense_folder", folder, "--gt_cloud", ply, "--json", tmp_path / "b.json")
    assert a.returncode == 0 and b.returncode == 0, (a.stderr, b.stderr)
    ja = json.loads((tmp_path / "a.json").read_text())["depth"]
    jb = json.loads((tmp_path / "b.json").read_text())["depth"]
    assert ja.pop("b") == str(tmp_path / "gtd") and jb.pop("b") == str(ply)
    assert ja == jb and ja["b_is_gt_depth"] is True and ja["failed_views"] == 0
    assert a.stdout == b.stdout
    t = ja["total"]
    # the same geometry on both sides (a camera that was not rescaled would miss most of the half-size
    # image). Not tighter: at half size the z-buffer keeps the nearest of about four cloud points per
    # pixel while depths.bin holds one sample, so slanted surfaces differ by more than 1e-2 there
    assert t["valid_both"] > 0.8 * t["pixels"] and t["within_1e-2"] > 0.5 * t["valid_both"] > 0


def test_cli_cloud_mode_with_visible_views(scans, tmp_path):
    sc, cloud = scans["scene"], scans["cloud"]
    folder = scans["full"][0]
    rng = np.random.default_rng(71)
    rec = (cloud[::2] + rng.normal(0, 0.01, cloud[::2].shape)).astype(f32)
    synth.write_ply(str(tmp_path / "rec.ply"), rec)
    cams = [_cli_camera(c, sc.width, sc.height, sc.width, sc.height) for c in sc.cameras]
    seen = seen_ref(cloud, cams, [render_ref(cloud, c, 1)[0] for c in cams], 0.02)
    gv = cloud[seen >= 2]
    assert 0.05 * len(cloud) < len(gv) < 0.95 * len(cloud)
    tol = [0.01, 0.02, 0.05, 0.1, 0.2, 0.5]
    d_acc, d_comp = brute(rec, cloud, 0.5), brute(gv, rec, 0.5)
    p = run_eval("--cloud", tmp_path / "rec.ply", "--gt", scans["root"] / "gt.ply", "--scan", folder, "--visible_views", 2,
                 "--splat", 1, "--occlusion_tol", 0.02, "--json", tmp_path / "c.json")
    assert p.returncode == 0, (p.stdout, p.stderr)
    j = json.loads((tmp_path / "c.json").read_text())["cloud"]
    assert j["gt"] == {"points_in": len(cloud), "points_finite": len(cloud), "points": len(cloud),
                       "points_visible": len(gv)}
    assert j["visibility"]["views"] == len(cams) and j["visibility"]["min_views"] == 2 and j["visibility"]["splat"] == 1
    assert j["accuracy"]["points"] == len(rec) and j["completeness"]["points"] == len(gv)
    assert j["accuracy"]["within"] == [int((d_acc <= f32(t)).sum()) for t in tol]
    assert j["completeness"]["within"] == [int((d_comp <= f32(t)).sum()) for t in tol]
    assert "z-buffer" in j["definition"]
    assert f"Visible ground truth: {len(gv)} of {len(cloud)} points" in p.stdout
    comp = [w / len(gv) for w in j["completeness"]["within"]]
    lines = dict(l.split(":", 1) for l in p.stdout.strip().splitlines())
    assert lines["Completenesses"].split() == ["%.6f" % c for c in comp]
    # the same numbers from Python
    m = A.cloud_metrics(rec, cloud, tol, gt_cams=cams, min_views=2, splat=1, occlusion_tol=0.02)
    assert m["gt"]["points_visible"] == len(gv) and m["completeness"]["within"] == j["completeness"]["within"]
