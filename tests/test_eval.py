"""include/apd_eval.h on the GPU: truncated nearest-neighbour distances and voxel down-sampling against
the literal float32 brute force of tests/eval_lib.py, bit for bit; counts, context reuse, device
pointers, status codes; cloud_metrics and the `apd_eval` command line."""
import ctypes as C
import json
import subprocess

import numpy as np
import pytest

import apd_abi as A
from eval_lib import APD_EVAL, INF, brute, f32, plane_pair, ply_apd_layout, ply_gt_layout, same_bits, voxel_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    return A.load_library()


@pytest.fixture(scope="module")
def eng(lib):
    e = A.EvalEngine(0, lib)
    yield e
    e.close()


def check(eng, q, t, md, tol=None):
    eng.set_target(t)
    dist, within = eng.distances(q, md, tol)
    ref = brute(q, t, md)
    assert same_bits(dist, ref), (int((dist.view(np.uint32) != ref.view(np.uint32)).sum()), len(ref))
    if tol is not None:
        assert within.tolist() == [int((ref <= f32(x)).sum()) for x in tol]
    return ref


def cube(rng, n):
    return rng.uniform(-1, 1, (n, 3)).astype(f32)


@pytest.mark.parametrize("n_target", [1, 2, 31, 32, 33, 63, 64, 65, 255, 256, 257, 2049])
def test_sizes_around_leaf_and_wave(eng, n_target):
    rng = np.random.default_rng(100 + n_target)
    check(eng, cube(rng, 130), cube(rng, n_target), 0.5)


@pytest.fixture(scope="module")
def cube5():
    rng = np.random.default_rng(5)
    return cube(rng, 3001), cube(rng, 4099), cube(rng, 5000)


@pytest.mark.parametrize("md,finite", [(0.05, 696), (10.0, 4099), (np.inf, 4099)])
def test_random_cube(eng, cube5, md, finite):
    t, q, _ = cube5
    ref = check(eng, q, t, md, [md])
    assert int(np.isfinite(ref).sum()) == finite


def test_max_dist_zero_matches_exact_duplicates_only(eng, cube5):
    t, q, _ = cube5
    qq = np.concatenate([t[:100], q[:100]])
    ref = check(eng, qq, t, 0.0, [0.0])
    assert (ref[:100] == 0).all() and np.isinf(ref[100:]).all()


@pytest.mark.parametrize("off,finite", [(0, 1638), (1000, 1048), (30000, 2768)])
def test_cutoff_boundary(eng, off, finite):
    rng = np.random.default_rng(11)
    md, n = f32(0.1), 3000
    x = f32(off) + np.arange(n, dtype=f32) + rng.random(n).astype(f32) * f32(0.5)
    sign = np.where(rng.random(n) < 0.5, f32(-1), f32(1))
    t = np.zeros((n + 1, 3), f32)
    t[1:, 0] = x
    q = np.zeros((n, 3), f32)
    q[:, 0] = x + sign * md
    assert q.dtype == f32
    ref = check(eng, q, t, md, [md])
    nfin = int(np.isfinite(ref).sum())
    assert 0.05 * n <= nfin <= 0.95 * n  # both outcomes of the cut are well represented
    assert nfin == finite


def _probe_queries(rng, pts):
    """Inside, near and far from a cloud."""
    c = pts[rng.integers(0, len(pts), 40)]
    return np.concatenate([c, c + rng.normal(0, 1e-4, c.shape).astype(f32), c + rng.normal(0, 0.05, c.shape).astype(f32),
                           c + f32(50.0), rng.uniform(-3, 3, (40, 3)).astype(f32)]).astype(f32)


@pytest.mark.parametrize("kind", ["copies", "coplanar", "collinear", "cluster_plus_far"])
@pytest.mark.parametrize("md", [0.1, np.inf])
def test_degenerate_geometry(eng, kind, md):
    rng = np.random.default_rng(7)
    if kind == "copies":
        t = np.tile(np.array([[0.25, -1.5, 3.0]], f32), (3000, 1))
    elif kind == "coplanar":
        t = cube(rng, 3000)
        t[:, 2] = f32(0.75)
    elif kind == "collinear":
        s = rng.uniform(-1, 1, 3000).astype(f32)
        t = np.stack([s, s * f32(2), s * f32(-0.5)], axis=1).astype(f32)
    else:
        t = np.concatenate([(rng.random((3000, 3)) * 1e-3).astype(f32) + f32(0.5),
                            np.array([[100, 0, 0], [0, -80, 0], [0, 0, 1e4], [-1e3, 5, 5], [7, 7, 7]], f32)])
    check(eng, _probe_queries(rng, t), t, md)


def test_non_finite_rows(eng):
    rng = np.random.default_rng(3)
    t, q = cube(rng, 500), cube(rng, 500)
    bad = [(np.nan, 0, 0), (0, np.inf, 0), (0, 0, -np.inf), (np.nan, np.nan, np.nan), (np.inf, -np.inf, 1)]
    for k, row in enumerate(bad):
        t[37 + 91 * k] = row
        q[11 + 83 * k] = row
    ref = check(eng, q, t, 0.5, [0.1, 0.5])
    assert np.isinf(ref[[11 + 83 * k for k in range(5)]]).all()
    check(eng, q, t, np.inf)
    # nothing but non-finite targets: no match at all
    check(eng, q, np.array(bad, f32), 0.5, [0.5])


def test_empty_sides(eng):
    rng = np.random.default_rng(4)
    t, q = cube(rng, 100), cube(rng, 70)
    eng.set_target(t)
    dist, within = eng.distances(np.zeros((0, 3), f32), 0.5, [0.1, 0.5])
    assert dist.shape == (0,) and within.tolist() == [0, 0]
    eng.set_target(np.zeros((0, 3), f32))
    dist, within = eng.distances(q, 0.5, [0.5])
    assert np.isinf(dist).all() and (dist > 0).all() and within.tolist() == [0]
    dist, within = eng.distances(q, np.inf, [np.inf])  # +inf <= +inf: the comparison is inclusive
    assert np.isinf(dist).all() and within.tolist() == [70]


def test_counts_inclusive_and_without_dist(eng, cube5):
    t, q, _ = cube5
    md = f32(0.08)
    ref = brute(q, t, md)
    hit = ref[np.isfinite(ref)]
    tol = [0.0, float(hit[len(hit) // 2]), 0.03, float(hit.max()), float(md)]  # two actual results, and max_dist
    want = [int((ref <= f32(x)).sum()) for x in tol]
    assert want[1] >= 1 and want[-1] == len(hit)
    eng.set_target(t)
    dist, within = eng.distances(q, md, tol)
    assert same_bits(dist, ref) and within.tolist() == want
    none, within = eng.distances(q, md, tol, want_dist=False)
    assert none is None and within.tolist() == want
    many = np.linspace(0, float(md), 19).astype(f32)  # more than one chunk of tolerances
    assert eng.distances(q, md, many)[1].tolist() == [int((ref <= x).sum()) for x in many]


def test_context_reuse(lib):
    rng = np.random.default_rng(8)
    targets = [cube(rng, 50), cube(rng, 5000), cube(rng, 300)]
    q1, q2 = cube(rng, 700), cube(rng, 90)
    eng = A.EvalEngine(0, lib)
    for t in targets:
        eng.set_target(t)
        for q in (q1, q2):
            got = eng.distances(q, 0.2)[0]
            fresh = A.EvalEngine(0, lib)
            fresh.set_target(t)
            assert same_bits(got, fresh.distances(q, 0.2)[0])
            fresh.close()
            assert same_bits(got, brute(q, t, 0.2))
    eng.close()


def test_device_pointers(eng, cube5):
    import torch
    t, q, v = cube5
    tol = [0.02, 0.05]
    eng.set_target(t)
    dist, within = eng.distances(q, 0.05, tol)
    keep = eng.voxel_downsample(v, 0.1)
    dev = torch.device("cuda", 0)
    eng.set_target(torch.from_numpy(t).to(dev))
    d_dist, d_within = eng.distances(torch.from_numpy(q).to(dev), 0.05, tol)
    assert d_dist.is_cuda and d_within.is_cuda
    assert same_bits(d_dist.cpu().numpy(), dist) and d_within.cpu().numpy().tolist() == within.tolist()
    d_keep = eng.voxel_downsample(torch.from_numpy(v).to(dev), 0.1)
    assert d_keep.is_cuda and np.array_equal(d_keep.cpu().numpy(), keep)


def test_status_codes(lib, cube5):
    t, q, _ = cube5
    assert lib.apd_eval_create(10_000) is None
    assert b"device" in lib.apd_eval_last_error(None)
    eng = A.EvalEngine(0, lib)
    ctx, qp, tp, n = eng.ctx, q.ctypes.data, t.ctypes.data, len(q)
    dist = np.zeros(n, f32)

    def distances(n_, ptr, md, tol=None):
        ta = None if tol is None else np.asarray(tol, f32)
        within = np.zeros(8, np.int64)
        return lib.apd_eval_distances(ctx, n_, ptr, md, dist.ctypes.data, 0 if ta is None else len(ta),
                                      None if ta is None else ta.ctypes.data, within.ctypes.data)

    assert distances(n, qp, 0.1) == -5  # APD_ESTATE: no target yet
    assert b"target" in lib.apd_eval_last_error(ctx)
    assert lib.apd_eval_set_target(ctx, -1, tp) == -1
    assert lib.apd_eval_set_target(ctx, 2**31, tp) == -1
    assert lib.apd_eval_set_target(ctx, 10, None) == -1
    assert distances(n, qp, 0.1) == -5  # the failed calls set no target
    assert lib.apd_eval_set_target(ctx, len(t), tp) == 0
    for bad in [(-1, qp, 0.1), (2**31, qp, 0.1), (n, None, 0.1), (n, qp, -0.5), (n, qp, float("nan")),
                (n, qp, 0.1, [0.05, -0.01]), (n, qp, 0.1, [float("nan")]), (n, qp, 0.1, [0.05, 0.2]),
                (n, qp, 0.1, [float("inf")])]:
        assert distances(*bad) == -1, bad
        assert lib.apd_eval_last_error(ctx)
        assert distances(n, qp, 0.05) == 0 and same_bits(dist, brute(q, t, 0.05))  # the context still works
    assert distances(n, qp, float("inf"), [float("inf")]) == 0  # +inf is allowed: no truncation
    keep, nk = np.zeros(n, np.int32), C.c_int64(-1)
    for bad_voxel in (0.0, -1.0, float("inf"), float("nan")):
        assert lib.apd_eval_voxel_downsample(ctx, n, qp, bad_voxel, keep.ctypes.data, C.addressof(nk)) == -1
    assert lib.apd_eval_voxel_downsample(ctx, -1, qp, 0.1, keep.ctypes.data, C.addressof(nk)) == -1
    assert lib.apd_eval_voxel_downsample(ctx, n, None, 0.1, keep.ctypes.data, C.addressof(nk)) == -1
    far = q.copy()
    far[5, 1] = 1e9
    assert lib.apd_eval_voxel_downsample(ctx, n, far.ctypes.data, 1e-3, keep.ctypes.data, C.addressof(nk)) == -1
    assert b"2^21" in lib.apd_eval_last_error(ctx)
    assert np.array_equal(eng.voxel_downsample(q, 0.1), voxel_ref(q, 0.1))
    assert distances(n, qp, 0.05) == 0 and same_bits(dist, brute(q, t, 0.05))  # the target survived all that
    tm = eng.timing()
    assert tm["build_ms"] > 0 and tm["query_ms"] > 0 and tm["voxel_ms"] > 0
    eng.close()


def test_voxel_random(eng, cube5):
    v = cube5[2]
    keep = eng.voxel_downsample(v, 0.1)
    assert keep.dtype == np.int32 and len(keep) == 3760
    assert np.array_equal(keep, voxel_ref(v, 0.1))


def test_voxel_faces_and_negative_coordinates(eng):
    rng = np.random.default_rng(9)
    vox = f32(0.1)
    k = rng.integers(-40, 40, (3000, 3)).astype(f32)
    x = (k * vox).astype(f32)  # exactly on voxel faces, as float32 products
    x[1000:2000] = np.nextafter(x[1000:2000], f32(-np.inf))  # just below them
    x[2000:] = np.nextafter(x[2000:], f32(np.inf))
    x[::7] = np.where(x[::7] == 0, f32(-0.0), x[::7])
    assert np.array_equal(eng.voxel_downsample(x, vox), voxel_ref(x, vox))


def test_voxel_small_and_giant(eng, cube5):
    v = cube5[2]
    pos = np.abs(v)
    assert eng.voxel_downsample(pos, 1e6).tolist() == [0]  # one giant voxel keeps index 0
    assert eng.voxel_downsample(np.zeros((0, 3), f32), 0.1).tolist() == []
    assert eng.voxel_downsample(v[:1], 0.1).tolist() == [0]
    bad = v[:600].copy()
    bad[0] = (np.nan, 0, 0)
    bad[17] = (0, np.inf, 0)
    bad[599] = (0, 0, -np.inf)
    keep = eng.voxel_downsample(bad, 0.25)
    assert np.array_equal(keep, voxel_ref(bad, 0.25)) and not set(keep.tolist()) & {0, 17, 599}
    assert eng.voxel_downsample(bad[[0, 17, 599]], 0.25).tolist() == []


def _expected(rec, gt, tol, md):
    d_r, d_g = brute(rec, gt, md), brute(gt, rec, md)
    out = {}
    for name, d in (("accuracy", d_r), ("completeness", d_g)):
        fin = d[np.isfinite(d)].astype(np.float64)
        out[name] = {"within": [int((d <= f32(t)).sum()) for t in tol], "inf": int(len(d) - len(fin)),
                     "mean": float(fin.sum() / len(fin)) if len(fin) else 0.0, "n": len(d)}
    return out


@pytest.fixture(scope="module")
def clouds(tmp_path_factory):
    rng = np.random.default_rng(21)
    rec, gt = plane_pair(rng)
    rec[5] = (np.nan, 0, 0)  # dropped before anything is counted
    gt[9] = (0, np.inf, 0)
    d = tmp_path_factory.mktemp("eval_cli")
    (d / "rec.ply").write_bytes(ply_apd_layout(rec, rng))
    (d / "gt.ply").write_bytes(ply_gt_layout(gt))
    return d, rec, gt


@pytest.mark.parametrize("voxel", [0.0, 0.05])
def test_cloud_metrics_and_cli(eng, clouds, voxel):
    d, rec, gt = clouds
    tol = [0.01, 0.02, 0.05, 0.1, 0.2, 0.5]
    r = rec[np.isfinite(rec).all(axis=1)]
    g = gt[np.isfinite(gt).all(axis=1)]
    if voxel:
        r, g = r[voxel_ref(r, voxel)], g[voxel_ref(g, voxel)]
        assert len(r) < len(rec) - 1 and len(g) < len(gt) - 1
    want = _expected(r, g, tol, 0.5)
    assert want["accuracy"]["inf"] > 0 and want["completeness"]["inf"] > 0

    m = A.cloud_metrics(rec, gt, tol, voxel=voxel, engine=eng)
    args = [APD_EVAL, "--cloud", str(d / "rec.ply"), "--gt", str(d / "gt.ply"), "--json", str(d / "out.json")]
    if voxel:
        args += ["--voxel", str(voxel)]
    p = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.stdout, p.stderr)
    j = json.loads((d / "out.json").read_text())["cloud"]

    for res in (m, j):
        assert res["rec"] == {"points_in": len(rec), "points_finite": len(rec) - 1, "points": len(r)}
        assert res["gt"] == {"points_in": len(gt), "points_finite": len(gt) - 1, "points": len(g)}
        assert res["max_dist"] == 0.5 and res["voxel"] == float(f32(voxel))
        for name in ("accuracy", "completeness"):
            assert res[name]["within"] == want[name]["within"]
            assert res[name]["inf"] == want[name]["inf"]
            assert abs(res[name]["mean"] - want[name]["mean"]) <= 1e-9 * want[name]["mean"]
    assert j["accuracy"]["build_ms"] > 0 and j["accuracy"]["query_ms"] > 0

    lines = dict(l.split(":", 1) for l in p.stdout.strip().splitlines())
    assert list(lines) == ["Tolerances", "Completenesses", "Accuracies", "F1-scores"]
    assert [float(x) for x in lines["Tolerances"].split()] == tol
    acc = [w / want["accuracy"]["n"] for w in want["accuracy"]["within"]]
    comp = [w / want["completeness"]["n"] for w in want["completeness"]["within"]]
    f1 = [2 * a * c / (a + c) if a + c > 0 else 0.0 for a, c in zip(acc, comp)]
    assert lines["Accuracies"].split() == ["%.6f" % a for a in acc]
    assert lines["Completenesses"].split() == ["%.6f" % c for c in comp]
    assert lines["F1-scores"].split() == ["%.6f" % f for f in f1]
    assert m["f1"] == pytest.approx(f1, rel=1e-12)
