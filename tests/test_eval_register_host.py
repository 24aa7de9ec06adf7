"""The host twins of include/apd_eval.h's crop / nearest / registration calls against the numpy
restatement of tests/register_lib.py, the crop-volume and matrix readers of `apd_eval --tat_gt`, and
those readers under AddressSanitizer + UndefinedBehaviorSanitizer (a stand-alone program, run
directly). No GPU."""
import json
import os
import subprocess

import numpy as np
import pytest

import apd_abi as A
import register_lib as RL
from eval_lib import APD_EVAL, HOST, f32, same_bits

SAN_BIN = os.path.join(HOST, "build-san", "tat_corpus_main")
NO_GPU = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
SIZES = [1, 3, 1023, 1024, 1025, 5000]

CONVEX = np.array([[-2.0, -1.5], [0.0, -2.5], [2.0, -1.5], [2.5, 0.5], [1.0, 2.0], [-1.0, 2.25], [-2.5, 0.5],
                   [-2.75, -0.5]])
# 8 vertices, one reflex (the notch at (0, 0.25))
CONCAVE = np.array([[-2.0, -2.0], [2.0, -2.0], [2.5, 0.0], [2.0, 2.0], [0.0, 0.25], [-2.0, 2.0], [-2.5, 0.5],
                    [-2.25, -1.0]])
POLYGONS = {"convex": CONVEX, "concave": CONCAVE}
SKEW = RL.similarity(7.0, [1.0, -2.0, 0.5], 1.1, [0.2, -0.1, 0.3])


@pytest.fixture(scope="module")
def lib():
    return A.load_library()


def crop_points(axis, poly, lo, hi, seed=5):
    """5 000 seeded points plus the edge cases: v equal to a vertex's v, w on both bounds, a NaN."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-3.5, 3.5, (5000, 3)).astype(f32)
    ui, vi, wi = RL.UVW[axis]
    k = 0
    for V in poly[:, 1]:  # v exactly a vertex's v (all vertex coordinates are fp32-exact), u swept across
        for u in np.linspace(-3.0, 3.0, 13):
            x[k, ui], x[k, vi] = u, V
            k += 1
    for U, V in poly:  # the vertices themselves
        x[k, ui], x[k, vi], x[k, wi] = U, V, 0.0
        k += 1
    x[k:k + 40, wi] = lo
    x[k + 40:k + 80, wi] = hi
    x[k + 80:k + 120, wi] = np.nextafter(f32(hi), f32(np.inf))
    x[k + 120] = [np.nan, 0.0, 0.0]
    x[k + 121, vi] = np.inf
    return x


@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("name", sorted(POLYGONS))
@pytest.mark.parametrize("with_T", [False, True])
def test_crop_host_equals_the_numpy_rule(lib, axis, name, with_T):
    poly, lo, hi = POLYGONS[name], -1.25, 1.5
    x = crop_points(axis, poly, lo, hi)
    T = SKEW if with_T else None
    want = RL.crop_ref(x, axis, lo, hi, poly, T)
    got = A.crop_volume_host(x, axis, lo, hi, poly, T, lib=lib)
    assert 200 < len(want) < 4800
    assert np.array_equal(got, want)
    if not with_T:
        wi = RL.UVW[axis][2]
        kept = x[got]
        assert (kept[:, wi] == f32(lo)).sum() > 5 and (kept[:, wi] == f32(hi)).sum() > 5  # the bounds are kept
        assert not (kept[:, wi] > hi).any() and np.isfinite(kept).all()
        # the > asymmetry: on a vertex's own v the rule still decides, and numpy agrees point by point
        vi = RL.UVW[axis][1]
        on_vertex_v = np.isin(x[:, vi], poly[:, 1].astype(f32))
        assert on_vertex_v.sum() >= 100 and 0 < np.isin(np.flatnonzero(on_vertex_v), got).sum() < on_vertex_v.sum()


def test_crop_host_rejects_bad_arguments(lib):
    x = np.zeros((4, 3), f32)
    for kw in [dict(polygon=CONVEX[:2]), dict(axis=3), dict(axis_min=np.nan),
               dict(polygon=np.array([[0, 0], [1, np.inf], [1, 1.0]]))]:
        args = dict(axis=0, axis_min=-1.0, axis_max=1.0, polygon=CONVEX)
        args.update(kw)
        with pytest.raises(A.ApdError, match="APD_EINVAL"):
            A.crop_volume_host(x, lib=lib, **args)
    assert len(A.crop_volume_host(np.zeros((0, 3), f32), 0, -1.0, 1.0, CONVEX, lib=lib)) == 0


def test_nearest_host_ties_go_to_the_lowest_index(lib):
    rng = np.random.default_rng(8)
    base = rng.uniform(-1, 1, (300, 3)).astype(f32)
    t = np.concatenate([base, base[::-1], base[:50]])  # every point two or three times
    t[7] = np.nan
    q = np.concatenate([base + f32(1e-3), base, rng.uniform(-3, 3, (200, 3)).astype(f32), [[np.nan, 0, 0]]]).astype(f32)
    for md in (0.05, 0.5, np.inf, 0.0):  # grid, grid, brute force, brute force
        dist, idx = A.nearest_host(t, q, md, lib=lib)
        wd, wi, _ = RL.nearest_ref(t, q, md)
        assert same_bits(dist, wd) and np.array_equal(idx, wi)
    dist, idx = A.nearest_host(t, base, 0.5, lib=lib)
    first = np.arange(300)
    first[7] = 592  # target 7 is not finite: its first finite duplicate is base[::-1][292]
    assert np.array_equal(idx, first) and (dist == 0).all()
    dist, idx = A.nearest_host(np.zeros((0, 3), f32), base, 0.5, lib=lib)
    assert (idx == -1).all() and np.isinf(dist).all()


def moments_case(n, seed=3):
    rng = np.random.default_rng(seed + n)
    src = rng.uniform(-4, 4, (n, 3)).astype(f32)
    tgt = RL.transform_ref(src, RL.similarity(1.0, [1, 1, 0], 1.0, [0.01, 0, 0]))
    tgt = np.concatenate([tgt, tgt[: n // 3]])  # duplicates: ties
    far = rng.random(n) < 0.2
    src[far] += f32(100.0)  # no correspondence
    if n > 3:
        src[2] = np.nan
    return src, tgt


@pytest.mark.parametrize("n", SIZES)
def test_host_sums_are_bit_equal_to_the_numpy_tree(lib, n):
    src, tgt = moments_case(n)
    for T in (None, SKEW @ np.linalg.inv(SKEW) @ RL.similarity(0.5, [0, 0, 1], 1.001, [0, 0.01, 0])):
        got = A.register_sums_host(tgt, src, 0.3, T, lib=lib)
        want = RL.sums_ref(tgt, src, 0.3, T)
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (got, want)
        if n >= 1023:
            assert 0 < got[0] < got[18] <= n
        if n == 5000:  # the order is part of the contract: a left-to-right sum of the same terms gives other bits
            plain = np.cumsum(RL.terms_ref(tgt, src, 0.3, T), axis=0)[-1]
            assert (plain != got).any() and np.allclose(plain, got, rtol=1e-12)


@pytest.mark.parametrize("with_scale", [1, 0])
def test_registration_recovers_a_known_similarity(lib, with_scale):
    rng = np.random.default_rng(17)
    src = rng.uniform(-4, 4, (3000, 3)).astype(f32)
    truth = RL.similarity(5.0, [0.3, -0.5, 0.8], 1.02 if with_scale else 1.0, [0.05, 0.05, 0.05])
    tgt = RL.transform_ref(src, truth)
    T, info, st = A.register_host(tgt, src, 0.5, None, with_scale, 30, 0.0, 0.0, lib=lib)
    print("max |T - truth| =", np.abs(T - truth).max(), info)
    assert st == 0 and info["iterations"] <= 30
    # fp32 coordinate rounding 2^-24 * 4 = 2.4e-7, a margin of about 40 for the accumulated solve
    assert np.abs(T - truth).max() < 1e-5
    assert info["n_corr"] == 3000 and info["fitness"] == 1.0 and info["rmse"] < 1e-5
    # the numpy loop (numpy.linalg.svd in place of the Jacobi SVD) ends at the same place
    Tn, info_n, ok = RL.register_ref(tgt, src, 0.5, None, with_scale, 30, 0.0, 0.0)
    assert ok and np.abs(Tn - T).max() < 1e-9 and info_n["n_corr"] == info["n_corr"]


def test_registration_stops_on_the_open3d_rule(lib):
    rng = np.random.default_rng(18)
    src = rng.uniform(-4, 4, (1500, 3)).astype(f32)
    tgt = RL.transform_ref(src, RL.similarity(1.0, [0, 0, 1], 1.0, [0.02, 0, 0]))
    T, info, st = A.register_host(tgt, src, 0.5, None, 0, 30, 1e-6, 1e-6, lib=lib)
    assert st == 0 and 1 <= info["iterations"] < 30


def test_registration_degenerate_inputs(lib):
    rng = np.random.default_rng(19)
    src = rng.uniform(-1, 1, (100, 3)).astype(f32)
    tgt = src[:2] + f32(0.01)  # two correspondences at the most
    T0 = RL.similarity(0.0, [0, 0, 1], 1.0, [0.001, 0, 0])
    T, info, st = A.register_host(tgt + f32(50), src, 0.05, T0, 1, 10, 0.0, 0.0, lib=lib)
    assert A.STATUS[st] == "APD_ESTATE" and np.array_equal(T, T0) and info["n_corr"] == 0 and info["n_finite"] == 100
    T, info, st = A.register_host(tgt, src, 0.05, T0, 1, 10, 0.0, 0.0, lib=lib)
    assert A.STATUS[st] == "APD_ESTATE" and np.array_equal(T, T0) and info["n_corr"] == 2 and info["iterations"] == 0
    T, info, st = A.register_host(tgt, np.zeros((0, 3), f32), 0.05, None, 1, 10, 0.0, 0.0, lib=lib)
    assert A.STATUS[st] == "APD_ESTATE" and np.array_equal(T, np.eye(4)) and info["n_finite"] == 0 and info["fitness"] == 0
    T, info, st = A.register_host(np.zeros((0, 3), f32), src, 0.05, None, 1, 10, 0.0, 0.0, lib=lib)
    assert A.STATUS[st] == "APD_ESTATE" and info["n_corr"] == 0
    for kw in [dict(max_corr=0.0), dict(max_iter=0), dict(max_iter=1001), dict(eps_rmse=-1.0), dict(T0=np.full(16, np.nan))]:
        args = dict(max_corr=0.1, T0=None, with_scale=1, max_iter=5, eps_fitness=0.0, eps_rmse=0.0)
        args.update(kw)
        with pytest.raises(A.ApdError, match="APD_EINVAL"):
            A.register_host(tgt, src, lib=lib, **args)


def test_transform_host_matches_numpy(lib):
    rng = np.random.default_rng(2)
    x = rng.uniform(-50, 50, (1000, 3)).astype(f32)
    assert same_bits(A.transform_host(x, SKEW, lib=lib), RL.transform_ref(x, SKEW))
    assert same_bits(A.transform_host(x, None, lib=lib), x)


def test_new_symbols_are_exported(lib):
    new = ["apd_eval_crop_volume", "apd_eval_crop_volume_host", "apd_eval_nearest", "apd_eval_nearest_host",
           "apd_eval_transform", "apd_eval_transform_host", "apd_eval_register", "apd_eval_register_host",
           "apd_eval_register_sums", "apd_eval_register_sums_host", "apd_eval_get_register_timing"]
    assert all(s in A.EVAL_EXPORTS and hasattr(lib, s) for s in new)
    assert A.REG_BLOCK == RL.REG_BLOCK == 1024 and C_sizeof_info() == 40


def C_sizeof_info():
    import ctypes
    return ctypes.sizeof(A.ApdEvalRegInfo)


# ---- the readers of `apd_eval --tat_gt` ------------------------------------------------------------------

CROP = {"axis_max": 1.5, "axis_min": -1.25, "orthogonal_axis": "Y",
        "bounding_polygon": [[u, 0.0, v] for u, v in CONVEX.tolist()]}


def run_eval(*args):
    return subprocess.run([APD_EVAL, *map(str, args)], capture_output=True, text=True, timeout=120, env=NO_GPU)


def good_crop_text():
    return json.dumps(dict(CROP, class_name="SelectionPolygonVolume", version_major=1, version_minor=0,
                           nested={"a": [1, {"b": None}], "s": 'x"y\\'}, flag=True), indent=1)


def bad_inputs():
    """name -> (crop text, matrix text); each must be rejected with a message."""
    good_m = "1 0 0 0.5\n0 1 0 0\n0 0 1 0\n0 0 0 1\n"
    g = good_crop_text()

    def crop(**kw):
        return json.dumps(dict(CROP, **kw))
    return {
        "crop_truncated": (g[: len(g) // 2], good_m),
        "crop_empty": ("", good_m),
        "crop_wrong_type_axis_max": (crop(axis_max="high"), good_m),
        "crop_wrong_type_axis": (crop(orthogonal_axis=1), good_m),
        "crop_bad_axis_name": (crop(orthogonal_axis="W"), good_m),
        "crop_two_vertices": (crop(bounding_polygon=CROP["bounding_polygon"][:2]), good_m),
        "crop_vertex_of_two": (crop(bounding_polygon=[[0, 0], [1, 0], [1, 1]]), good_m),
        "crop_non_numeric_vertex": (crop(bounding_polygon=[[0, 0, "a"], [1, 0, 0], [1, 0, 1]]), good_m),
        "crop_missing_key": (json.dumps({k: v for k, v in CROP.items() if k != "axis_min"}), good_m),
        "crop_not_an_object": ("[1, 2, 3]", good_m),
        "crop_trailing_garbage": (g + " x", good_m),
        "crop_huge_number": (g.replace("1.5", "1e999"), good_m),
        "crop_deep_nesting": ('{"x": ' + "[" * 5000 + "]" * 5000 + ", " + g[1:], good_m),
        "matrix_3x4": (g, "1 0 0 0\n0 1 0 0\n0 0 1 0\n"),
        "matrix_17": (g, good_m + "1\n"),
        "matrix_non_numeric": (g, good_m.replace("0.5", "half")),
        "matrix_nan": (g, good_m.replace("0.5", "nan")),
        "matrix_bad_last_row": (g, "1 0 0 0\n0 1 0 0\n0 0 1 0\n0 0 1 1\n"),
        "matrix_empty": (g, ""),
        "matrix_hex_float": (g, good_m.replace("0.5", "0x1p-1")),
        "matrix_leading_dot": (g, good_m.replace("0.5", ".5")),
    }


def huge_inputs():
    """name -> (crop text, matrix text, what the message must say): the bounds on what the readers allocate.
    Built on demand: each is megabytes."""
    good_m = "1 0 0 0.5\n0 1 0 0\n0 0 1 0\n0 0 0 1\n"
    head = '{"axis_max": 1, "axis_min": 0, "orthogonal_axis": "Z", "bounding_polygon": ['
    return {
        "crop_huge_count": lambda: (head + "[0,0,0]," * (1 << 20) + "[0,0,0]]}", good_m, "more than 2^20"),
        "crop_over_64MiB": lambda: (good_crop_text() + " " * (64 << 20), good_m, "larger than 64 MiB"),
        "matrix_over_1MiB": lambda: (good_crop_text(), good_m + " " * (1 << 20), "larger than 1 MiB"),
    }


@pytest.fixture(scope="module")
def tat_files(tmp_path_factory):
    import synth
    d = tmp_path_factory.mktemp("tat")
    rng = np.random.default_rng(4)
    synth.write_ply(str(d / "rec.ply"), rng.uniform(-1, 1, (50, 3)).astype(f32))
    (d / "crop.json").write_text(good_crop_text())
    (d / "trans.txt").write_text("1 0 0 0.5\n0 1 0 0\n0 0 1 0\n0 0 0 1\n")
    return d


def test_valid_crop_and_matrix_get_past_the_readers(tat_files):
    """Everything parses, so the tool goes on to the device and fails there (status 1, not 2)."""
    d = tat_files
    p = run_eval("--cloud", d / "rec.ply", "--tat_gt", d / "rec.ply", "--tat_crop", d / "crop.json", "--tau", 0.01,
                 "--tat_trans", d / "trans.txt", "--init_trans", d / "trans.txt")
    assert p.returncode == 1 and "device" in p.stderr, (p.stdout, p.stderr)


def test_readers_round_trip(tat_files, tmp_path):
    """--tat_dump prints what the readers understood, as JSON, without touching a device."""
    d = tat_files
    T = RL.similarity(3.0, [1, 2, 3], 1.25, [0.1, -2.5e-7, 1e10])
    RL.write_matrix(tmp_path / "m.txt", T)
    RL.write_crop_json(tmp_path / "c.json", CROP)
    p = run_eval("--tat_dump", "--tat_crop", tmp_path / "c.json", "--tat_trans", tmp_path / "m.txt")
    assert p.returncode == 0, (p.stdout, p.stderr)
    got = json.loads(p.stdout)
    assert np.array_equal(np.array(got["trans"]).reshape(4, 4), T)
    assert got["crop"]["orthogonal_axis"] == "Y" and got["crop"]["axis_min"] == -1.25 and got["crop"]["axis_max"] == 1.5
    assert got["crop"]["bounding_polygon"] == CROP["bounding_polygon"]
    p = run_eval("--tat_dump", "--tat_crop", d / "crop.json")  # unknown keys of any shape are skipped
    assert p.returncode == 0 and json.loads(p.stdout)["crop"]["bounding_polygon"] == CROP["bounding_polygon"]


@pytest.mark.parametrize("name", sorted(bad_inputs()))
def test_malformed_crop_or_matrix_is_rejected_on_the_host(tat_files, tmp_path, name):
    crop, mat = bad_inputs()[name]
    (tmp_path / "c.json").write_text(crop)
    (tmp_path / "m.txt").write_text(mat)
    d = tat_files
    p = run_eval("--cloud", d / "rec.ply", "--tat_gt", d / "rec.ply", "--tat_crop", tmp_path / "c.json", "--tau", 0.01,
                 "--tat_trans", tmp_path / "m.txt", "--json", tmp_path / "o.json")
    assert p.returncode == 2, (p.stdout, p.stderr)
    bad = str(tmp_path / ("c.json" if name.startswith("crop") else "m.txt"))
    assert bad in p.stderr and len(p.stderr.strip()) > len(bad) + 10 and "device" not in p.stderr
    assert not (tmp_path / "o.json").exists()


@pytest.mark.parametrize("name", sorted(huge_inputs()))
def test_oversized_crop_or_matrix_is_rejected_on_the_host(tat_files, tmp_path, name):
    crop, mat, message = huge_inputs()[name]()
    (tmp_path / "c.json").write_text(crop)
    (tmp_path / "m.txt").write_text(mat)
    d = tat_files
    p = run_eval("--cloud", d / "rec.ply", "--tat_gt", d / "rec.ply", "--tat_crop", tmp_path / "c.json", "--tau", 0.01,
                 "--tat_trans", tmp_path / "m.txt", "--json", tmp_path / "o.json")
    assert p.returncode == 2, (p.stdout, p.stderr)
    bad = str(tmp_path / ("c.json" if name.startswith("crop") else "m.txt"))
    assert bad in p.stderr and message in p.stderr and "device" not in p.stderr, p.stderr
    assert not (tmp_path / "o.json").exists()
    if name == "crop_huge_count":  # exactly 2^20 vertices are still read
        (tmp_path / "c.json").write_text(crop.replace("[0,0,0],", "", 1))
        p = run_eval("--tat_dump", "--tat_crop", tmp_path / "c.json")
        assert p.returncode == 0 and p.stdout.count("[0, 0, 0]") == 1 << 20, p.stderr


def test_tat_bad_arguments(tat_files):
    d = tat_files
    base = ["--cloud", d / "rec.ply", "--tat_gt", d / "rec.ply", "--tat_crop", d / "crop.json"]
    for extra, message in [([], "needs --cloud, --tat_gt, --tat_crop and --tau"), (["--tau", "0"], "bad --tau 0"),
                           (["--tau", "x"], "bad --tau x"),
                           (["--tau", "0.01", "--refine_stages", "0.01"], "bad refinement stage '0.01'"),
                           (["--tau", "0.01", "--refine_stages", "0.01:-1"], "bad refinement stage '0.01:-1'"),
                           (["--tau", "0.01", "--refine_stages", ",".join(["0.01:0.1"] * 17)], "1 to 16 stages"),
                           (["--tau", "0.01", "--gt", d / "rec.ply"], "--tat_gt excludes the other modes"),
                           (["--tau", "0.01", "--voxel", "0.01"], "--tat_gt excludes the other modes"),
                           (["--tau", "0.01", "--no_refine", "--refine_stages", "0.01:0.1"],
                            "--no_refine with --refine_stages")]:
        p = run_eval(*base, *extra)
        assert p.returncode == 2 and message in p.stderr, (extra, p.stdout, p.stderr)
    p = run_eval("--cloud", d / "rec.ply", "--tat_gt", d / "rec.ply", "--tau", "0.01")
    assert p.returncode == 2 and "needs --cloud, --tat_gt, --tat_crop and --tau" in p.stderr, p.stderr
    for flag in (["--no_scale"], ["--no_refine"], ["--tau", "0.01"], ["--tat_crop", d / "crop.json"],
                 ["--aligned_cloud_out", d / "a.ply"]):  # a TaT flag without --tat_gt
        p = run_eval("--cloud", d / "rec.ply", "--gt", d / "rec.ply", *flag)
        assert p.returncode == 2 and "without --tat_gt" in p.stderr, (flag, p.stderr)


def test_readers_under_sanitizers(tat_files, tmp_path):
    r = subprocess.run(["make", "-C", HOST, "sanitize-tat"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    rng = np.random.default_rng(1)
    blobs = {"good.json": good_crop_text().encode(), "good.txt": b"1 0 0 0.5\n0 1 0 0\n0 0 1 0\n0 0 0 1\n"}
    for name, (crop, mat) in bad_inputs().items():
        blobs[name + ".json"] = crop.encode()
        blobs[name + ".txt"] = mat.encode()
    blobs["huge_count.json"] = ('{"axis_max": 1, "axis_min": 0, "orthogonal_axis": "Z", "bounding_polygon": [' +
                                ",".join(["[0,0,0]"] * 300000) + "]}").encode()
    blobs["huge_matrix.txt"] = b"1 " * 400000
    for name, make in huge_inputs().items():
        crop, mat, _ = make()
        if name.startswith("crop"):
            blobs[name + ".json"] = crop.encode()
        else:
            blobs[name + ".txt"] = mat.encode()
    blobs["long_token.txt"] = b"1" * 100000
    files = []
    for name, data in blobs.items():
        variants = {"": data}
        if data and len(data) < 100000:
            for k, cut in enumerate(sorted(set(np.linspace(0, len(data) - 1, 25).astype(int).tolist()))):
                variants[f".cut{k}"] = data[:cut]
            for k in range(25):
                b = bytearray(data)
                for _ in range(int(rng.integers(1, 6))):
                    b[int(rng.integers(0, len(b)))] = int(rng.integers(0, 256))
                variants[f".flip{k}"] = bytes(b)
        for suffix, blob in variants.items():
            stem, ext = os.path.splitext(name)
            p = tmp_path / (stem + suffix + ext)
            p.write_bytes(blob)
            files.append(str(p))
    files += [str(tmp_path), str(tmp_path / "none.json"), str(tmp_path / "none.txt")]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([SAN_BIN, *files], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    read, rejected = (int(x) for x in r.stdout.split("tat corpus:")[1].replace("read,", "").replace("rejected", "").split())
    assert read + rejected == len(files) and read >= 2 and rejected > len(bad_inputs()) + len(huge_inputs())
    # the whole files: exactly the malformed and oversized ones are rejected
    whole = [f for f in files if ".cut" not in f and ".flip" not in f]
    bad = {n + (".json" if n.startswith("crop") else ".txt") for n in list(bad_inputs()) + list(huge_inputs())}
    bad |= {"huge_matrix.txt", "long_token.txt", "none.json", "none.txt", os.path.basename(str(tmp_path))}
    assert bad <= {os.path.basename(f) for f in whole}
    r = subprocess.run([SAN_BIN, *whole], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "tat corpus: %d read, %d rejected" % (len(whole) - len(bad), len(bad)) in r.stdout, \
        (r.stdout, r.stderr[-2000:])
