"""The host side of `apd_eval`'s scanner mode, without a GPU: the MeshLab project reader and the
coloured-cloud writer through libapdhost.so, apd_eval_cube_cameras (host only), the option conflicts
and unreadable inputs of the new mode (exit 2 before a device is touched), --help, and the exports."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import apd_abi as A
from eval_lib import APD_EVAL, HOST, f32, ply_apd_layout, ply_gt_layout, same_bits
from protocol_lib import CUBE_R, cube_cameras_ref, in_view_ref, mlp_text, read_ply_xyz_rgb, to_world_ref

NO_GPU = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
NEW_SYMBOLS = ["apd_eval_cube_cameras", "apd_eval_free_gap", "apd_eval_voxel_scores", "apd_eval_get_protocol_timing"]
HOST_LIB = os.path.join(HOST, "build", "libapdhost.so")
IDENTITY = np.eye(4)
ANGLE = 0.3  # a rotation about z plus a translation: not representable in float32
POSE = np.array([[np.cos(ANGLE), -np.sin(ANGLE), 0, 0.25], [np.sin(ANGLE), np.cos(ANGLE), 0, -1.5], [0, 0, 1, 0.1],
                 [0, 0, 0, 1]])


def run_eval(*args):
    return subprocess.run([APD_EVAL, *map(str, args)], capture_output=True, text=True, timeout=120, env=NO_GPU)


@pytest.fixture(scope="module")
def host():
    A.torch_runtime_first()  # libapdhost.so links libapd_hip.so
    lib = C.CDLL(HOST_LIB)
    lib.apdhost_read_mlp.restype = C.c_long
    lib.apdhost_read_mlp.argtypes = [C.c_char_p, C.c_void_p, C.c_long, C.c_char_p, C.c_long, C.c_char_p, C.c_long]
    lib.apdhost_read_mlp_scan.restype = C.c_long
    lib.apdhost_read_mlp_scan.argtypes = [C.c_char_p, C.c_long, C.c_void_p, C.c_long, C.c_void_p, C.c_char_p, C.c_long]
    lib.apdhost_read_ply_xyz.restype = C.c_long
    lib.apdhost_read_ply_xyz.argtypes = [C.c_char_p, C.c_void_p, C.c_long, C.c_char_p, C.c_long]
    lib.apdhost_write_ply_xyz_rgb.restype = C.c_int
    lib.apdhost_write_ply_xyz_rgb.argtypes = [C.c_char_p, C.c_void_p, C.c_void_p, C.c_long]
    return lib


def read_mlp(lib, path, cap=8):
    """(list of (ply path, 4x4 float64)) or the error message"""
    mats = np.zeros((cap, 16), np.float64)
    paths, err = C.create_string_buffer(1 << 14), C.create_string_buffer(1024)
    n = lib.apdhost_read_mlp(str(path).encode(), mats.ctypes.data, cap, paths, len(paths), err, len(err))
    if n < 0:
        return err.value.decode()
    names = paths.value.decode().split("\n")
    assert len(names) == n
    return [(names[i], mats[i].reshape(4, 4).copy()) for i in range(n)]


def read_scan(lib, path, index, cap=4096):
    out, origin, err = np.zeros((cap, 3), f32), np.zeros(3, f32), C.create_string_buffer(1024)
    n = lib.apdhost_read_mlp_scan(str(path).encode(), index, out.ctypes.data, out.size, origin.ctypes.data, err, len(err))
    return err.value.decode() if n < 0 else (out[:n].copy(), origin)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("protocol_host")
    rng = np.random.default_rng(3)
    os.makedirs(d / "scans")
    pts = [rng.uniform(-2, 2, (300, 3)).astype(f32), rng.uniform(-2, 2, (200, 3)).astype(f32)]
    (d / "a.ply").write_bytes(ply_apd_layout(pts[0], rng))
    (d / "scans" / "b.ply").write_bytes(ply_gt_layout(pts[1]))
    (d / "rec.ply").write_bytes(ply_apd_layout(rng.uniform(-2, 2, (100, 3)).astype(f32)))
    (d / "one.mlp").write_text(mlp_text([("a.ply", IDENTITY)]))
    (d / "two.mlp").write_text(mlp_text([("a.ply", IDENTITY), ("scans/b.ply", POSE)]))
    (d / "split.mlp").write_text(mlp_text([("scans/b.ply", POSE)], numbers_per_line=3))
    (d / "oneline.mlp").write_text(mlp_text([("a.ply", POSE)], numbers_per_line=16))
    (d / "absolute.mlp").write_text(mlp_text([(str(d / "scans" / "b.ply"), POSE)]))
    fifteen = " ".join(["1 0 0 0", "0 1 0 0", "0 0 1 0", "0 0 0"])
    bad = {"empty.mlp": mlp_text([]), "no_matrix.mlp": mlp_text([("a.ply", IDENTITY), ("scans/b.ply", None)]),
           "fifteen.mlp": mlp_text([("a.ply", fifteen)]), "seventeen.mlp": mlp_text([("a.ply", fifteen + " 1 1")]),
           "word.mlp": mlp_text([("a.ply", "1 0 0 0 0 1 0 0 0 0 one 0 0 0 0 1")]),
           "nan.mlp": mlp_text([("a.ply", "1 0 0 0 0 1 0 0 0 0 nan 0 0 0 0 1")]),
           "trailing.mlp": mlp_text([("a.ply", "1 0 0 0 0 1 0 0 0 0 1x 0 0 0 0 1")]),
           "last_row.mlp": mlp_text([("a.ply", "1 0 0 0 0 1 0 0 0 0 1 0 0 0 0.5 1")]),
           "last_row_w.mlp": mlp_text([("a.ply", "1 0 0 0 0 1 0 0 0 0 1 0 0 0 0 2")]),
           "no_ply.mlp": mlp_text([("a.ply", IDENTITY), ("scans/missing.ply", POSE)])}
    for name, text in bad.items():
        (d / name).write_text(text)
    return d, pts


# ---- read_mlp -----------------------------------------------------------------------------------------

def test_read_mlp_accepts(host, files):
    d, pts = files
    one = read_mlp(host, d / "one.mlp")
    assert len(one) == 1 and one[0][0] == str(d / "a.ply") and np.array_equal(one[0][1], IDENTITY)
    two = read_mlp(host, d / "two.mlp")
    assert [n for n, _ in two] == [str(d / "a.ply"), str(d / "scans" / "b.ply")]
    assert np.array_equal(two[0][1], IDENTITY) and np.array_equal(two[1][1], POSE)  # %.17g round-trips doubles
    for name, ply in (("split.mlp", "scans/b.ply"), ("oneline.mlp", "a.ply")):
        got = read_mlp(host, d / name)
        assert len(got) == 1 and got[0][0] == str(d / ply) and np.array_equal(got[0][1], POSE)
    assert read_mlp(host, d / "absolute.mlp")[0][0] == str(d / "scans" / "b.ply")


def test_mlp_points_are_transformed_in_double_and_rounded_once(host, files):
    d, pts = files
    got, origin = read_scan(host, d / "two.mlp", 0)
    assert same_bits(got, pts[0]) and np.array_equal(origin, [0, 0, 0])
    got, origin = read_scan(host, d / "two.mlp", 1)
    want, o = to_world_ref(pts[1], POSE)
    assert same_bits(got, want) and same_bits(origin, o) and same_bits(o, np.array([0.25, -1.5, 0.1], f32))
    # not the float32 evaluation: the pose is not representable in float32
    naive = (pts[1] @ POSE[:3, :3].astype(f32).T + POSE[:3, 3].astype(f32)).astype(f32)
    assert not same_bits(naive, want)
    got, _ = read_scan(host, d / "split.mlp", 0)  # a relative filename in a sub-directory
    assert same_bits(got, want)


@pytest.mark.parametrize("name,message", [
    ("nowhere.mlp", "cannot open"), ("empty.mlp", "no <MLMesh> in the project"),
    ("no_matrix.mlp", "has no <MLMatrix44>"), ("fifteen.mlp", "15 numbers in the matrix, 16 expected"),
    ("seventeen.mlp", "more than 16 numbers"), ("word.mlp", "'one' in the matrix is not a number"),
    ("nan.mlp", "'nan' in the matrix is not a number"), ("trailing.mlp", "'1x' in the matrix is not a number"),
    ("last_row.mlp", "last row of the matrix is not 0 0 0 1"), ("last_row_w.mlp", "last row of the matrix is not 0 0 0 1")])
def test_read_mlp_rejects(host, files, name, message):
    d, _ = files
    got = read_mlp(host, d / name)
    assert isinstance(got, str) and message in got and name in got, got
    # the command line decides the same on the host: exit 2, the same message, no device
    p = run_eval("--cloud", d / "rec.ply", "--gt_mlp", d / name)
    assert p.returncode == 2 and message in p.stderr and "device" not in p.stderr and p.stdout == "", (p.stdout, p.stderr)


def test_missing_scan_ply_is_rejected(host, files):
    d, _ = files
    assert len(read_mlp(host, d / "no_ply.mlp")) == 2  # the project itself is well formed
    got = read_scan(host, d / "no_ply.mlp", 1)
    assert isinstance(got, str) and "cannot open" in got and "missing.ply" in got
    p = run_eval("--cloud", d / "rec.ply", "--gt_mlp", d / "no_ply.mlp", "--json", d / "o.json")
    assert p.returncode == 2 and "missing.ply" in p.stderr and "device" not in p.stderr and p.stdout == ""
    assert not (d / "o.json").exists()


# ---- write_ply_xyz_rgb ----------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [0, 1, 7, 70000])
def test_coloured_cloud_round_trip(host, tmp_path, n):
    rng = np.random.default_rng(n)
    xyz = rng.normal(0, 3, (n, 3)).astype(f32)
    if n > 4:
        xyz[2] = [np.nan, np.inf, -np.inf]  # written as they are
    rgb = rng.integers(0, 256, (n, 3)).astype(np.uint8)
    path = tmp_path / "c.ply"
    assert host.apdhost_write_ply_xyz_rgb(str(path).encode(), xyz.ctypes.data, rgb.ctypes.data, n) == 0
    assert os.path.getsize(path) == len(open(path, "rb").read().split(b"end_header\n")[0]) + 11 + 15 * n
    p, c = read_ply_xyz_rgb(path)
    assert same_bits(p, xyz) and np.array_equal(c, rgb)
    back = np.zeros((max(n, 1), 3), f32)
    err = C.create_string_buffer(256)
    assert host.apdhost_read_ply_xyz(str(path).encode(), back.ctypes.data, back.size, err, len(err)) == n
    assert same_bits(back[:n], xyz)
    assert host.apdhost_write_ply_xyz_rgb(str(tmp_path / "no" / "dir.ply").encode(), xyz.ctypes.data, rgb.ctypes.data, n) == -1


# ---- the reader and the writer under sanitizers ----------------------------------------------------------

def test_mlp_reader_under_sanitizers(files, tmp_path):
    """A stand-alone program built with AddressSanitizer + UBSan reads every project of the fixture,
    whole, truncated and with flipped bytes: each is read or rejected, none is read out of bounds."""
    d, _ = files
    r = subprocess.run(["make", "-C", HOST, "sanitize-mlp"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    rng = np.random.default_rng(4)
    names = sorted(p for p in os.listdir(d) if p.endswith(".mlp"))
    paths = []
    for name in names:
        # absolute PLY paths, so that the variants written elsewhere still find their scans
        data = (d / name).read_text().replace('filename="a.ply"', 'filename="%s"' % (d / "a.ply")) \
                                     .replace('filename="scans/', 'filename="%s/scans/' % d).encode()
        variants = {"": data}
        for k, cut in enumerate(sorted(set(np.linspace(0, len(data) - 1, 25).astype(int).tolist()))):
            variants[".cut%d" % k] = data[:cut]
        for k in range(25):
            b = bytearray(data)
            for _ in range(int(rng.integers(1, 4))):
                b[int(rng.integers(0, len(b)))] = int(rng.integers(0, 256))
            variants[".flip%d" % k] = bytes(b)
        for suffix, blob in variants.items():
            (tmp_path / (name + suffix)).write_bytes(blob)
            paths.append(str(tmp_path / (name + suffix)))
    paths += [str(tmp_path), str(tmp_path / "none.mlp")]  # a directory, no such file
    (tmp_path / "tag_at_end.mlp").write_bytes(b"<MLMesh")
    (tmp_path / "open_tag.mlp").write_bytes(b'<MLMesh filename="a.ply"')
    (tmp_path / "open_matrix.mlp").write_bytes(b'<MLMesh filename="a.ply"><MLMatrix44>1 0 0 0')
    (tmp_path / "empty_name.mlp").write_bytes(b'<MLMesh filename=""><MLMatrix44>1 0 0 0 0 1 0 0 0 0 1 0 0 0 0 1</MLMatrix44>')
    paths += [str(tmp_path / n) for n in ("tag_at_end.mlp", "open_tag.mlp", "open_matrix.mlp", "empty_name.mlp")]
    env = dict(NO_GPU, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([os.path.join(HOST, "build-san", "mlp_corpus_main"), *paths], capture_output=True, text=True,
                       timeout=300, env=env)
    assert p.returncode == 0 and "runtime error" not in p.stderr and "Sanitizer" not in p.stderr, (p.stdout, p.stderr[-3000:])
    last = p.stdout.strip().splitlines()[-1]
    assert last.startswith("mlp corpus: ")
    read, rejected, clouds = [int(w) for w in last.replace(",", "").split() if w.isdigit()]
    assert read + rejected == len(paths) and read >= 6 and rejected > len(names) * 20 and clouds >= 7


# ---- cube_cameras ---------------------------------------------------------------------------------------

def test_cube_cameras_table_without_a_gpu():
    origin = np.array([0.3, -1.25, 7.0], f32)
    for size in (2, 8, 48, 2048, 16384):
        cams = A.cube_cameras(origin, size)
        assert len(cams) == 6
        for cam, rows, ref in zip(cams, CUBE_R, cube_cameras_ref(origin, size)):
            R = np.array(cam.R[:], f32).reshape(3, 3)
            assert np.array_equal(R, np.array(rows, f32)) and round(float(np.linalg.det(R.astype(np.float64)))) == 1
            assert np.array_equal(np.array(cam.t[:], f32), -(R.astype(np.float64) @ origin.astype(np.float64)))
            assert np.array_equal(np.array(cam.K[:], f32),
                                  np.array([size / 2, 0, size / 2 - 0.5, 0, size / 2, size / 2 - 0.5, 0, 0, 1], f32))
            assert (cam.width, cam.height) == (size, size)
            assert bytes(cam) == bytes(ref)  # c, depth_min, depth_max, interval, depth_num as make_cam leaves them
    # the forward axes are +X, -X, +Y, -Y, +Z, -Z
    fwd = [tuple(np.array(c.R[6:9], f32)) for c in A.cube_cameras((0, 0, 0), 8)]
    assert fwd == [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]


@pytest.mark.parametrize("size", [8, 48])
def test_cube_faces_cover_every_direction(size):
    rng = np.random.default_rng(size)
    origin = np.array([0.5, 0.3, -0.4], f32)
    pts = (origin + rng.normal(0, 1, (20000, 3)) * rng.uniform(0.5, 3, (20000, 1))).astype(f32)
    hits = sum(in_view_ref(pts, cam)[0].astype(int) for cam in A.cube_cameras(origin, size))
    assert hits.min() == 1 and hits.max() <= 3
    # a face spans exactly +-45 degrees up to rounding: the seams hold a share that shrinks with the size
    assert int((hits > 1).sum()) == {8: 2326, 48: 456}[size]


def test_cube_cameras_status_codes():
    lib = A.load_library()
    arr = (A.ApdCamera * 6)()
    o = np.array([0, 0, 0], f32)
    assert lib.apd_eval_cube_cameras(o.ctypes.data, 2, arr) == 0 and lib.apd_eval_cube_cameras(o.ctypes.data, 16384, arr) == 0
    for size in (1, 0, -8, 16385):
        assert lib.apd_eval_cube_cameras(o.ctypes.data, size, arr) == -1
    assert lib.apd_eval_cube_cameras(None, 8, arr) == -1 and lib.apd_eval_cube_cameras(o.ctypes.data, 8, None) == -1
    for bad in (np.nan, np.inf, -np.inf):
        for axis in range(3):
            b = o.copy()
            b[axis] = bad
            assert lib.apd_eval_cube_cameras(b.ctypes.data, 8, arr) == -1
    with pytest.raises(A.ApdError):
        A.cube_cameras((0, np.nan, 0), 8)
    with pytest.raises(A.ApdError):
        A.cube_cameras((0, 0, 0), 1)


# ---- command line -------------------------------------------------------------------------------------

def test_scanner_mode_option_conflicts(files, tmp_path):
    d, _ = files
    rec, mlp, out = d / "rec.ply", d / "two.mlp", tmp_path / "out"
    mode = ("--cloud", rec, "--gt_mlp", mlp)
    for args in [("--gt_mlp", mlp), (*mode, "--gt", d / "a.ply"), (*mode, "--dense_folder", d),
                 (*mode, "--render_gt", d / "a.ply", "--scan", d, "--out", out), (*mode, "--visible_views", 2),
                 (*mode, "--scan", d), (*mode, "--scan", d, "--visible_views", 1),
                 (*mode, "--cube_size", 1), (*mode, "--cube_size", 16385), (*mode, "--cube_size", "x"),
                 (*mode, "--voxel", 0), (*mode, "--voxel", -1), (*mode, "--splat", 17),
                 (*mode, "--max_dist", 0.1), (*mode, "--tolerances", "0.1,-1"), (*mode, "--occlusion_tol", 0.1),
                 ("--cloud", rec, "--gt", d / "a.ply", "--cube_size", 48),
                 ("--cloud", rec, "--gt", d / "a.ply", "--accuracy_cloud_out", out),
                 ("--cloud", rec, "--gt", d / "a.ply", "--completeness_cloud_out", out), ("--accuracy_cloud_out", out)]:
        p = run_eval(*args, "--json", tmp_path / "o.json")
        assert p.returncode == 2, (args, p.stdout, p.stderr)
        assert "device" not in p.stderr and p.stderr.startswith("apd_eval: ") and p.stdout == ""
    assert not out.exists() and not (tmp_path / "o.json").exists()


def test_unreadable_inputs_exit_2_before_any_device(files, tmp_path):
    d, _ = files
    (tmp_path / "bad.ply").write_bytes(b"ply\nformat ascii 1.0\nelement vertex 1\nproperty float x\nend_header\n0\n")
    (tmp_path / "bad_scan.mlp").write_text(mlp_text([(str(tmp_path / "bad.ply"), IDENTITY)]))
    (tmp_path / "far.mlp").write_text(mlp_text([(str(d / "a.ply"), "1 0 0 1e300 0 1 0 0 0 0 1 0 0 0 0 1")]))
    out = tmp_path / "out"
    for args in [("--cloud", tmp_path / "nowhere.ply", "--gt_mlp", d / "two.mlp"),
                 ("--cloud", tmp_path / "bad.ply", "--gt_mlp", d / "two.mlp"),
                 ("--cloud", d / "rec.ply", "--gt_mlp", tmp_path / "nowhere.mlp"),
                 ("--cloud", d / "rec.ply", "--gt_mlp", tmp_path),  # a directory opens but does not read
                 ("--cloud", d / "rec.ply", "--gt_mlp", tmp_path / "bad_scan.mlp"),
                 ("--cloud", d / "rec.ply", "--gt_mlp", tmp_path / "far.mlp")]:
        p = run_eval(*args, "--json", tmp_path / "o.json", "--accuracy_cloud_out", out)
        assert p.returncode == 2, (args, p.stdout, p.stderr)
        assert "device" not in p.stderr and len(p.stderr.strip()) > 20 and p.stdout == ""
    assert not out.exists() and not (tmp_path / "o.json").exists()


def test_a_valid_invocation_reaches_the_device(files, tmp_path):
    """Everything parses, so the tool goes on to the device and fails THERE (status 1, not 2) on a
    machine with no visible GPU; nothing is written."""
    d, _ = files
    p = run_eval("--cloud", d / "rec.ply", "--gt_mlp", d / "two.mlp", "--cube_size", 48, "--voxel", 0.25, "--splat", 0,
                 "--max_dist", 1, "--accuracy_cloud_out", tmp_path / "acc", "--completeness_cloud_out", tmp_path / "comp")
    assert p.returncode == 1 and "device" in p.stderr, (p.stdout, p.stderr)
    assert not (tmp_path / "acc").exists() and not (tmp_path / "comp").exists()


def test_help_lists_the_new_options():
    p = run_eval("--help")
    assert p.returncode == 0
    for word in ("--gt_mlp", "--cube_size", "--accuracy_cloud_out", "--completeness_cloud_out", "--voxel", "--splat",
                 "--max_dist", "--tolerances", "scanner mode", "unobserved", "NOT the ETH3D tool", "unpinned",
                 "Completenesses:", "Accuracies:", "F1-scores:"):
        assert word in p.stdout, word


def test_library_exports_the_protocol_entries():
    assert all(s in A.EVAL_EXPORTS for s in NEW_SYMBOLS)
    lib = A.load_library()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s), s
    # a NULL context is refused without touching a device
    assert lib.apd_eval_free_gap(None, 0, None, 0, None, None, None) == -1
    assert lib.apd_eval_voxel_scores(None, 0, None, 0.1, None, None, 0, None, None, None, None, None) == -1
    assert lib.apd_eval_get_protocol_timing(None, None, None) == -1
