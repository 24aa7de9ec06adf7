"""The undistortion of include/apd_prep.h without a GPU: apd_prep_undistort_bgr8_host, apd_prep_atan_c
and apd_prep_undistort_xy against known answers, the numpy restatement in tests/undistort_lib.py (bit
for bit), libm's atan and an analytic image; the COLMAP reader with distorted models; `apd_prepare`
without a device; and the host entries under ASan + UBSan as a stand-alone program."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import apd_abi as A
import prep_lib as P
import undistort_lib as U

HOST = os.path.join(A.HERE, "host")
HOST_LIB = os.path.join(HOST, "build", "libapdhost.so")
APD_PREPARE = os.path.join(HOST, "build", "apd_prepare")
NO_GPU = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
EINVAL = -1


@pytest.fixture(scope="module")
def lib():
    return A.load_library()


@pytest.fixture(scope="module")
def image():
    return np.random.default_rng(31).integers(0, 256, (48, 64, 3)).astype(np.uint8)


def test_exports(lib):
    assert [s for s in A.PREP_UNDISTORT_EXPORTS if not hasattr(lib, s)] == []
    nm = subprocess.run(["nm", "-D", "--defined-only", A.LIB_PATH], capture_output=True, text=True).stdout
    assert all((" T " + s) in nm for s in A.PREP_UNDISTORT_EXPORTS)
    assert {m: v for m, v in A.PREP_CAMERA_MODELS.items()} == U.MODELS


# ---- 1. known answers ----------------------------------------------------------------------------------

def test_pinhole_known_answers(lib, image):
    # f a power of two and a half-integer-free principal point: every source coordinate is exact
    p = [64.0, 64.0, 32.0, 24.0]
    assert np.array_equal(A.prep_undistort_host(image, "PINHOLE", p, lib=lib), image)
    assert np.array_equal(A.prep_undistort_host(image, "SIMPLE_PINHOLE", [64.0, 32.0, 24.0], lib=lib), image)
    got = A.prep_undistort_host(image, "PINHOLE", p, out_K=[64.0, 64.0, 32.0 - 3, 24.0], lib=lib)
    assert np.array_equal(got[:, :-3], image[:, 3:]) and not got[:, -3:].any()
    got = A.prep_undistort_host(image, "PINHOLE", p, out_K=[64.0, 64.0, 32.0 - 0.5, 24.0], lib=lib)
    a = image.astype(np.int64)
    b = np.concatenate([a[:, 1:], np.zeros_like(a[:, :1])], 1)  # the neighbour to the right, black past the edge
    assert np.array_equal(got, (a + b + 1) >> 1)


@pytest.mark.parametrize("model", U.DISTORTED)
def test_zero_coefficients_are_the_identity(lib, image, model):
    zeros = [0.0] * len(U.COEFFS[model])
    if "FISHEYE" not in model:
        p = U.camera(model, zeros, f=64.0, cx=32.0, cy=24.0)
        if model not in U.ONE_F:
            p[1] = 64.0
        assert np.array_equal(A.prep_undistort_host(image, model, p, lib=lib), image)
        return
    # a fisheye model without coefficients is the equidistant projection, the identity only where
    # atan(r) = r in double: a 3x2 image with f = 2^40 keeps r below 2^-29, where atan_c(r) is r
    small = image[:2, :3]
    p = U.camera(model, zeros, f=2.0 ** 40, cx=1.5, cy=1.0)
    if model not in U.ONE_F:
        p[1] = 2.0 ** 40
    assert np.array_equal(A.prep_undistort_host(small, model, p, lib=lib), small)
    # at 64x48 and f = 50 it is not the identity, but it is the restatement's image
    p = U.camera(model, zeros)
    got = A.prep_undistort_host(image, model, p, lib=lib)
    assert np.array_equal(got, U.warp(image, model, p)) and not np.array_equal(got, image)


# ---- 2. the restatement --------------------------------------------------------------------------------

CASES = U.warp_cases(list(U.MODELS))


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_warp_equals_the_restatement(lib, case):
    label, model, params, shape, out_K, out_size = case
    src = np.random.default_rng(32).integers(1, 256, shape + (3,)).astype(np.uint8)  # no black in the source
    got = A.prep_undistort_host(src, model, params, out_K, out_size, lib=lib)
    want, inside, full = U.warp(src, model, params, out_K, out_size, details=True)
    assert got.shape == want.shape and np.array_equal(got, want), int((got != want).sum())
    if label.endswith("/corners-outside"):
        assert (~inside).any() and not got[~inside].any()  # black pixels
        border = inside & ~full
        assert border.any() and got[border].any()           # and pixels blended with the black border
    if label.endswith("/overflow"):
        sx, sy = U.source_coords(model, params, out_K, shape[1], shape[0])
        assert np.isnan(sx).any() or np.isnan(sy).any()
        with np.errstate(invalid="ignore"):
            assert (np.abs(sx) >= 1e300).any() or (np.abs(sy) >= 1e300).any()
        assert not got.any()


def test_rejected_arguments(lib, image):
    p = np.array(U.camera("OPENCV"))
    K = np.array([50.0, 50.0, 30.0, 20.0])
    dst = np.zeros((48, 64, 3), np.uint8)

    def call(model=4, params=p, n=8, sw=64, sh=48, src=image, K=K, ow=64, oh=48, dst=dst):
        ptr = lambda a: None if a is None else a.ctypes.data
        return lib.apd_prep_undistort_bgr8_host(model, ptr(params), n, sw, sh, ptr(src), ptr(K), ow, oh, ptr(dst))

    assert call() == 0
    assert call(model=7, n=5) == EINVAL and call(model=11) == EINVAL and call(model=-1) == EINVAL
    assert call(n=7) == EINVAL and call(n=9) == EINVAL and call(model=2) == EINVAL
    for k in (0, 1, 5):
        for bad in (np.nan, np.inf):
            q = p.copy()
            q[k] = bad
            assert call(params=q) == EINVAL
    for k, bad in ((0, 0.0), (1, -1.0)):
        q = p.copy()
        q[k] = bad
        assert call(params=q) == EINVAL
    assert call(K=np.array([0.0, 50, 30, 20])) == EINVAL and call(K=np.array([50.0, 50, np.nan, 20])) == EINVAL
    assert call(sw=0) == EINVAL and call(sh=65537) == EINVAL and call(ow=0) == EINVAL and call(oh=65537) == EINVAL
    assert call(params=None) == EINVAL and call(src=None) == EINVAL and call(K=None) == EINVAL and call(dst=None) == EINVAL


# ---- 3. atan_c -----------------------------------------------------------------------------------------

def test_atan_c(lib):
    x = np.concatenate([[0.0], np.logspace(-9, 4, 100000)])
    for b in U.ATAN_BREAKS:
        x = np.concatenate([x, [np.nextafter(b, 0.0), b, np.nextafter(b, np.inf)]])
    got = np.array([lib.apd_prep_atan_c(float(v)) for v in x])
    assert np.array_equal(got.view(np.uint64), U.atan_c(x).view(np.uint64))
    err = np.abs(got - np.array([math.atan(float(v)) for v in x]))
    print("atan_c: max |error| against math.atan = %.3g rad" % err.max())
    # 1e-13 rad times f <= 1e5 px is 1e-8 px, far below the 1/512 px weight quantum
    assert err.max() <= 1e-13
    assert lib.apd_prep_atan_c(float("inf")) == math.pi / 2 and math.isnan(lib.apd_prep_atan_c(float("nan")))


# ---- 4. geometry against an analytic image -------------------------------------------------------------

def scene(x, y):
    """(..., 3) doubles at pinhole pixel coordinates (x, y), the centre of pixel (0, 0) being (0.5, 0.5)"""
    return np.stack([127.5 + 100 * np.sin(2 * np.pi * x / 32), 127.5 + 100 * np.cos(2 * np.pi * y / 32),
                     127.5 + 60 * np.sin(2 * np.pi * (x + y) / 32)], -1)


@pytest.mark.parametrize("model,coeffs", [("SIMPLE_RADIAL", [-0.12]), ("SIMPLE_RADIAL", [0.1]),
                                          ("OPENCV", [-0.15, 0.05, 0.004, -0.003]), ("RADIAL_FISHEYE", [0.03, -0.01])])
def test_geometry_against_an_analytic_image(lib, model, coeffs):
    """|out - I| <= 2.5 grey levels where all four taps are inside: the bilinear error is at most
    2 * (1/8) * 100 * (2 pi / 32)^2 * m^2 with the local magnification m <= 1.25, plus 0.5 for the
    rounding of the source, 0.5 for that of the output and < 0.1 for the 1/256 weights. A half-pixel
    convention error shows as about 10 levels. Measured: at most 1.5."""
    w, h = 64, 48
    p = U.camera(model, coeffs, f=50.0, cx=32.0, cy=24.0)
    if model not in U.ONE_F:
        p[1] = 50.0
    jj, ii = np.mgrid[0:h, 0:w]
    px, py = U.undistort_pixels(model, p, ii + 0.5, jj + 0.5)  # where each source pixel centre looks
    src = np.where(np.isnan(px)[..., None], 0.0, np.floor(scene(np.nan_to_num(px), np.nan_to_num(py)) + 0.5))
    out = A.prep_undistort_host(src.astype(np.uint8), model, p, lib=lib)
    _, inside, full = U.warp(src.astype(np.uint8), model, p, details=True)
    err = np.abs(out.astype(np.float64) - scene(ii + 0.5, jj + 0.5))[full]
    print("%s %s: inside share %.3f, max |out - I| = %.3f" % (model, coeffs, full.mean(), err.max()))
    assert full.mean() >= 0.85
    assert err.max() <= 2.5


# ---- 5. keypoints --------------------------------------------------------------------------------------

@pytest.mark.parametrize("model", U.DISTORTED)
def test_undistort_xy_round_trip(lib, model):
    """forward(result) is the input within 1e-6 px: the iteration stops at steps below 1e-10 normalised
    and f <= 1e4."""
    p = U.camera(model)
    pts = np.random.default_rng(33).uniform([0, 0], [64, 48], (1000, 2))
    out, bad = A.prep_undistort_xy(pts, model, p, lib)
    assert bad == 0 and out.shape == pts.shape
    bx, by = U.distort_pixels(model, p, out[:, 0], out[:, 1])
    assert np.abs(bx - pts[:, 0]).max() <= 1e-6 and np.abs(by - pts[:, 1]).max() <= 1e-6
    # and the tests' own inverse agrees
    ux, uy = U.undistort_pixels(model, p, pts[:, 0], pts[:, 1])
    assert np.abs(ux - out[:, 0]).max() <= 1e-6 and np.abs(uy - out[:, 1]).max() <= 1e-6


def test_undistort_xy_unresolved_and_rejected(lib):
    # A fisheye image is bounded: t = atan(r) < pi/2, and t (1 + k t^2) with k = -0.3 stays below 0.71 there,
    # so a point at a distorted radius of 3 (150 px at f = 50) has no preimage at all. (A polynomial model
    # of odd degree always has some far real root, which Newton's method may find.)
    p = [50.0, 32.0, 24.0, -0.3]
    pts = np.array([[32.0 + 150.0, 24.0], [40.0, 30.0], [32.0, 24.0 - 150.0]])
    out, bad = A.prep_undistort_xy(pts, "SIMPLE_RADIAL_FISHEYE", p, lib)
    assert bad == 2 and out[0].tolist() == [-1.0, -1.0] and out[2].tolist() == [-1.0, -1.0]
    bx, by = U.distort_pixels("SIMPLE_RADIAL_FISHEYE", p, out[1, 0], out[1, 1])
    assert abs(bx - 40.0) <= 1e-6 and abs(by - 30.0) <= 1e-6
    p = [50.0, 32.0, 24.0, -0.5]
    out, bad = A.prep_undistort_xy(np.zeros((0, 2)), "SIMPLE_RADIAL", p, lib)
    assert bad == 0 and out.shape == (0, 2)
    out, bad = A.prep_undistort_xy(pts, "PINHOLE", [50.0, 51.0, 32.0, 24.0], lib)
    assert bad == 0 and np.abs(out - pts).max() <= 1e-9
    q = np.array(p)
    xy = np.zeros(2)
    assert lib.apd_prep_undistort_xy(7, q.ctypes.data, 4, 1, xy.ctypes.data, xy.ctypes.data, None) == EINVAL
    assert lib.apd_prep_undistort_xy(2, q.ctypes.data, 5, 1, xy.ctypes.data, xy.ctypes.data, None) == EINVAL
    assert lib.apd_prep_undistort_xy(2, q.ctypes.data, 4, 1, None, xy.ctypes.data, None) == EINVAL
    assert lib.apd_prep_undistort_xy(2, q.ctypes.data, 4, -1, xy.ctypes.data, xy.ctypes.data, None) == EINVAL
    assert lib.apd_prep_undistort_xy(2, np.array([0.0, 1, 1, 0]).ctypes.data, 4, 1, xy.ctypes.data, xy.ctypes.data, None) == EINVAL
    assert lib.apd_prep_undistort_xy(2, np.array([50.0, 1, 1, np.nan]).ctypes.data, 4, 1, xy.ctypes.data, xy.ctypes.data, None) == EINVAL


# ---- 6. the reader -------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def host():
    A.torch_runtime_first()  # libapdhost.so links libapd_hip.so
    h = C.CDLL(HOST_LIB)
    for f in (h.apdhost_colmap_dump, h.apdhost_colmap_dump_distorted):
        f.restype = C.c_long
        f.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_long]
    return h


def dump(fn, d, ext, path=None):
    err = C.create_string_buffer(1024)
    n = fn(str(d).encode(), ext.encode(), None if path is None else str(path).encode(), err, len(err))
    return n if n >= 0 else err.value.decode()


def all_cameras():
    # one camera per model, with parameters that have no short decimal form
    return [{"id": 3 + i, "model": m, "width": 64, "height": 48, "params": [v + 0.1 * (k + 1) / 3 for k, v in enumerate(U.camera(m))]}
            for i, m in enumerate(U.MODELS)]


def write_model(d, cameras, rng):
    images, pids, xyz = P.ring_model(len(cameras), 30, rng, mean_track=3)
    for im, c in zip(images, cameras):
        im["camera_id"] = c["id"]
        im["xys"] = rng.uniform(0, 30, (len(im["point_ids"]), 2))
    pin = [{"id": c["id"], "model": "PINHOLE", "width": 64, "height": 48, "params": [1.0, 1.0, 1.0, 1.0]} for c in cameras]
    P.write_colmap_text(str(d), pin, images, pids, xyz)
    P.write_colmap_bin(str(d), pin, images, pids, xyz)
    U.write_cameras_txt(str(d / "cameras.txt"), cameras)
    U.write_cameras_bin(str(d / "cameras.bin"), cameras)
    return images, pids, xyz


@pytest.fixture(scope="module")
def distorted_model(tmp_path_factory):
    d = tmp_path_factory.mktemp("distorted")
    cams = all_cameras()
    return (d, cams) + write_model(d, cams, np.random.default_rng(34))


def test_reader_with_distorted_models(host, distorted_model, tmp_path):
    d, cams = distorted_model[:2]
    assert isinstance(dump(host.apdhost_colmap_dump_distorted, d, ".txt", tmp_path / "t.dump"), int)
    assert isinstance(dump(host.apdhost_colmap_dump_distorted, d, ".bin", tmp_path / "b.dump"), int)
    text = (tmp_path / "t.dump").read_text()
    assert text == (tmp_path / "b.dump").read_text()
    lines = [l.split() for l in text.split("\n") if l.startswith("camera ")]
    assert len(lines) == len(cams)
    for l, c in zip(lines, cams):
        assert l[1:5] == [str(c["id"]), c["model"], "64", "48"]
        assert [float.fromhex(v) for v in l[5:]] == c["params"]  # the model's own count, exact doubles
    # the plain export refuses them as before, in both formats, with the present words
    for ext in (".txt", ".bin"):
        msg = dump(host.apdhost_colmap_dump, d, ext)
        assert "unsupported camera model SIMPLE_RADIAL (only SIMPLE_PINHOLE and PINHOLE; undistort the images first)" in msg


def test_reader_still_rejects(host, distorted_model, tmp_path):
    d = distorted_model[0]

    def variant(name, cameras):
        v = tmp_path / name
        shutil.copytree(d, v)
        U.write_cameras_txt(str(v / "cameras.txt"), cameras)
        U.write_cameras_bin(str(v / "cameras.bin"), cameras)
        return v

    cams = all_cameras()
    fov = [dict(c) for c in cams]
    fov[2] = dict(fov[2], model="FOV", params=[50.0, 50.0, 32.0, 24.0, 0.9])
    v = variant("fov", fov)
    for fn in (host.apdhost_colmap_dump_distorted, host.apdhost_colmap_dump):
        for ext in (".txt", ".bin"):
            msg = dump(fn, v, ext)
            assert isinstance(msg, str) and "unsupported camera model" in msg
    assert "unsupported camera model FOV" in dump(host.apdhost_colmap_dump_distorted, v, ".txt")
    assert "unsupported camera model FOV" in dump(host.apdhost_colmap_dump_distorted, v, ".bin")
    unknown = [dict(c) for c in cams]
    unknown[0] = dict(unknown[0], model=11)
    U.write_cameras_bin(str(v / "cameras.bin"), unknown)
    assert "unsupported camera model id 11" in dump(host.apdhost_colmap_dump_distorted, v, ".bin")
    # a wrong parameter count: one too few and one too many
    for k, cut in enumerate((-1, 1)):
        bad = [dict(c) for c in cams]
        bad[4] = dict(bad[4], params=bad[4]["params"][:cut] if cut < 0 else bad[4]["params"] + [0.5])
        v = variant("count%d" % k, bad)
        assert "wrong number of parameters" in dump(host.apdhost_colmap_dump_distorted, v, ".txt")
        msg = dump(host.apdhost_colmap_dump_distorted, v, ".bin")  # the binary count is the model's: the file ends early or late
        assert isinstance(msg, str) and ("truncated" in msg or "bytes after" in msg or "unsupported" in msg or "size out of range" in msg), msg
    for k, value in enumerate((float("nan"), float("inf"))):
        bad = [dict(c) for c in cams]
        bad[7] = dict(bad[7], params=bad[7]["params"][:-1] + [value])
        v = variant("nonfinite%d" % k, bad)
        assert "bad parameter" in dump(host.apdhost_colmap_dump_distorted, v, ".txt")
        assert "non-finite camera parameters" in dump(host.apdhost_colmap_dump_distorted, v, ".bin")


# ---- 7. the binary without a device --------------------------------------------------------------------

def test_apd_prepare_without_a_device(distorted_model, tmp_path):
    d, cams, images = distorted_model[:3]
    img = tmp_path / "img"
    for im in images:
        P.write_png(str(img / im["name"]), np.zeros((48, 64, 3), np.uint8))
    out = tmp_path / "out"

    def run(*args):
        return subprocess.run([APD_PREPARE, "--model_dir", str(d), "--image_dir", str(img), "--save_folder", str(out),
                               *map(str, args)], capture_output=True, text=True, timeout=120, env=NO_GPU)

    r = run("--help")
    assert r.returncode == 0 and "--undistort" in r.stdout and "THIN_PRISM_FISHEYE" in r.stdout
    for ext in (".txt", ".bin"):
        r = run("--model_ext", ext)
        assert r.returncode == 2 and not out.exists()
        assert "unsupported camera model SIMPLE_RADIAL (only SIMPLE_PINHOLE and PINHOLE; undistort the images first)" in r.stderr
    # with the flag the inputs are good, so the missing device is what stops it (exit 1), before any file
    r = run("--undistort")
    assert r.returncode == 1 and "no such HIP device" in r.stderr and not out.exists()
    # ... unless an image is not of its distorted camera's size: exit 2
    P.write_png(str(img / images[3]["name"]), np.zeros((40, 64, 3), np.uint8))
    r = run("--undistort")
    assert r.returncode == 2 and "64x40" in r.stderr and not out.exists()
    # FOV stays unsupported with the flag
    fov = tmp_path / "fov"
    shutil.copytree(d, fov)
    bad = [dict(c) for c in cams]
    bad[1] = dict(bad[1], model="FOV", params=[50.0, 50.0, 32.0, 24.0, 0.9])
    U.write_cameras_txt(str(fov / "cameras.txt"), bad)
    r = subprocess.run([APD_PREPARE, "--model_dir", str(fov), "--image_dir", str(img), "--save_folder", str(out),
                        "--undistort"], capture_output=True, text=True, timeout=120, env=NO_GPU)
    assert r.returncode == 2 and "unsupported camera model FOV" in r.stderr and not out.exists()


# ---- 8. sanitizers -------------------------------------------------------------------------------------

def test_host_entries_under_sanitizers():
    """The stand-alone program host/undistort_san_main.cpp, built with AddressSanitizer + UBSan, runs
    apd_prep_undistort_bgr8_host and apd_prep_undistort_xy on the shapes of the restatement test (the
    overflowing coefficients and the 1x1 source included) with exact-size heap buffers."""
    r = subprocess.run(["make", "-C", HOST, "sanitize-undistort"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    env = dict(NO_GPU, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([os.path.join(HOST, "build-san", "undistort_san_main")], capture_output=True, text=True,
                       timeout=300, env=env)
    assert p.returncode == 0 and "runtime error" not in p.stderr and "Sanitizer" not in p.stderr, (p.stdout, p.stderr[-3000:])
    assert p.stdout.strip().splitlines()[-1].endswith(" 0 failures")
