"""apd_prep_undistort_bgr8 (k_pr_undistort) and `apd_prepare --undistort` on the GPU: the device equals
the host entry byte for byte (which tests/test_undistort_host.py ties to the restatement), status codes
leave the context usable, and the binary writes what tests/undistort_lib.py computes."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import apd_abi as A
import prep_lib as P
import undistort_lib as U

pytestmark = pytest.mark.gpu

EINVAL = -1
APD_PREPARE = os.path.join(A.HERE, "host", "build", "apd_prepare")
APD = os.path.join(A.HERE, "host", "build", "apd")
CASES = U.warp_cases(list(U.MODELS))


@pytest.fixture(scope="module")
def lib():
    return A.load_library()


@pytest.fixture(scope="module")
def eng(lib):
    e = A.PrepEngine(0, lib)
    yield e
    e.close()


def random_image(shape, seed=41):
    return np.random.default_rng(seed).integers(1, 256, tuple(shape) + (3,)).astype(np.uint8)


# ---- 1. device equals host -----------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_device_equals_host(lib, eng, case):
    label, model, params, shape, out_K, out_size = case
    src = random_image(shape)
    want = A.prep_undistort_host(src, model, params, out_K, out_size, lib=lib)
    got = eng.undistort(src, model, params, out_K, out_size)
    assert got.shape == want.shape and np.array_equal(got, want), int((got != want).sum())
    t = eng.undistort_timing()
    assert set(t) == {"upload_ms", "kernel_ms", "download_ms"} and all(v >= 0 for v in t.values())


@pytest.mark.parametrize("model", list(U.MODELS))
def test_partial_tiles_on_both_axes(lib, eng, model):
    """257 x 131: one column and three rows past the last full 64 x 4 tile."""
    src = random_image((131, 257), 42)
    p = U.camera(model, f=200.0, cx=127.25, cy=66.5)
    want = A.prep_undistort_host(src, model, p, lib=lib)
    assert np.array_equal(eng.undistort(src, model, p), want)
    # and an output that is a single partial tile, from the same source
    K = [150.0, 150.0, 20.5, 1.5]
    assert np.array_equal(eng.undistort(src, model, p, K, (41, 3)), A.prep_undistort_host(src, model, p, K, (41, 3), lib=lib))


def test_device_pointers(lib, eng):
    import torch
    src = random_image((48, 64), 43)
    p = np.array(U.camera("THIN_PRISM_FISHEYE"))
    K = np.array([40.0, 41.0, 20.0, 15.0])
    want = A.prep_undistort_host(src, "THIN_PRISM_FISHEYE", p, K, (41, 29), lib=lib)
    d_src = torch.from_numpy(src).cuda()
    d_dst = torch.zeros((29, 41, 3), dtype=torch.uint8, device="cuda")
    h_dst = np.zeros((29, 41, 3), np.uint8)
    torch.cuda.synchronize()
    for s, d in ((d_src.data_ptr(), d_dst.data_ptr()), (src.ctypes.data, d_dst.data_ptr()), (d_src.data_ptr(), h_dst.ctypes.data)):
        d_dst.zero_()
        h_dst[:] = 0
        torch.cuda.synchronize()
        assert lib.apd_prep_undistort_bgr8(eng.ctx, 10, p.ctypes.data, 12, 64, 48, s, K.ctypes.data, 41, 29, d) == 0
        got = d_dst.cpu().numpy() if d == d_dst.data_ptr() else h_dst
        assert np.array_equal(got, want)


def test_two_sizes_and_interleaving_on_one_context(lib):
    """Buffers grow and shrink in use without stale data, and a warp between set_model and pair_counts
    leaves both results as they are alone."""
    rng = np.random.default_rng(44)
    images, pids, xyz = P.ring_model(10, 300, rng, mean_track=4)
    m = P.model_ref(images, pids, xyz)
    off, pts = P.csr(m["obs"])
    gate = A.prep_cos_gate(1.0, lib)
    want_s, want_n, _ = P.pair_counts_ref(m["centres"], m["xyz"], m["obs"], gate)
    small, large = random_image((24, 32), 45), random_image((131, 257), 46)
    p_small, p_large = U.camera("OPENCV", f=30.0, cx=15.5, cy=11.0), U.camera("RADIAL_FISHEYE", f=200.0, cx=127.25, cy=66.5)
    w_small = A.prep_undistort_host(small, "OPENCV", p_small, lib=lib)
    w_large = A.prep_undistort_host(large, "RADIAL_FISHEYE", p_large, lib=lib)
    e = A.PrepEngine(0, lib)
    try:
        assert np.array_equal(e.undistort(small, "OPENCV", p_small), w_small)
        assert np.array_equal(e.undistort(large, "RADIAL_FISHEYE", p_large), w_large)
        assert np.array_equal(e.undistort(small, "OPENCV", p_small), w_small)
        e.set_model(m["rot"], m["trans"], m["centres"], m["xyz"], off, pts)
        assert np.array_equal(e.undistort(large, "RADIAL_FISHEYE", p_large), w_large)
        s, n = e.pair_counts(gate)
        assert np.array_equal(e.undistort(small, "OPENCV", p_small), w_small)
        z, _ = e.depth_ranks([0.01, 0.99])
        assert np.array_equal(s, want_s) and np.array_equal(n, want_n)
        assert P.same_bits64(z, P.depth_ranks_ref(m["rot"], m["trans"], m["xyz"], m["obs"], [0.01, 0.99])[0])
    finally:
        e.close()


# ---- 2. status codes -----------------------------------------------------------------------------------

def test_status_codes_leave_the_context_usable(lib, eng):
    src = random_image((48, 64), 47)
    p = np.array(U.camera("OPENCV"))
    K = np.array([50.0, 50.0, 30.0, 20.0])
    dst = np.zeros((48, 64, 3), np.uint8)
    want = A.prep_undistort_host(src, "OPENCV", p, K, lib=lib)

    def call(ctx=eng.ctx, model=4, params=p, n=8, sw=64, sh=48, s=src, K=K, ow=64, oh=48, d=dst):
        ptr = lambda a: None if a is None else a.ctypes.data
        return lib.apd_prep_undistort_bgr8(ctx, model, ptr(params), n, sw, sh, ptr(s), ptr(K), ow, oh, ptr(d))

    def still_works():
        dst[:] = 0
        return call() == 0 and np.array_equal(dst, want)

    assert still_works()
    assert call(ctx=None) == EINVAL
    for kw in (dict(model=7, n=5), dict(model=11), dict(model=-1), dict(n=7), dict(n=9), dict(model=2),
               dict(sw=0), dict(sh=65537), dict(ow=0), dict(oh=65537), dict(ow=-1),
               dict(params=None), dict(s=None), dict(K=None), dict(d=None),
               dict(K=np.array([0.0, 50, 30, 20])), dict(K=np.array([50.0, -1, 30, 20])), dict(K=np.array([50.0, 50, np.inf, 20]))):
        assert call(**kw) == EINVAL, kw
        assert b"apd_prep_undistort_bgr8" in lib.apd_prep_last_error(eng.ctx)
        assert still_works(), kw
    for k, bad in ((0, 0.0), (1, -2.0), (0, np.nan), (5, np.inf), (7, np.nan)):
        q = p.copy()
        q[k] = bad
        assert call(params=q) == EINVAL and still_works(), (k, bad)
    assert lib.apd_prep_get_undistort_timing(None, None, None, None) == EINVAL
    assert lib.apd_prep_get_undistort_timing(eng.ctx, None, None, None) == 0


# ---- 3. the binary -------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def host():
    A.torch_runtime_first()  # libapdhost.so links libapd_hip.so
    h = C.CDLL(os.path.join(A.HERE, "host", "build", "libapdhost.so"))
    h.apdhost_read_camera.argtypes = [C.c_char_p, C.POINTER(A.ApdCamera)]
    h.apdhost_read_bgr8.restype = C.c_long
    h.apdhost_read_bgr8.argtypes = [C.c_char_p, C.c_void_p, C.c_long, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    return h


def read_bgr(host, path):
    w, h = C.c_int(), C.c_int()
    n = host.apdhost_read_bgr8(str(path).encode(), None, 0, C.byref(w), C.byref(h))
    assert n > 0, path
    out = np.zeros(n, np.uint8)
    host.apdhost_read_bgr8(str(path).encode(), out.ctypes.data, n, C.byref(w), C.byref(h))
    return out.reshape(h.value, w.value, 3)


OPENCV_PARAMS = [40.0, 41.0, 15.5, 11.5, -0.15, 0.05, 0.004, -0.003]


def write_two_camera_model(d, declared):
    """12 images of 32x24, even ones of PINHOLE camera 7, odd ones of camera 8 (`declared`)."""
    rng = np.random.default_rng(48)
    images, pids, xyz = P.ring_model(12, 800, rng, mean_track=5, first_id=3, id_step=2)
    pictures = []
    for i, im in enumerate(images):
        im["camera_id"] = 7 + i % 2
        im["name"] = "im%02d.png" % i
        im["xys"] = rng.uniform(0, [32, 24], (len(im["point_ids"]), 2))
        pictures.append(rng.integers(0, 256, (24, 32, 3)).astype(np.uint8))
        P.write_png(str(d / "images" / im["name"]), pictures[-1])
    pin = [{"id": 7, "model": "PINHOLE", "width": 32, "height": 24, "params": [40.0, 41.0, 15.5, 11.5]},
           {"id": 8, "model": "PINHOLE", "width": 32, "height": 24, "params": OPENCV_PARAMS[:4]}]
    P.write_colmap_text(str(d / "sparse"), pin, images, pids, xyz)
    if declared != "PINHOLE":
        pin[1] = dict(pin[1], model=declared, params=OPENCV_PARAMS)
        U.write_cameras_txt(str(d / "sparse" / "cameras.txt"), pin)
    return images, pictures


def test_apd_prepare_undistort(host, lib, tmp_path):
    images, pictures = write_two_camera_model(tmp_path / "dist", "OPENCV")
    write_two_camera_model(tmp_path / "pin", "PINHOLE")
    out, ref = tmp_path / "scan", tmp_path / "scan_pin"
    r = subprocess.run([APD_PREPARE, "--dense_folder", tmp_path / "dist", "--save_folder", out, "--undistort",
                        "--no-sequential", "--json", tmp_path / "p.json"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    r = subprocess.run([APD_PREPARE, "--dense_folder", tmp_path / "pin", "--save_folder", ref, "--no-sequential"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    info = json.loads((tmp_path / "p.json").read_text())
    assert info["images"] == 12 and info["images_undistorted"] == 6 and info["images_copied"] == 6
    assert info["keypoints_unresolved"] == 0
    assert all(info[k] >= 0 for k in ("undistort_upload_ms", "undistort_kernel_ms", "undistort_download_ms"))
    # selection and depth ranges do not depend on distortion
    assert (out / "pair.txt").read_bytes() == (ref / "pair.txt").read_bytes()
    for i in range(12):
        cam_file = "cams/%08d_cam.txt" % i
        assert (out / cam_file).read_bytes() == (ref / cam_file).read_bytes()
        cam = A.ApdCamera()
        assert host.apdhost_read_camera(str(out / cam_file).encode(), C.byref(cam)) == 0
        assert cam.K[:] == [40.0, 0, 15.5, 0, 41.0, 11.5, 0, 0, 1]
        if i % 2 == 0:  # the pinhole camera's images are byte copies
            assert (out / "images" / ("%08d.png" % i)).read_bytes() == (tmp_path / "dist" / "images" / ("im%02d.png" % i)).read_bytes()
        else:
            assert np.array_equal(read_bgr(host, out / "images" / ("%08d.png" % i)), U.warp(pictures[i], "OPENCV", OPENCV_PARAMS))
    cams_txt = (out / "sparse" / "0" / "cameras.txt").read_text()
    assert "7 PINHOLE 32 24 40 41 15.5 11.5" in cams_txt and "8 PINHOLE 32 24 40 41 15.5 11.5" in cams_txt
    assert "OPENCV" not in cams_txt
    rows = [l for l in (out / "sparse" / "0" / "images.txt").read_text().split("\n") if not l.startswith("#")]
    by_id = {int(rows[k].split()[0]): rows[k + 1].split() for k in range(0, len(rows) - 1, 2)}
    for i, im in enumerate(images):
        t = by_id[im["id"]]
        got = np.array([[float(t[3 * k]), float(t[3 * k + 1])] for k in range(len(t) // 3)])
        assert [int(v) for v in t[2::3]] == np.asarray(im["point_ids"]).tolist()  # length and order kept
        want = A.prep_undistort_xy(im["xys"], "OPENCV", OPENCV_PARAMS, lib)[0] if i % 2 else im["xys"]
        assert P.same_bits64(got, want)


# ---- 4. the chain --------------------------------------------------------------------------------------

def test_distorted_scan_runs_through_apd(tmp_path):
    """A synth scene whose images are distorted here (each distorted pixel looks up its pinhole position
    by the tests' own inverse and samples the synth image bilinearly), declared SIMPLE_RADIAL ->
    apd_prepare --undistort -> apd."""
    import synth
    rng = np.random.default_rng(49)
    sc = synth.make_scene(128, 96, 3, seed=11)
    cams, images, pids, xyz = P.scene_to_colmap(sc, rng)
    fx, fy, cx, cy = cams[0]["params"]
    params = [fx, cx, cy, -0.08]
    jj, ii = np.mgrid[0:96, 0:128]
    px, py = U.undistort_pixels("SIMPLE_RADIAL", params, ii + 0.5, jj + 0.5)
    px, py = np.nan_to_num(px - 0.5, nan=-10.0), np.nan_to_num(py - 0.5, nan=-10.0)  # array coordinates
    x0, y0 = np.floor(px).astype(int), np.floor(py).astype(int)
    ax, ay = px - x0, py - y0
    src = tmp_path / "colmap"
    for im, img in zip(images, sc.images):
        g = np.pad(np.asarray(img, np.float64), 1)
        tap = lambda yy, xx: g[np.clip(yy + 1, 0, 97), np.clip(xx + 1, 0, 129)]
        val = ((1 - ax) * (1 - ay) * tap(y0, x0) + ax * (1 - ay) * tap(y0, x0 + 1) + (1 - ax) * ay * tap(y0 + 1, x0) +
               ax * ay * tap(y0 + 1, x0 + 1))
        P.write_png(str(src / "images" / im["name"]), np.repeat(np.clip(np.rint(val), 0, 255).astype(np.uint8)[:, :, None], 3, 2))
        dx, dy = U.distort_pixels("SIMPLE_RADIAL", params, im["xys"][:, 0], im["xys"][:, 1])
        im["xys"] = np.column_stack([dx, dy])
    P.write_colmap_text(str(src / "sparse"), cams, images, pids, xyz)
    U.write_cameras_txt(str(src / "sparse" / "cameras.txt"),
                        [dict(cams[0], model="SIMPLE_RADIAL", params=params)])
    out = tmp_path / "scan"
    r = subprocess.run([APD_PREPARE, "--dense_folder", src, "--save_folder", out, "--undistort", "--no-sequential"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert json.loads(r.stdout.strip().splitlines()[-1])["images_undistorted"] == len(images)
    r = subprocess.run([APD, "--dense_folder", out, "--no_fuse", "true", "--memory_cache", "false"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    depth = synth.read_bin_mat(str(out / "APD" / "00000000" / "depths.bin"))
    assert depth.shape == (96, 128) and (depth > 0).any()
