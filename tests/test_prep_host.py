"""The host side of `apd_prepare`, without a GPU: the COLMAP model readers (text and binary) and the
writers through libapdhost.so, the image copy-versus-PNG rule, the sequential selection against the
restatement in tests/prep_lib.py, option conflicts and unreadable inputs (exit 2 before a device is
touched), --help, the exports, and the readers under ASan + UBSan as a stand-alone program."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import apd_abi as A
import prep_lib as P

HOST = os.path.join(A.HERE, "host")
HOST_LIB = os.path.join(HOST, "build", "libapdhost.so")
APD_PREPARE = os.path.join(HOST, "build", "apd_prepare")
NO_GPU = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
CAMS = [{"id": 2, "model": "PINHOLE", "width": 32, "height": 24, "params": [40.25, 41.0, 15.5, 11.5]},
        {"id": 9, "model": "SIMPLE_PINHOLE", "width": 32, "height": 24, "params": [0.1 + 0.2, 16.0, 12.0]}]


@pytest.fixture(scope="module")
def host():
    A.torch_runtime_first()  # libapdhost.so links libapd_hip.so
    h = C.CDLL(HOST_LIB)
    h.apdhost_colmap_dump.restype = C.c_long
    h.apdhost_colmap_dump.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_long]
    h.apdhost_write_cam_txt.argtypes = [C.c_char_p, C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_double] * 4
    h.apdhost_read_camera.argtypes = [C.c_char_p, C.POINTER(A.ApdCamera)]
    h.apdhost_write_pair_sequential.argtypes = [C.c_char_p, C.c_int, C.c_int]
    h.apdhost_write_pair_scored.argtypes = [C.c_char_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
    h.apdhost_write_png_bgr8.argtypes = [C.c_char_p, C.c_void_p, C.c_int, C.c_int]
    h.apdhost_read_bgr8.restype = C.c_long
    h.apdhost_read_bgr8.argtypes = [C.c_char_p, C.c_void_p, C.c_long, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    h.apdhost_convert_scan_images.restype = C.c_long
    h.apdhost_convert_scan_images.argtypes = [C.c_char_p, C.c_char_p, C.c_double, C.c_char_p, C.c_char_p, C.c_long,
                                              C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_char_p, C.c_long]
    return h


def make_model(rng, n=6, points=40):
    images, pids, xyz = P.ring_model(n, points, rng, mean_track=3, first_id=5, id_step=3,
                                     point_id=lambda k: (1 << 35) + 7 * k if k % 3 == 0 else k + 1)
    for i, im in enumerate(images):
        im["camera_id"] = CAMS[i % 2]["id"]
        im["point_ids"] = np.concatenate([im["point_ids"], [-1], im["point_ids"][:1]]).astype(np.int64)
        im["xys"] = rng.uniform(0, 30, (len(im["point_ids"]), 2))
    return images[::-1], pids, xyz  # descending ids in the file


def dump(host, d, ext, path=None):
    err = C.create_string_buffer(1024)
    n = host.apdhost_colmap_dump(str(d).encode(), ext.encode(), None if path is None else str(path).encode(), err, len(err))
    return n if n >= 0 else err.value.decode()


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    d = tmp_path_factory.mktemp("model")
    images, pids, xyz = make_model(np.random.default_rng(21))
    P.write_colmap_text(str(d), CAMS, images, pids, xyz)
    P.write_colmap_bin(str(d), CAMS, images, pids, xyz)
    return d, images, pids, xyz


def read_bgr(host, path):
    w, h = C.c_int(), C.c_int()
    n = host.apdhost_read_bgr8(str(path).encode(), None, 0, C.byref(w), C.byref(h))
    assert n > 0, path
    out = np.zeros(n, np.uint8)
    host.apdhost_read_bgr8(str(path).encode(), out.ctypes.data, n, C.byref(w), C.byref(h))
    return out.reshape(h.value, w.value, 3)


# ---- readers -------------------------------------------------------------------------------------------

def test_text_and_binary_readers_agree(host, model, tmp_path):
    d, images, pids, xyz = model
    n_obs = sum(int((im["point_ids"] != -1).sum()) for im in images)
    assert dump(host, d, ".txt", tmp_path / "t.dump") == n_obs
    assert dump(host, d, ".bin", tmp_path / "b.dump") == n_obs
    text = (tmp_path / "t.dump").read_text()
    assert text == (tmp_path / "b.dump").read_text()
    # and both hold what was written: ascending image ids, exact doubles, the restatement's arrays
    m = P.model_ref(images, pids, xyz)
    lines = text.split("\n")
    assert lines[0].split()[:5] == ["camera", "2", "PINHOLE", "32", "24"]
    assert [float.fromhex(v) for v in lines[0].split()[5:]] == CAMS[0]["params"]
    assert [float.fromhex(v) for v in lines[1].split()[5:]] == CAMS[1]["params"]
    im_lines = [l.split() for l in lines if l.startswith("image ")]
    prep_lines = [l.split() for l in lines if l.startswith("prep")]
    ordered = sorted(images, key=lambda im: im["id"])
    assert [int(l[1]) for l in im_lines] == [im["id"] for im in ordered]
    for k, (il, pl, im) in enumerate(zip(im_lines, prep_lines, ordered)):
        assert [float.fromhex(v) for v in il[2:9]] == [float(v) for v in list(im["qvec"]) + list(im["tvec"])]
        assert il[10] == im["name"] and [int(v) for v in il[13::3]] == im["point_ids"].tolist()
        assert [float.fromhex(v) for v in il[11::3]] == im["xys"][:, 0].tolist()
        got = np.array([float.fromhex(v) for v in pl[1:13]])
        assert P.same_bits64(got[:9], m["rot"][k].ravel()) and P.same_bits64(got[9:], m["centres"][k])
        assert [int(v) for v in pl[13:]] == m["obs"][k].tolist()
    pt_lines = [l.split() for l in lines if l.startswith("point ")]
    assert [int(l[1]) for l in pt_lines] == pids.tolist()
    assert P.same_bits64(np.array([[float.fromhex(v) for v in l[2:5]] for l in pt_lines]), xyz)


def variant(model, tmp_path, name, ext, file, edit):
    d = tmp_path / name
    shutil.copytree(model[0], d)
    p = d / (file + ext)
    p.write_bytes(edit(p.read_bytes()))
    return d


def test_rejected_models(host, model, tmp_path):
    assert "cannot open" in dump(host, tmp_path, ".txt")
    assert "extension" in dump(host, model[0], ".dat")
    # truncated
    for ext, file in ((".bin", "images"), (".bin", "points3D"), (".bin", "cameras")):
        for cut in (4, 60, -5):
            d = variant(model, tmp_path, "cut%s%s%d" % (file, ext[1:], cut), ext, file, lambda b: b[:cut])
            msg = dump(host, d, ext)
            assert isinstance(msg, str) and ("truncated" in msg or "exceeds" in msg or "unterminated" in msg), msg
    d = variant(model, tmp_path, "cuttxt", ".txt", "images", lambda b: b[:b.rindex(b" ") - 3])
    assert "triples" in dump(host, d, ".txt") or "bad 2D point" in dump(host, d, ".txt")
    # wrong counts: a count the file cannot hold is refused before anything is allocated
    for file in ("images", "points3D", "cameras"):
        d = variant(model, tmp_path, "count" + file, ".bin", file, lambda b: (1 << 60).to_bytes(8, "little") + b[8:])
        assert "exceeds the file" in dump(host, d, ".bin")
    d = variant(model, tmp_path, "fewer", ".bin", "points3D", lambda b: (3).to_bytes(8, "little") + b[8:])
    assert "bytes after the last point" in dump(host, d, ".bin")
    # unknown camera model
    d = variant(model, tmp_path, "radial", ".txt", "cameras", lambda b: b.replace(b"SIMPLE_PINHOLE", b"SIMPLE_RADIAL"))
    assert "unsupported camera model SIMPLE_RADIAL" in dump(host, d, ".txt")
    d = variant(model, tmp_path, "radialbin", ".bin", "cameras", lambda b: b[:12] + (4).to_bytes(4, "little") + b[16:])
    assert "unsupported camera model OPENCV" in dump(host, d, ".bin")
    # a point id that points3D lacks
    keep = lambda b: b"\n".join(b.split(b"\n")[:6]) + b"\n"  # the comment line and five points
    d = variant(model, tmp_path, "lacks", ".txt", "points3D", keep)
    assert "which points3D lacks" in dump(host, d, ".txt")
    # a non-numeric token, a non-finite number, a missing camera
    d = variant(model, tmp_path, "token", ".txt", "points3D", lambda b: b.replace(b" 10 20 30 ", b" 10 2x 30 ", 1))
    assert isinstance(dump(host, d, ".txt"), int)  # colours are not read
    first_x = repr(float(model[3][0, 0])).encode()
    d = variant(model, tmp_path, "token2", ".txt", "points3D", lambda b: b.replace(first_x, b"1.0e", 1))
    assert "bad point line" in dump(host, d, ".txt")
    d = variant(model, tmp_path, "nan", ".txt", "points3D", lambda b: b.replace(first_x, b"nan", 1))
    assert "bad point line" in dump(host, d, ".txt")
    d = variant(model, tmp_path, "nocam", ".txt", "cameras", lambda b: b.replace(b"\n9 SIMPLE", b"\n8 SIMPLE"))
    assert "names camera 9, which is missing" in dump(host, d, ".txt")


# ---- writers -------------------------------------------------------------------------------------------

def test_cam_txt_round_trip(host, tmp_path):
    rng = np.random.default_rng(22)
    R = P.rotation_ref(P.random_quat(rng))
    t = rng.normal(size=3) * 10
    K = np.array([[3411.25, 0, 3115.5], [0, 3410.7, 2064.1], [0, 0, 1]])
    vals = (0.123456789, 1 / 3, 192.0, 23.75)
    path = tmp_path / "00000000_cam.txt"
    assert host.apdhost_write_cam_txt(str(path).encode(), R.ctypes.data, t.ctypes.data, K.ctypes.data, *vals) == 0
    rows = path.read_text().split("\n")
    assert rows[0] == "extrinsic" and rows[4].split() == ["0.0", "0.0", "0.0", "1.0"] and rows[6] == "intrinsic"
    back = np.array([[float(v) for v in rows[1 + r].split()] for r in range(3)])
    assert P.same_bits64(back[:, :3], R) and P.same_bits64(back[:, 3], t)
    assert all(len(v) <= len(repr(float(x))) for v, x in zip(rows[1].split(), list(R[0]) + [t[0]]))  # shortest
    assert P.same_bits64(np.array([[float(v) for v in rows[7 + r].split()] for r in range(3)]), K)
    assert rows[11] == "%f %f %f %f" % vals
    cam = A.ApdCamera()
    assert host.apdhost_read_camera(str(path).encode(), C.byref(cam)) == 0
    assert np.array_equal(np.array(cam.R[:], np.float32), R.astype(np.float32).ravel())
    assert np.array_equal(np.array(cam.K[:], np.float32), K.astype(np.float32).ravel())
    assert cam.depth_num == 192.0 and cam.depth_max == 23.75
    assert host.apdhost_write_cam_txt(str(tmp_path / "no" / "cam.txt").encode(), R.ctypes.data, t.ctypes.data,
                                      K.ctypes.data, *vals) != 0


def pair_text(sel):
    return "%d\n" % len(sel) + "".join("%d\n%d %s\n" % (i, len(s), "".join("%d %d " % js for js in s))
                                      for i, s in enumerate(sel))


@pytest.mark.parametrize("k", [1, 5])
@pytest.mark.parametrize("n", [1, 2, 30])
def test_sequential_selection(host, tmp_path, n, k):
    path = tmp_path / "pair.txt"
    assert host.apdhost_write_pair_sequential(str(path).encode(), n, k) == 0
    want = P.sequential_ref(n, k)
    assert path.read_text() == pair_text(want)
    assert A.prep_select_sequential(n, k) == want
    assert all(len(s) == min(n - 1, 2 * k, len(s)) and i not in [j for j, _ in s] for i, s in enumerate(want))


def test_scored_selection_writer(host, tmp_path):
    rng = np.random.default_rng(23)
    n = 25
    up = np.triu(rng.integers(0, 6, (n, n)), 1)
    shared = (up + up.T).astype(np.uint32)
    nup = np.triu(rng.integers(0, 6, (n, n)), 1)
    narrow = np.minimum(nup + nup.T, shared).astype(np.uint32)
    path = tmp_path / "pair.txt"
    for max_views in (20, 3, 40):
        assert host.apdhost_write_pair_scored(str(path).encode(), n, shared.ctypes.data, narrow.ctypes.data, max_views) == 0
        want = P.select_ref(P.score_ref(shared, narrow), max_views)
        assert path.read_text() == pair_text(want)
        assert A.prep_select(A.prep_score(shared, narrow), max_views) == want


# ---- images --------------------------------------------------------------------------------------------

def convert(host, src, names, scale, out):
    os.makedirs(out, exist_ok=True)
    buf, err = C.create_string_buffer(1 << 12), C.create_string_buffer(512)
    w, h = C.c_int(), C.c_int()
    n = host.apdhost_convert_scan_images(str(src).encode(), "\n".join(names).encode(), scale, str(out).encode(), buf,
                                         len(buf), C.byref(w), C.byref(h), err, len(err))
    assert n >= 0, err.value
    return n, buf.value.decode().split("\n"), w.value, h.value


def test_png_writer_and_the_copy_rule(host, tmp_path):
    from PIL import Image
    rng = np.random.default_rng(24)
    src = tmp_path / "src"
    big = rng.integers(0, 256, (24, 32, 3)).astype(np.uint8)
    small = rng.integers(0, 256, (20, 31, 3)).astype(np.uint8)
    P.write_png(str(src / "a.PNG"), big)
    P.write_png(str(src / "sub" / "b.png"), big[::-1])
    Image.fromarray(np.ascontiguousarray(big[:, :, ::-1])).save(src / "c.jpg", quality=90)
    path = tmp_path / "w.png"
    assert host.apdhost_write_png_bgr8(str(path).encode(), small.ctypes.data, 31, 20) == 0
    assert np.array_equal(read_bgr(host, path), small)
    assert np.array_equal(np.asarray(Image.open(path).convert("RGB"))[:, :, ::-1], small)
    # same size, scale 1: copied byte for byte under the lower-cased extension
    n, names, w, h = convert(host, src, ["a.PNG", "sub/b.png", "c.jpg"], 1.0, tmp_path / "o1")
    assert (n, names, w, h) == (3, ["00000000.png", "00000001.png", "00000002.jpg"], 32, 24)
    for name, s in zip(names, ["a.PNG", "sub/b.png", "c.jpg"]):
        assert (tmp_path / "o1" / name).read_bytes() == (src / s).read_bytes()
    # a smaller image: it is padded bottom and right and written as PNG, the others are still copied
    P.write_png(str(src / "d.png"), small)
    n, names, w, h = convert(host, src, ["a.PNG", "d.png", "c.jpg"], 1.0, tmp_path / "o1")
    assert (n, names, w, h) == (2, ["00000000.png", "00000001.png", "00000002.jpg"], 32, 24)
    pad = np.zeros((24, 32, 3), np.uint8)
    pad[:20, :31] = small
    assert np.array_equal(read_bgr(host, tmp_path / "o1" / "00000001.png"), pad)
    # scale 2: every image is decoded, padded, resized (nearest: every second pixel) and written as PNG;
    # the .jpg an earlier run left for index 2 is gone
    n, names, w, h = convert(host, src, ["a.PNG", "d.png", "c.jpg"], 2.0, tmp_path / "o1")
    assert (n, names, w, h) == (0, ["00000000.png", "00000001.png", "00000002.png"], 16, 12)
    assert not (tmp_path / "o1" / "00000002.jpg").exists()
    assert np.array_equal(read_bgr(host, tmp_path / "o1" / "00000000.png"), big[::2, ::2])
    assert np.array_equal(read_bgr(host, tmp_path / "o1" / "00000001.png"), pad[::2, ::2])
    assert np.array_equal(read_bgr(host, tmp_path / "o1" / "00000002.png"), read_bgr(host, src / "c.jpg")[::2, ::2])
    n, names, w, h = convert(host, src, ["a.PNG"], 2.5, tmp_path / "o2")
    assert (w, h) == (12, 9)


# ---- the binary without a device -----------------------------------------------------------------------

def run_prepare(*args):
    return subprocess.run([APD_PREPARE, *map(str, args)], capture_output=True, text=True, timeout=120, env=NO_GPU)


def test_help_conflicts_and_unreadable_inputs(model, tmp_path):
    r = run_prepare("--help")
    assert r.returncode == 0
    for flag in ("--dense_folder", "--save_folder", "--max_d", "--interval_scale", "--scale_factor", "--theta0", "--sigma1",
                 "--sigma2", "--model_ext", "--sequential", "--no-sequential", "--sequential_k", "--model_dir",
                 "--image_dir", "--max_views", "--device", "--json"):
        assert flag in r.stdout, flag
    d = model[0]
    out = tmp_path / "out"
    for args in [(), ("--dense_folder", d), ("--save_folder", out),
                 ("--dense_folder", d, "--save_folder", out, "--sequential", "--no-sequential"),
                 ("--dense_folder", d, "--save_folder", out, "--model_ext", ".dat"),
                 ("--dense_folder", d, "--save_folder", out, "--max_d", "x"),
                 ("--dense_folder", d, "--save_folder", out, "--max_d", "1"),
                 ("--dense_folder", d, "--save_folder", out, "--scale_factor", "0"),
                 ("--dense_folder", d, "--save_folder", out, "--bogus", "1"),
                 ("--dense_folder", d, "--save_folder", out, "--json")]:
        r = run_prepare(*args)
        assert r.returncode == 2 and "usage:" in r.stderr, args
    # unreadable inputs: no model, a model whose images are missing, an image that is not one
    cases = [("--dense_folder", tmp_path, "--save_folder", out),
             ("--model_dir", d, "--image_dir", tmp_path, "--save_folder", out),
             ("--model_dir", d, "--image_dir", tmp_path, "--save_folder", out, "--model_ext", ".bin")]
    for args in cases:
        r = run_prepare(*args)
        assert r.returncode == 2 and "cannot open" in r.stderr and "usage:" not in r.stderr, (args, r.stderr)
    img = tmp_path / "img"
    for im in model[1]:
        os.makedirs(os.path.dirname(img / im["name"]), exist_ok=True)
        (img / im["name"]).write_bytes(b"not an image")
    r = run_prepare("--model_dir", d, "--image_dir", img, "--save_folder", out)
    assert r.returncode == 2 and "unsupported image format" in r.stderr
    assert not out.exists()  # nothing is written before the inputs are known to be good
    # readable inputs, no device: a device failure is exit 1, and still nothing is written
    for im in model[1]:
        P.write_png(str(img / im["name"]), np.zeros((4, 6, 3), np.uint8))
    r = run_prepare("--model_dir", d, "--image_dir", img, "--save_folder", out)
    assert r.returncode == 1 and "no such HIP device" in r.stderr and not out.exists()


def test_exports():
    lib = A.load_library()
    assert len(A.PREP_EXPORTS) == 8
    assert [s for s in A.PREP_EXPORTS if not hasattr(lib, s)] == []
    g = A.prep_cos_gate(1.0, lib)
    assert 0.9998 < g < 0.99985 and np.isnan(A.prep_cos_gate(-1.0, lib)) and A.prep_cos_gate(180.0, lib) >= -1.0
    nm = subprocess.run(["nm", "-D", "--defined-only", A.LIB_PATH], capture_output=True, text=True).stdout
    assert all((" T " + s) in nm for s in A.PREP_EXPORTS)


# ---- the readers under sanitizers ----------------------------------------------------------------------

def test_colmap_readers_under_sanitizers(model, tmp_path):
    """A stand-alone program built with AddressSanitizer + UBSan reads the model whole, truncated and
    with flipped bytes, in both formats: each is read or rejected, none is read out of bounds."""
    r = subprocess.run(["make", "-C", HOST, "sanitize-colmap"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    rng = np.random.default_rng(25)
    args = []
    k = 0
    for ext in (".txt", ".bin"):
        args += [str(model[0]), ext]
        for file in ("cameras", "images", "points3D"):
            data = (model[0] / (file + ext)).read_bytes()
            blobs = [data[:cut] for cut in sorted(set(np.linspace(0, len(data) - 1, 12).astype(int).tolist()))]
            for _ in range(20):
                b = bytearray(data)
                for _ in range(int(rng.integers(1, 4))):
                    b[int(rng.integers(0, len(b)))] = int(rng.integers(0, 256))
                blobs.append(bytes(b))
            for blob in blobs:
                d = tmp_path / ("v%d" % k)
                k += 1
                os.makedirs(d)
                for other in ("cameras", "images", "points3D"):
                    if other != file:
                        os.symlink(model[0] / (other + ext), d / (other + ext))
                (d / (file + ext)).write_bytes(blob)
                args += [str(d), ext]
    args += [str(tmp_path / "none"), ".txt", str(tmp_path), ".bin"]
    env = dict(NO_GPU, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([os.path.join(HOST, "build-san", "colmap_corpus_main"), *args], capture_output=True, text=True,
                       timeout=300, env=env)
    assert p.returncode == 0 and "runtime error" not in p.stderr and "Sanitizer" not in p.stderr, (p.stdout, p.stderr[-3000:])
    last = p.stdout.strip().splitlines()[-1]
    assert last.startswith("colmap corpus: ")
    read, rejected = [int(w) for w in last.replace(",", "").split() if w.isdigit()]
    assert read + rejected == len(args) // 2 and read >= 2 and rejected >= 40
