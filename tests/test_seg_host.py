"""Flat-zone sa_masks (include/apd_seg.h) without a GPU: the host twin against known answers and against
the numpy restatement in tests/seg_lib.py (everything is integer: every comparison is exact); the
labelling alone on masks no image produces; rejected arguments; `apd_segment --host`; the host entries
under ASan + UBSan as a stand-alone program; and run_scans.py's opt-in flag."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import apd_abi as A
import prep_lib as P
import seg_lib as L
import synth

HOST = os.path.join(A.HERE, "host")
APD_SEGMENT = os.path.join(HOST, "build", "apd_segment")
RUN_SCANS = os.path.join(A.HERE, "run_scans.py")
NO_GPU = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
EINVAL = -1


@pytest.fixture(scope="module")
def lib():
    return A.load_library()


def test_exports(lib):
    assert [s for s in A.SEG_EXPORTS if not hasattr(lib, s)] == []
    nm = subprocess.run(["nm", "-D", "--defined-only", A.LIB_PATH], capture_output=True, text=True).stdout
    assert all((" T " + s) in nm for s in A.SEG_EXPORTS)
    # a list of its own: the pinned lists do not name the new symbols
    assert not [s for s in A.EXPORTS + A.EVAL_EXPORTS + A.PREP_EXPORTS + A.PREP_UNDISTORT_EXPORTS if s.startswith("apd_seg_")]
    assert [L.colour(k) for k in range(256)] == [A.seg_label_colour(k, lib) for k in range(256)]
    assert L.colour(0) == (255, 255, 255) and all(max(L.colour(k)) < 224 for k in range(1, 256))


# ---- 1. known answers ----------------------------------------------------------------------------------

def zones(lib, img, max_size=0, q8=256, min_area=1):
    labels, ns, nl, st = A.seg_flat_zones_host(img, max_size, q8 / 256.0, min_area, stages=True, lib=lib)
    assert A.seg_threshold_q8(q8 / 256.0) == q8
    return labels, ns, nl, st


def test_constant_image(lib):
    img = np.full((30, 40, 3), 77, np.uint8)
    labels, ns, nl, st = zones(lib, img)
    assert (ns, nl) == (1, 1) and (labels == 1).all()
    assert st["areas"][0, 0] == 40 * 30 and st["areas"].sum() == 40 * 30 and (st["roots"] == 0).all()
    assert (st["smooth"] == 77 * 256).all() and st["flat"].all()
    # min_area at area - 1, area, area + 1
    for min_area, want in ((1199, 1), (1200, 1), (1201, 0)):
        labels, ns, nl, _ = zones(lib, img, min_area=min_area)
        assert (ns, nl) == (want, want) and (labels == want).all()


def test_vertical_step_pins_the_comparison(lib):
    """A step of 16 levels between columns c - 1 and c: S differs between neighbouring columns by
    256 * (1, 4, 6, 4, 1) across the edge. At threshold_q8 = 256 the difference 256 passes, so the band that
    is not flat is c - 2 .. c + 1; at 255 it does not, and the band is c - 3 .. c + 2."""
    h, w, c = 12, 50, 20
    img = L.step_image(h, w, c)
    labels, ns, nl, st = zones(lib, img, q8=256)
    S = st["smooth"][0, 0].astype(np.int64)
    assert np.diff(S)[c - 3:c + 2].tolist() == [256, 1024, 1536, 1024, 256] and not np.diff(S)[:c - 3].any()
    assert np.array_equal(np.nonzero(~st["flat"][5].astype(bool))[0], np.arange(c - 2, c + 2))
    # two regions ranked by area: the right one, 28 columns, before the left one, 18 columns
    assert (ns, nl) == (2, 2)
    assert (labels[:, :c - 2] == 2).all() and (labels[:, c - 2:c + 2] == 0).all() and (labels[:, c + 2:] == 1).all()
    assert st["areas"][0, 0] == 18 * h and st["areas"][0, c + 2] == 28 * h
    labels, ns, nl, st = zones(lib, img, q8=255)
    assert np.array_equal(np.nonzero(~st["flat"][5].astype(bool))[0], np.arange(c - 3, c + 3))
    assert (labels[:, :c - 3] == 2).all() and (labels[:, c - 3:c + 3] == 0).all() and (labels[:, c + 3:] == 1).all()


def test_equal_areas_are_ordered_by_root(lib):
    h, w, c = 12, 40, 20
    labels, ns, nl, st = zones(lib, L.step_image(h, w, c))
    assert (ns, nl) == (2, 2) and st["areas"][0, 0] == st["areas"][0, c + 2] == 18 * h
    assert (labels[:, :c - 2] == 1).all() and (labels[:, c + 2:] == 2).all()
    # and a min_area between nothing: both or neither
    assert zones(lib, L.step_image(h, w, c), min_area=18 * h)[1] == 2
    assert zones(lib, L.step_image(h, w, c), min_area=18 * h + 1)[1] == 0


def test_ramps(lib):
    """One level per pixel: neighbouring columns of S differ by 256 inside and by less at the clamped
    border (176, 240), so everything is flat at 256. Two levels per pixel: 512 inside, 480 next to the
    border and 352 = 16 * 22 between the first two columns (T = 12, 34, 64, 96, ...), so at 256 nothing is
    flat, and the clamping makes exactly the first and the last column flat from 352 on."""
    h, w = 9, 100
    labels, ns, nl, st = zones(lib, L.ramp_image(h, w, 1))
    assert np.diff(st["smooth"][1, 4].astype(np.int64))[:4].tolist() == [176, 240, 256, 256]
    assert st["flat"].all() and (ns, nl) == (1, 1) and (labels == 1).all()
    img = L.ramp_image(h, w, 2)
    labels, ns, nl, st = zones(lib, img)
    assert np.diff(st["smooth"][2, 0].astype(np.int64))[:4].tolist() == [352, 480, 512, 512]
    assert not st["flat"].any() and (ns, nl) == (0, 0) and not labels.any()
    assert not zones(lib, img, q8=351)[3]["flat"].any()
    labels, ns, nl, st = zones(lib, img, q8=352)
    assert st["flat"][:, 0].all() and st["flat"][:, -1].all() and not st["flat"][:, 1:-1].any()
    assert (ns, nl) == (2, 2) and (labels[:, 0] == 1).all() and (labels[:, -1] == 2).all()


def test_downscale_by_hand(lib):
    """5 x 3 by s = 2 (max_size 3): blocks of 4, 4, 2 / 2, 2, 1 pixels; 12.25 -> 12, 22 -> 22, 7.5 -> 8,
    1.5 -> 2, 3.5 -> 4, 5 -> 5."""
    b = np.array([[10, 11, 20, 21, 7], [12, 14, 22, 25, 8], [1, 2, 3, 4, 5]], np.uint8)
    img = np.stack([b, b + 100, np.full_like(b, 255)], -1)
    assert A.seg_working_size(5, 3, 3, lib) == (2, 3, 2) and L.working_size(5, 3, 3) == (2, 3, 2)
    labels, ns, nl, st = zones(lib, img, max_size=3)
    want = np.array([[12, 22, 8], [2, 4, 5]])
    assert labels.shape == (2, 3)
    assert np.array_equal(st["work"][..., 0], want) and np.array_equal(st["work"][..., 1], want + 100)
    assert (st["work"][..., 2] == 255).all()
    assert A.seg_working_size(5, 3, 0, lib) == (1, 5, 3) and A.seg_working_size(5, 3, 5, lib) == (1, 5, 3)
    assert A.seg_working_size(6048, 4032, 2560, lib) == (3, 2016, 1344)


@pytest.fixture(scope="module")
def squares():
    img = L.squares_image()
    return img, L.flat_zones(img, 0, 256, 1)


def test_more_than_255_survivors(lib, squares):
    img, (want_labels, want_ns, want_nl, want_st) = squares
    labels, ns, nl, st = zones(lib, img)
    assert ns > 255 and nl == 255 and ns >= 17 * 17
    areas = st["areas"].ravel()
    order = sorted((-int(areas[r]), int(r)) for r in np.nonzero(areas)[0])
    assert len(order) == ns
    roots = st["roots"]
    for k, (_, r) in enumerate(order):
        assert (labels[roots == r] == (k + 1 if k < 255 else 0)).all()
    assert (labels[roots < 0] == 0).all() and labels.max() == 255
    # equal areas sit on either side of the cap: the order by root decides who is labelled
    assert order[254][0] == order[255][0]
    assert (ns, nl) == (want_ns, want_nl) and np.array_equal(labels, want_labels)


# ---- 2. the restatement --------------------------------------------------------------------------------

IMAGES = L.IMAGE_CASES


@pytest.mark.parametrize("case", IMAGES, ids=[c[0] for c in IMAGES])
def test_host_equals_the_restatement(lib, case):
    _, make, max_size, q8, min_area = case
    img = make()
    labels, ns, nl, st = zones(lib, img, max_size, q8, min_area)
    want_labels, want_ns, want_nl, want_st = L.flat_zones(img, max_size, q8, min_area)
    for name in A.SEG_STAGES:  # in the stages' order: the first that differs is named
        assert st[name].shape == want_st[name].shape and np.array_equal(st[name], want_st[name]), name
    assert (ns, nl) == (want_ns, want_nl) and np.array_equal(labels, want_labels)
    assert st["flat"].any() and not st["flat"].all()
    got = A.seg_flat_zones_host(img, max_size, q8 / 256.0, min_area, lib=lib)
    assert np.array_equal(got[0], labels) and got[1:] == (ns, nl)


MASK_SIZES = [(1, 1), (1, 97), (97, 1), (37, 53)]


@pytest.mark.parametrize("size", MASK_SIZES, ids=["%dx%d" % s for s in MASK_SIZES])
def test_label_mask_host_equals_the_restatement(lib, size):
    H, W = size
    for name, mask in L.mask_cases(H, W, seed=H * 1000 + W).items():
        got = A.seg_label_mask_host(mask, lib)
        want = L.label_mask(mask)
        assert got.dtype == np.int32 and np.array_equal(got, want), name
    if (H, W) == (37, 53):
        cases = L.mask_cases(H, W)
        count = lambda m: len(np.unique(A.seg_label_mask_host(m, lib)[m != 0]))
        assert count(cases["ones"]) == count(cases["spiral"]) == count(cases["serpentine"]) == count(cases["comb"]) == 1
        assert count(cases["checkerboard"]) == (H * W + 1) // 2 and count(cases["two_spirals"]) >= 2
        assert (A.seg_label_mask_host(cases["zeros"], lib) == -1).all()


# ---- 3. rejected arguments -----------------------------------------------------------------------------

def test_rejected_arguments(lib):
    img = np.zeros((4, 6, 3), np.uint8)
    labels = np.zeros((4, 6), np.uint8)
    ow, oh = A.C.c_int32(), A.C.c_int32()

    def call(w=6, h=4, src=img, max_size=0, q8=256, min_area=1, labels=labels, pw=ow, ph=oh):
        ptr = lambda a: None if a is None else a.ctypes.data
        ref = lambda v: None if v is None else A.C.byref(v)
        return lib.apd_seg_flat_zones_bgr8_host(w, h, ptr(src), max_size, q8, min_area, ptr(labels), ref(pw), ref(ph),
                                                None, None, None, None, None, None, None)

    assert call() == 0 and (ow.value, oh.value) == (6, 4)
    assert call(w=0) == EINVAL and call(h=0) == EINVAL and call(w=65537) == EINVAL and call(h=-1) == EINVAL
    assert call(w=65536, h=65536) == EINVAL            # W * H above INT32_MAX (nothing is read before the check)
    assert call(max_size=-1) == EINVAL
    assert call(q8=-1) == EINVAL and call(q8=65281) == EINVAL and call(q8=65280) == 0 and call(q8=0) == 0
    assert call(min_area=0) == EINVAL and call(min_area=-5) == EINVAL
    assert call(src=None) == EINVAL and call(labels=None) == EINVAL and call(pw=None) == EINVAL and call(ph=None) == EINVAL
    mask = np.ones((4, 6), np.uint8)
    roots = np.zeros((4, 6), np.int32)
    lm = lib.apd_seg_label_mask_host
    assert lm(6, 4, mask.ctypes.data, roots.ctypes.data) == 0
    assert lm(0, 4, mask.ctypes.data, roots.ctypes.data) == EINVAL and lm(6, 65537, mask.ctypes.data, roots.ctypes.data) == EINVAL
    assert lm(65536, 65536, mask.ctypes.data, roots.ctypes.data) == EINVAL
    assert lm(6, 4, None, roots.ctypes.data) == EINVAL and lm(6, 4, mask.ctypes.data, None) == EINVAL
    with pytest.raises(A.ApdError, match="APD_EINVAL"):
        A.seg_flat_zones_host(img, min_area=0, lib=lib)
    with pytest.raises(A.ApdError, match="APD_EINVAL"):
        A.seg_flat_zones_host(img, threshold=300.0, lib=lib)
    with pytest.raises(A.ApdError, match="APD_EINVAL"):
        A.seg_working_size(5, 5, -1, lib)


# ---- 4. the binary without a device --------------------------------------------------------------------

def make_scan(folder, images):
    for name, img in images.items():
        P.write_png(os.path.join(str(folder), "images", name), img)
    return str(folder)


def segment(*args):
    return subprocess.run([APD_SEGMENT, *map(str, args)], capture_output=True, text=True, timeout=300, env=NO_GPU)


def test_apd_segment_host(lib, tmp_path):
    from PIL import Image
    images = {"00000000.png": L.patches_image(60, 80, 11, patch=20), "00000001.png": L.gradient_image(60, 80, 12),
              "00000002.v2.png": L.patches_image(90, 130, 13, patch=30)}  # the stem ends at the first dot
    scan = make_scan(tmp_path / "scan", images)
    r = segment("--dense_folder", scan, "--host", "--min_area", 16, "--max_size", 70)
    assert r.returncode == 0, r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["views"] == 3 and out["host"] is True and out["threshold_q8"] == 256 and out["min_area"] == 16
    assert sorted(os.listdir(os.path.join(scan, "sa_masks"))) == sorted(
        s + e for s in ("00000000", "00000001", "00000002") for e in (".bin", ".png"))
    for (name, img), view in zip(sorted(images.items()), out["per_view"]):
        stem = name.split(".")[0]
        labels, ns, nl = A.seg_flat_zones_host(img, 70, 1.0, 16, lib=lib)
        H, W = labels.shape
        assert view == {"view": stem, "width": W, "height": H, "survivors": ns, "labels": nl}
        path = os.path.join(scan, "sa_masks", stem + ".bin")
        assert os.path.getsize(path) == 16 + W * H
        assert np.fromfile(path, np.int32, 4).tolist() == [1, H, W, 0]  # version, rows, cols, CV_8UC1
        assert np.array_equal(synth.read_bin_mat(path), labels)
        rgb = np.asarray(Image.open(os.path.join(scan, "sa_masks", stem + ".png")).convert("RGB"))
        lut = np.array([L.colour(k)[::-1] for k in range(256)], np.uint8)
        assert rgb.shape == (H, W, 3) and np.array_equal(rgb, lut[labels])
    assert out["per_view"][2]["width"] == 65 and out["per_view"][2]["height"] == 45 and out["per_view"][0]["width"] == 40
    assert any(v["labels"] > 1 for v in out["per_view"])
    # an existing folder is refused, unless told otherwise
    r = segment("--dense_folder", scan, "--host")
    assert r.returncode == 2 and "exists" in r.stderr
    r = segment("--dense_folder", scan, "--host", "--overwrite", "--no_png", "--views", "00000001,00000002", "--max_size", 0,
                "--threshold", 0.5)
    assert r.returncode == 0, r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert [v["view"] for v in out["per_view"]] == ["00000001", "00000002"] and out["threshold_q8"] == 128
    labels = A.seg_flat_zones_host(images["00000002.v2.png"], 0, 0.5, 256, lib=lib)[0]
    assert np.array_equal(synth.read_bin_mat(os.path.join(scan, "sa_masks", "00000002.bin")), labels)


def test_apd_segment_exit_2(tmp_path):
    scan = make_scan(tmp_path / "scan", {"00000000.png": L.patches_image(30, 40, 14)})
    masks = os.path.join(scan, "sa_masks")
    assert segment("--help").returncode == 0 and "not SAM" in segment("--help").stdout
    for args in (["--host"], ["--dense_folder", scan, "--bogus", 1], ["--dense_folder", scan, "--min_area", 0],
                 ["--dense_folder", scan, "--max_size", -1], ["--dense_folder", scan, "--threshold", "x"],
                 ["--dense_folder", scan, "--threshold", 256], ["--dense_folder", scan, "--threshold", -1],
                 ["--dense_folder", scan, "--views", "nope"], ["--dense_folder", scan, "--max_size"],
                 ["--dense_folder", str(tmp_path / "missing")]):
        for host in ([], ["--host"]):  # before any context: the same without a device
            r = segment(*args, *host)
            assert r.returncode == 2 and not os.path.exists(masks), (args, r.stderr)
    empty = tmp_path / "empty"
    (empty / "images").mkdir(parents=True)
    assert segment("--dense_folder", empty, "--host").returncode == 2
    with open(os.path.join(scan, "images", "00000001.png"), "wb") as fh:
        fh.write(b"\x89PNG\r\n\x1a\nnot a picture")
    r = segment("--dense_folder", scan)
    assert r.returncode == 2 and "00000001.png" in r.stderr and not os.path.exists(masks)
    os.remove(os.path.join(scan, "images", "00000001.png"))
    # with good inputs and no device, the missing device is what stops it (exit 1) ...
    r = segment("--dense_folder", scan)
    assert r.returncode == 1 and "no such HIP device" in r.stderr and not os.path.exists(masks)
    # ... and the host twin needs none
    assert segment("--dense_folder", scan, "--host").returncode == 0 and os.path.exists(os.path.join(masks, "00000000.bin"))


# ---- 5. sanitizers -------------------------------------------------------------------------------------

def test_host_entries_under_sanitizers(tmp_path):
    """The stand-alone program host/segment_san_main.cpp, built with AddressSanitizer + UBSan, runs the host
    entries over the small shapes (1 x 1, 1 x 97, 97 x 1, tile-sized and odd), rejected arguments and
    truncated sa_masks bin-mats, with exact-size heap buffers."""
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", str(tmp_path / "probe")],
                           input="int main() { return 0; }\n", capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip("the compiler has no sanitizer runtime")
    r = subprocess.run(["make", "-C", HOST, "sanitize-segment"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    env = dict(NO_GPU, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1", TMPDIR=str(tmp_path))
    p = subprocess.run([os.path.join(HOST, "build-san", "segment_san_main")], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0 and "runtime error" not in p.stderr and "Sanitizer" not in p.stderr, (p.stdout, p.stderr[-3000:])
    assert p.stdout.strip().splitlines()[-1].endswith(" 0 failures")


# ---- 6. run_scans.py -----------------------------------------------------------------------------------

def test_run_scans_flag(tmp_path):
    root = tmp_path / "ETH3D"
    for name, n, masks in (("scan_a", 1, False), ("scan_b", 2, True), ("scan_c", 3, False)):
        for i in range(n):
            os.makedirs(root / name / "images", exist_ok=True)
            (root / name / "images" / ("%d.png" % i)).write_bytes(b"")
        if masks:
            os.makedirs(root / name / "sa_masks")

    def review(*flags):
        r = subprocess.run([sys.executable, RUN_SCANS, "--data_dir", str(root), "--review", "--APD_path", "/x/bin/apd", *flags],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        shutil.rmtree(root / "scan_a" / "APD")  # --review leaves the (empty) result folders
        shutil.rmtree(root / "scan_b" / "APD")
        shutil.rmtree(root / "scan_c" / "APD")
        return r.stdout

    def apd_line(scan):
        return ("/x/bin/apd --dense_folder {0} --gpu_index 0 --dataset ETH3D --only_fuse false --no_fuse false  --use_sa true "
                "--memory_cache false --flush false --export_anchor false --export_curve false --export_color true "
                "--use_impetus true --weak_filter true > {0}/APD/log.txt\n").format(root / scan)

    # without the flag: byte for byte the output from before the flag existed
    head = ("Namespace(data_dir='{}', APD_path='/x/bin/apd', resume=False, gpu_num=1, work_num=1, gpus_per_scan=1, scans=[], "
            "only_fuse=False, no_fuse=False, memory_cache=False, no_sam=False, no_impetus=False, no_weak_filter=False, "
            "no_color=False, flush=False, ETH3D_train=False, ETH3D_test=False, TaT_intermediate=False, TaT_advanced=False, "
            "export_anchor=False, export_curve=False, no_image_symlink=False, review=True, "
            "image_dir_name=['images', 'undist/images'], image_suffixes=['.jpg', '.jpeg', '.png']{})\n"
            "scans: ['scan_c', 'scan_b', 'scan_a']\n")
    note = "[{}] no sa_masks/ (SAM generation is out of scope): running without SA masks\n"
    assert review() == (head.format(root, "") + note.format("scan_c") + apd_line("scan_c") + apd_line("scan_b") +
                        note.format("scan_a") + apd_line("scan_a") + "done\n")
    # with it: apd_segment before the command of every scan without masks, and only there
    seg_line = "/x/bin/apd_segment --dense_folder {0} --device 0 >> {0}/APD/segment_log.txt\n"
    assert review("--flat_zone_masks") == (head.format(root, ", flat_zone_masks=True") + seg_line.format(root / "scan_c") +
                                           apd_line("scan_c") + apd_line("scan_b") + seg_line.format(root / "scan_a") +
                                           apd_line("scan_a") + "done\n")
    # --no_sam: the scans run without masks, so none are made
    assert "apd_segment" not in review("--flat_zone_masks", "--no_sam")
