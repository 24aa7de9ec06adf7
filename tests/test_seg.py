"""Flat-zone sa_masks on the GPU (csrc/apd_seg.hip): the connected-component kernels on masks that no
image produces, at sizes that span several 64 x 16 tiles and a partial one in both directions; the five
stages against the host twin and the numpy restatement (tests/seg_lib.py), every stage read back;
run-to-run identity on one context; status codes; and `apd_segment` followed by `apd --use_sa true`.
Everything is integer: every comparison is exact."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import apd_abi as A
import host_schedule as HS
import seg_lib as L
import synth

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -5
APD_SEGMENT = os.path.join(A.HERE, "host", "build", "apd_segment")
APD = os.path.join(A.HERE, "host", "build", "apd")


@pytest.fixture(scope="module")
def lib():
    return A.load_library()


@pytest.fixture(scope="module")
def eng(lib):
    e = A.SegEngine(0, lib)
    yield e
    e.close()


# ---- 1. the labelling alone ----------------------------------------------------------------------------

# 136 x 200 (H x W): 3 tiles and 8 columns, 8 tiles and 8 rows; the thin ones are a single partial tile row or
# column; 16 x 64, 17 x 65 and 32 x 128 sit on the tile borders themselves
MASK_SIZES = [(136, 200), (1, 1), (1, 97), (97, 1), (1, 200), (136, 1), (16, 64), (17, 65), (32, 128)]
MASK_NAMES = list(L.mask_cases(3, 3))


@pytest.fixture(scope="module")
def masks():
    out = {}
    for H, W in MASK_SIZES:
        for name, m in L.mask_cases(H, W, seed=H * 1000 + W).items():
            out[(H, W, name)] = (m, L.label_mask(m))
    return out


@pytest.mark.parametrize("name", MASK_NAMES)
@pytest.mark.parametrize("size", MASK_SIZES, ids=["%dx%d" % s for s in MASK_SIZES])
def test_label_mask_equals_the_restatement(eng, masks, size, name):
    mask, want = masks[size + (name,)]
    got = eng.label_mask(mask)
    assert got.dtype == np.int32 and got.shape == want.shape
    assert np.array_equal(got, want), int((got != want).sum())
    assert np.array_equal(eng.stage("roots"), want) and np.array_equal(eng.stage("flat"), mask)
    areas = eng.stage("areas").ravel()
    assert np.array_equal(areas, np.bincount(want[want >= 0], minlength=want.size))


def test_label_mask_longest_chains(eng, masks):
    """A serpentine and a spiral through every tile: one component each, its root the first pixel"""
    for name in ("serpentine", "spiral", "ones", "comb"):
        mask, _ = masks[(136, 200, name)]
        got = eng.label_mask(mask)
        assert (got[mask != 0] == 0).all() and (got[mask == 0] == -1).all(), name


def test_label_mask_large_random(lib, eng):
    """1031 x 517 at density 0.59, near the percolation threshold: large tortuous components across hundreds
    of tiles; against the host twin, with a device-resident mask as well"""
    import torch
    mask = (np.random.default_rng(59).random((517, 1031)) < 0.59).astype(np.uint8)
    want = A.seg_label_mask_host(mask, lib)
    assert np.array_equal(eng.label_mask(mask), want)
    got = eng.label_mask(torch.from_numpy(mask).to("cuda:0"))
    assert got.is_cuda and np.array_equal(got.cpu().numpy(), want)
    sizes = np.bincount(want[want >= 0])
    print("components: %d, the largest %d of %d set pixels" % ((sizes > 0).sum(), sizes.max(), (mask != 0).sum()))
    assert sizes.max() > 10000


# ---- 2. the five stages --------------------------------------------------------------------------------

CASES = L.KNOWN_CASES + L.IMAGE_CASES


@pytest.fixture(scope="module")
def references(lib):
    out = {}
    for name, make, max_size, q8, min_area in CASES:
        img = make()
        out[name] = (img, A.seg_flat_zones_host(img, max_size, q8 / 256.0, min_area, stages=True, lib=lib),
                     L.flat_zones(img, max_size, q8, min_area))
    return out


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_flat_zones_equal_host_and_restatement(eng, references, case, where):
    name, _, max_size, q8, min_area = case
    img, host, restated = references[name]
    src = img
    if where == "device":
        import torch
        src = torch.from_numpy(img).to("cuda:0")
    labels, ns, nl = eng.flat_zones(src, max_size, q8 / 256.0, min_area)
    if where == "device":
        assert labels.is_cuda
        labels = labels.cpu().numpy()
    for st_name in A.SEG_STAGES:  # in the stages' order: the first that differs is named
        got = eng.stage(st_name)
        assert got.shape == host[3][st_name].shape, st_name
        assert np.array_equal(got, host[3][st_name]), "%s differs from the host twin" % st_name
        assert np.array_equal(got, restated[3][st_name]), "%s differs from the restatement" % st_name
    assert (ns, nl) == host[1:3] == restated[1:3]
    assert np.array_equal(labels, host[0]) and np.array_equal(labels, restated[0])
    t = eng.timing()
    assert list(t) == A.SEG_TIMES and all(v >= 0 for v in t.values())
    if A.seg_working_size(img.shape[1], img.shape[0], max_size)[0] > 1:
        assert t["downscale_ms"] > 0


def test_known_answers_on_the_device(eng, references):
    labels, ns, nl = eng.flat_zones(references["constant"][0], 0, 1.0, 1)
    assert (ns, nl) == (1, 1) and (labels == 1).all() and eng.stage("areas")[0, 0] == 1200
    labels, ns, nl = eng.flat_zones(references["step/256"][0], 0, 1.0, 1)
    assert (ns, nl) == (2, 2) and (labels[:, :18] == 2).all() and not labels[:, 18:22].any() and (labels[:, 22:] == 1).all()
    labels, ns, nl = eng.flat_zones(references["step/255"][0], 0, 255 / 256.0, 1)
    assert (labels[:, :17] == 2).all() and not labels[:, 17:23].any() and (labels[:, 23:] == 1).all()
    labels, ns, nl = eng.flat_zones(references["squares"][0], 0, 1.0, 1)
    assert ns > 255 and nl == 255 and labels.max() == 255


def test_run_to_run_identity(eng, references):
    """The same call twice, and again after a larger and a smaller call on the same context: buffers are
    kept and grown, nothing of an earlier call shows"""
    img = references["random"][0]
    big = L.patches_image(300, 400, 21)

    def run(image, max_size):
        labels, ns, nl = eng.flat_zones(image, max_size, 1.0, 2)
        return [labels, ns, nl] + [eng.stage(s) for s in A.SEG_STAGES]

    def same(a, b):
        return all(np.array_equal(x, y) for x, y in zip(a, b))

    first = run(img, 0)
    assert same(first, run(img, 0))
    big_first = run(big, 0)
    assert same(first, run(img, 0))
    run(img[:20, :30].copy(), 0)
    eng.label_mask(L.serpentine(50, 70))
    assert same(first, run(img, 0)) and same(big_first, run(big, 0))
    small = run(big, 100)  # s = 4 after s = 1
    assert small[0].shape == (75, 100) and same(small, run(big, 100))


# ---- 3. status codes -----------------------------------------------------------------------------------

def test_rejected_arguments_and_states(lib):
    e = A.SegEngine(0, lib)
    out = np.zeros(4 * 6 * 3, np.uint16)
    for which in range(5):
        assert lib.apd_seg_get_stage(e.ctx, which, out.ctypes.data) == ESTATE  # before any call
    assert lib.apd_seg_get_stage(e.ctx, 5, out.ctypes.data) == EINVAL and lib.apd_seg_get_stage(e.ctx, -1, out.ctypes.data) == EINVAL
    img = np.zeros((4, 6, 3), np.uint8)
    labels = np.zeros((4, 6), np.uint8)
    ow, oh = A.C.c_int32(), A.C.c_int32()

    def call(w=6, h=4, src=img, max_size=0, q8=256, min_area=1, labels=labels, pw=ow, ph=oh):
        ptr = lambda a: None if a is None else a.ctypes.data
        ref = lambda v: None if v is None else A.C.byref(v)
        return lib.apd_seg_flat_zones_bgr8(e.ctx, w, h, ptr(src), max_size, q8, min_area, ptr(labels), ref(pw), ref(ph), None, None)

    assert call(w=0) == EINVAL and call(h=0) == EINVAL and call(w=65537) == EINVAL and call(h=-1) == EINVAL
    assert call(w=65536, h=65536) == EINVAL
    assert call(max_size=-1) == EINVAL
    assert call(q8=-1) == EINVAL and call(q8=65281) == EINVAL
    assert call(min_area=0) == EINVAL
    assert call(src=None) == EINVAL and call(labels=None) == EINVAL and call(pw=None) == EINVAL and call(ph=None) == EINVAL
    assert b"apd_seg_flat_zones_bgr8" in lib.apd_seg_last_error(e.ctx)
    assert lib.apd_seg_get_stage(e.ctx, 2, out.ctypes.data) == ESTATE  # a rejected call leaves no stage
    assert call() == 0 and (ow.value, oh.value) == (6, 4) and (labels == 1).all()
    assert call(q8=65280) == 0 and call(q8=0) == 0
    for which in range(5):
        assert lib.apd_seg_get_stage(e.ctx, which, out.ctypes.data) == 0
    assert lib.apd_seg_get_stage(e.ctx, 2, None) == EINVAL
    mask = np.ones((4, 6), np.uint8)
    roots = np.zeros((4, 6), np.int32)
    lm = lambda W, H, m, r: lib.apd_seg_label_mask(e.ctx, W, H, None if m is None else m.ctypes.data, None if r is None else r.ctypes.data)
    assert lm(0, 4, mask, roots) == EINVAL and lm(6, 65537, mask, roots) == EINVAL and lm(65536, 65536, mask, roots) == EINVAL
    assert lm(6, 4, None, roots) == EINVAL and lm(6, 4, mask, None) == EINVAL
    assert lm(6, 4, mask, roots) == 0 and not roots.any()
    assert lib.apd_seg_get_stage(e.ctx, 0, out.ctypes.data) == ESTATE and lib.apd_seg_get_stage(e.ctx, 1, out.ctypes.data) == ESTATE
    assert lib.apd_seg_get_stage(e.ctx, 3, out.ctypes.data) == 0
    with pytest.raises(A.ApdError, match="APD_ESTATE"):
        e.stage("smooth")
    e.close()


# ---- 4. the binaries -----------------------------------------------------------------------------------

def test_apd_segment_then_apd(tmp_path):
    """`apd_segment` on a 3-view 160 x 120 scan writes what `apd_segment --host` writes, byte for byte, and
    `apd --use_sa true` then finds and reads the folder."""
    sc = synth.make_scene(160, 120, 2, seed=9)
    dev, host = str(tmp_path / "dev"), str(tmp_path / "host")
    HS.write_dense_folder(sc, dev, ext=".png")
    shutil.copytree(dev, host)
    args = ["--min_area", "64"]
    r = subprocess.run([APD_SEGMENT, "--dense_folder", dev, *args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    h = subprocess.run([APD_SEGMENT, "--dense_folder", host, "--host", *args], capture_output=True, text=True, timeout=300)
    assert h.returncode == 0, h.stderr[-2000:]
    names = sorted(os.listdir(os.path.join(host, "sa_masks")))
    assert names == sorted(os.listdir(os.path.join(dev, "sa_masks"))) and len(names) == 6
    for n in names:
        with open(os.path.join(dev, "sa_masks", n), "rb") as a, open(os.path.join(host, "sa_masks", n), "rb") as b:
            assert a.read() == b.read(), n
    out = json.loads(r.stdout.strip().splitlines()[-1])
    print(out)
    assert out["views"] == 3 and out["host"] is False and all(v["labels"] >= 1 for v in out["per_view"])
    assert [v["labels"] for v in out["per_view"]] == [v["labels"] for v in json.loads(h.stdout.strip().splitlines()[-1])["per_view"]]
    assert synth.read_bin_mat(os.path.join(dev, "sa_masks", "00000000.bin")).shape == (120, 160)
    p = subprocess.run([APD, "--dense_folder", dev, "--dataset", "ETH3D", "--no_fuse", "true", "--use_sa", "true"],
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    assert "Can't find sa mask folder" not in p.stdout and "Error opening file" not in p.stdout
    assert os.path.exists(os.path.join(dev, "APD", "00000000", "depths.bin"))
