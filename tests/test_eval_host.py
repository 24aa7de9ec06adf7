"""The host side of `apd_eval`, without a GPU: the PLY reader (valid layouts are read, malformed files
are rejected with status 2 before any device context exists), depth mode against numpy, and the
reader under AddressSanitizer + UndefinedBehaviorSanitizer over a corrupted corpus (a stand-alone
program, run directly)."""
import json
import os
import subprocess

import numpy as np
import pytest

import synth
from eval_lib import APD_EVAL, HOST, f32, plane_pair, ply_apd_layout, ply_gt_layout

SAN_BIN = os.path.join(HOST, "build-san", "ply_corpus_main")
# no device is visible to the child: whatever it reports was decided on the host
NO_GPU = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")


def run_eval(*args):
    return subprocess.run([APD_EVAL, *map(str, args)], capture_output=True, text=True, timeout=120, env=NO_GPU)


@pytest.fixture(scope="module")
def plys(tmp_path_factory):
    d = tmp_path_factory.mktemp("plys")
    rng = np.random.default_rng(21)
    rec, gt = plane_pair(rng, 400)
    (d / "apd15.ply").write_bytes(ply_apd_layout(rec, rng))
    (d / "gt_extra.ply").write_bytes(ply_gt_layout(gt))
    synth.write_ply(str(d / "plain12.ply"), rec)
    (d / "empty_cloud.ply").write_bytes(ply_apd_layout(np.zeros((0, 3), f32)))
    return d


def _bad_plys():
    xyz = np.arange(30, dtype="<f4").reshape(10, 3)
    body = xyz.tobytes()
    props = "property float x\nproperty float y\nproperty float z\n"

    def hdr(fmt="binary_little_endian 1.0", n=10, p=props):
        return ("ply\nformat %s\nelement vertex %d\n%send_header\n" % (fmt, n, p)).encode()
    return {
        "ascii": hdr("ascii 1.0") + b"\n".join(b"%f %f %f" % tuple(r) for r in xyz) + b"\n",
        "big_endian": hdr("binary_big_endian 1.0") + xyz.astype(">f4").tobytes(),
        "list_property": hdr(p=props + "property list uchar int idx\n") + body,
        "missing_z": hdr(p="property float x\nproperty float y\nproperty float w\n") + body,
        "double_z": hdr(p="property float x\nproperty float y\nproperty double z\n") + body + body,
        "count_too_large": hdr(n=1 << 40) + body,
        "count_one_too_many": hdr(n=11) + body,
        "truncated_body": hdr() + body[:-5],
        "truncated_header": hdr()[:-8],
        "empty": b"",
        "not_ply": b"P5\n4 4\n255\n" + bytes(16),
    }


@pytest.mark.parametrize("name", ["apd15.ply", "gt_extra.ply", "plain12.ply", "empty_cloud.ply"])
def test_valid_ply_gets_past_the_reader(plys, name):
    """Both files parse, so the tool goes on to the device and fails THERE (status 1, not 2), on a
    machine with no visible GPU."""
    p = run_eval("--cloud", plys / name, "--gt", plys / "gt_extra.ply")
    assert p.returncode == 1, (p.stdout, p.stderr)
    assert "device" in p.stderr and "Tolerances" not in p.stdout


@pytest.mark.parametrize("name", sorted(_bad_plys()))
@pytest.mark.parametrize("side", ["--cloud", "--gt"])
def test_bad_ply_is_rejected_on_the_host(plys, tmp_path, name, side):
    bad = tmp_path / (name + ".ply")
    bad.write_bytes(_bad_plys()[name])
    other = "--gt" if side == "--cloud" else "--cloud"
    p = run_eval(side, bad, other, plys / "apd15.ply", "--json", tmp_path / "o.json")
    assert p.returncode == 2, (p.stdout, p.stderr)
    assert str(bad) in p.stderr and len(p.stderr.strip()) > len(str(bad)) + 10  # a message, naming the file
    assert "device" not in p.stderr and not (tmp_path / "o.json").exists()


def test_bad_arguments():
    for args in [(), ("--cloud", "a.ply"), ("--dense_folder", "a"), ("--dense_folder", "a", "--against", "b",
                                                                       "--gt_depth", "c"),
                 ("--cloud", "a.ply", "--gt", "b.ply", "--tolerances", "0.1,x"),
                 ("--cloud", "a.ply", "--gt", "b.ply", "--max_dist", "0.1"), ("--frobnicate", "1")]:
        assert run_eval(*args).returncode == 2, args
    p = run_eval("--help")
    assert p.returncode == 0 and "visibility" in p.stdout and "--gt_depth" in p.stdout


# ---- depth mode ---------------------------------------------------------------------------------

UNKNOWN = 2


def _result_folder(root, depths, weaks):
    os.makedirs(root, exist_ok=True)
    with open(os.path.join(root, "pair.txt"), "w") as fh:
        fh.write(f"{len(depths)}\n")
        for i in range(len(depths)):
            fh.write(f"{i}\n2 {(i + 1) % len(depths)} 3.0 {(i + 2) % len(depths)} 1.0\n")
    for i, (d, w) in enumerate(zip(depths, weaks)):
        v = os.path.join(root, "APD", f"{i:08d}")
        os.makedirs(v, exist_ok=True)
        synth.write_bin_mat(os.path.join(v, "depths.bin"), d)
        if w is not None:
            synth.write_bin_mat(os.path.join(v, "weak.bin"), w)


def _depth_ref(da, wa, db, wb):
    va = (da > 0) & (wa != UNKNOWN)
    vb = (db > 0) & ((wb != UNKNOWN) if wb is not None else True)
    both = va & vb
    a, b = da[both].astype(np.float64), db[both].astype(np.float64)
    diff = np.abs(a - b)
    rel = diff / b
    s = {"pixels": int(da.size), "valid_a": int(va.sum()), "valid_b": int(vb.sum()), "valid_both": int(both.sum()),
         "mask_agree": int((va == vb).sum()), "within_1e-3": int((diff <= 1e-3 * b).sum()),
         "within_1e-2": int((diff <= 1e-2 * b).sum()),
         "median_rel": float(np.sort(rel)[(len(rel) - 1) // 2]) if len(rel) else 0.0}
    return s, rel


@pytest.fixture(scope="module")
def depth_folders(tmp_path_factory):
    root = tmp_path_factory.mktemp("depth")
    rng = np.random.default_rng(2)
    shapes = [(37, 53), (37, 53), (20, 31)]
    A_d, A_w, B_d, B_w, G = [], [], [], [], []
    for h, w in shapes:
        g = rng.uniform(2, 9, (h, w)).astype(f32)
        g[rng.random((h, w)) < 0.1] = 0  # no surface
        a = (g * (1 + rng.normal(0, 6e-3, (h, w)))).astype(f32)
        b = a.copy()
        m = rng.random((h, w))
        b[m < 0.3] *= f32(1.0005)   # known small and large deviations; the rest identical
        b[(m > 0.5) & (m < 0.7)] *= f32(1.004)
        b[m > 0.9] *= f32(1.05)
        a[rng.random((h, w)) < 0.05] = 0
        b[rng.random((h, w)) < 0.05] = 0
        a[0, 0], b[0, 0] = f32(-1.0), f32(4.0)
        wa = rng.integers(0, 3, (h, w)).astype(np.uint8)
        wb = np.where(rng.random((h, w)) < 0.9, wa, rng.integers(0, 3, (h, w))).astype(np.uint8)
        A_d.append(a), A_w.append(wa), B_d.append(b), B_w.append(wb), G.append(g)
    _result_folder(str(root / "A"), A_d, A_w)
    _result_folder(str(root / "B"), B_d, B_w)
    os.makedirs(root / "gt")
    for i, g in enumerate(G):
        synth.write_bin_mat(str(root / "gt" / f"{i:08d}.bin"), g)
    return root, A_d, A_w, B_d, B_w, G


@pytest.mark.parametrize("mode", ["against", "gt_depth"])
def test_depth_mode_matches_numpy(depth_folders, tmp_path, mode):
    root, A_d, A_w, B_d, B_w, G = depth_folders
    out = tmp_path / "d.json"
    other = ("--against", root / "B") if mode == "against" else ("--gt_depth", root / "gt")
    p = run_eval("--dense_folder", root / "A", *other, "--json", out)
    assert p.returncode == 0, (p.stdout, p.stderr)
    j = json.loads(out.read_text())["depth"]
    assert j["failed_views"] == 0 and len(j["views"]) == 3 and j["b_is_gt_depth"] == (mode == "gt_depth")
    rels, total = [], None
    for i, v in enumerate(j["views"]):
        want, rel = _depth_ref(A_d[i], A_w[i], B_d[i] if mode == "against" else G[i],
                               B_w[i] if mode == "against" else None)
        assert want["valid_both"] > 100 and 0 < want["within_1e-3"] < want["within_1e-2"] < want["valid_both"]
        assert v == dict(want, id=i)  # the median is the same double operations: exactly equal
        rels.append(rel)
        total = want if total is None else {k: total[k] + want[k] for k in want}
    allrel = np.sort(np.concatenate(rels))
    total["median_rel"] = float(allrel[(len(allrel) - 1) // 2])
    assert j["total"] == total
    assert "total:" in p.stdout and "view 2:" in p.stdout


def test_depth_mode_reports_a_size_mismatch(depth_folders, tmp_path):
    root, A_d, A_w, B_d, B_w, _ = depth_folders
    _result_folder(str(tmp_path / "C"), [B_d[0], B_d[1][:, :-1].copy(), B_d[2]], [B_w[0], B_w[1][:, :-1].copy(), B_w[2]])
    p = run_eval("--dense_folder", root / "A", "--against", tmp_path / "C", "--json", tmp_path / "c.json")
    assert p.returncode == 1
    j = json.loads((tmp_path / "c.json").read_text())["depth"]
    assert j["failed_views"] == 1 and "size mismatch" in j["views"][1]["error"] and "size mismatch" in p.stdout
    assert "error" not in j["views"][0] and j["total"]["pixels"] == A_d[0].size + A_d[2].size
    assert run_eval("--dense_folder", tmp_path / "nowhere", "--against", root / "B").returncode == 2


def test_synth_helpers(tmp_path):
    sc = synth.make_scene(48, 36, 2)
    cloud = synth.gt_cloud(sc)
    assert cloud.dtype == f32 and cloud.shape == (sum(int((d > 0).sum()) for d in sc.gt_depth), 3)
    # the points of view 1 project back onto view 1's pixel grid at the stored depth
    n0 = int((sc.gt_depth[0] > 0).sum())
    m = sc.gt_depth[1] > 0
    cam = sc.cameras[1]
    p = cam.K @ (cam.R @ cloud[n0:n0 + int(m.sum())].astype(np.float64).T + cam.t[:, None])
    ys, xs = np.nonzero(m)
    assert np.abs(p[0] / p[2] - xs).max() < 1e-3 and np.abs(p[1] / p[2] - ys).max() < 1e-3
    assert np.abs(p[2] - sc.gt_depth[1][m]).max() < 1e-4
    synth.write_ply(str(tmp_path / "c.ply"), cloud)
    raw = (tmp_path / "c.ply").read_bytes()
    assert raw.endswith(cloud.tobytes()) and b"element vertex %d\n" % len(cloud) in raw
    synth.write_gt_depths(sc, str(tmp_path / "gt"))
    assert np.array_equal(synth.read_bin_mat(str(tmp_path / "gt" / "00000002.bin")), sc.gt_depth[2])


# ---- the reader under sanitizers ------------------------------------------------------------------

def test_ply_reader_under_sanitizers(plys, tmp_path):
    r = subprocess.run(["make", "-C", HOST, "sanitize-ply"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    rng = np.random.default_rng(1)
    blobs = {n: (plys / n).read_bytes() for n in ("apd15.ply", "gt_extra.ply", "plain12.ply")}
    blobs.update({k + ".ply": v for k, v in _bad_plys().items()})
    body = np.arange(30, dtype="<f4").tobytes()
    for k, n in {"zero": 0, "huge31": (1 << 31) - 1, "huge63": (1 << 63) - 1, "huge64": 1 << 64, "neg": -4}.items():
        blobs[f"count_{k}.ply"] = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\n"
                                   "property float y\nproperty float z\nend_header\n" % n).encode() + body
    files = []
    for name, data in blobs.items():
        variants = {"": data}
        if data:
            for k, cut in enumerate(sorted(set(np.linspace(0, len(data) - 1, 40).astype(int).tolist()))):
                variants[f".cut{k}"] = data[:cut]
            head = data.find(b"end_header") + 11 if b"end_header" in data else len(data)
            for k in range(40):
                b = bytearray(data)
                for _ in range(int(rng.integers(1, 6))):  # mostly in the header, where the parsing is
                    hi = head if k % 4 else len(b)
                    b[int(rng.integers(0, max(hi, 1)))] = int(rng.integers(0, 256))
                variants[f".flip{k}"] = bytes(b)
        for suffix, blob in variants.items():
            p = tmp_path / (name + suffix)
            p.write_bytes(blob)
            files.append(str(p))
    files.append(str(tmp_path))           # a directory
    files.append(str(tmp_path / "none"))  # no such file
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([SAN_BIN, *files], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    read, rejected = (int(x) for x in r.stdout.split("ply corpus:")[1].replace("read,", "").replace("rejected", "").split())
    assert read + rejected == len(files) and read >= 3 and rejected >= len(_bad_plys())
