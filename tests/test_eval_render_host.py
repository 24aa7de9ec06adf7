"""The host side of `apd_eval`'s render / visibility options, without a GPU: every argument error and
unreadable input exits 2 before a device is touched, --help names the new options and keeps the
caveat, and the library exports the new entries."""
import os
import subprocess

import numpy as np
import pytest

import apd_abi as A
import synth
from eval_lib import APD_EVAL, f32

NO_GPU = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
NEW_SYMBOLS = ["apd_eval_render_depth", "apd_eval_visibility", "apd_eval_get_render_timing"]


def run_eval(*args):
    return subprocess.run([APD_EVAL, *map(str, args)], capture_output=True, text=True, timeout=120, env=NO_GPU)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("render_host")
    sc = synth.make_scene(48, 36, 2)
    synth.write_scan(sc, str(d / "scan"), ext=".png")
    synth.write_ply(str(d / "gt.ply"), synth.gt_cloud(sc))
    synth.write_ply(str(d / "rec.ply"), synth.gt_cloud(sc)[::3])
    (d / "bad.ply").write_bytes(b"ply\nformat ascii 1.0\nelement vertex 1\nproperty float x\nend_header\n0\n")
    for i, g in enumerate(sc.gt_depth):
        v = d / "scan" / "APD" / f"{i:08d}"
        os.makedirs(v)
        synth.write_bin_mat(str(v / "depths.bin"), g)
        synth.write_bin_mat(str(v / "weak.bin"), np.ones(g.shape, np.uint8))
    return d


def test_new_bad_arguments(files):
    gt, rec, scan, out = files / "gt.ply", files / "rec.ply", files / "scan", files / "out"
    render = ("--render_gt", gt, "--scan", scan, "--out", out)
    cloud = ("--cloud", rec, "--gt", gt)
    for args in [("--render_gt", gt), ("--render_gt", gt, "--scan", scan), ("--render_gt", gt, "--out", out),
                 (*render, "--splat", -1), (*render, "--splat", 17), (*render, "--splat", "x"),
                 (*cloud, "--scan", scan, "--visible_views", 0), (*cloud, "--scan", scan, "--visible_views", -2),
                 (*cloud, "--visible_views", 2), (*cloud, "--scan", scan), ("--scan", scan),
                 ("--scan", scan, "--visible_views", 2), (*cloud, "--scan", scan, "--visible_views", 2, "--occlusion_tol", -1),
                 (*cloud, "--occlusion_tol", 0.01), (*cloud, "--splat", 1), ("--out", out),
                 ("--dense_folder", scan, "--gt_cloud", gt, "--against", scan),
                 ("--dense_folder", scan, "--gt_cloud", gt, "--gt_depth", scan), ("--gt_cloud", gt)]:
        p = run_eval(*args)
        assert p.returncode == 2, (args, p.stdout, p.stderr)
        assert "device" not in p.stderr and p.stderr.startswith("apd_eval: ")
    assert not out.exists()


def test_unreadable_inputs_exit_2_before_any_device(files, tmp_path):
    gt, rec, scan, bad = files / "gt.ply", files / "rec.ply", files / "scan", files / "bad.ply"
    nowhere = tmp_path / "nowhere"
    no_cams = tmp_path / "no_cams"
    os.makedirs(no_cams / "images")
    (no_cams / "pair.txt").write_text((scan / "pair.txt").read_text())
    no_images = tmp_path / "no_images"
    os.makedirs(no_images / "cams")
    (no_images / "pair.txt").write_text((scan / "pair.txt").read_text())
    for f in os.listdir(scan / "cams"):
        (no_images / "cams" / f).write_text((scan / "cams" / f).read_text())
    out = tmp_path / "out"
    for args in [("--render_gt", bad, "--scan", scan, "--out", out), ("--render_gt", nowhere, "--scan", scan, "--out", out),
                 ("--render_gt", gt, "--scan", nowhere, "--out", out), ("--render_gt", gt, "--scan", no_cams, "--out", out),
                 ("--render_gt", gt, "--scan", no_images, "--out", out),
                 ("--dense_folder", scan, "--gt_cloud", bad), ("--dense_folder", scan, "--gt_cloud", nowhere),
                 ("--dense_folder", nowhere, "--gt_cloud", gt),
                 ("--cloud", rec, "--gt", gt, "--scan", nowhere, "--visible_views", 1),
                 ("--cloud", rec, "--gt", bad, "--scan", scan, "--visible_views", 1),
                 # a second mode's unreadable input stops the first mode as well
                 ("--dense_folder", scan, "--gt_cloud", gt, "--cloud", rec, "--gt", bad)]:
        p = run_eval(*args, "--json", tmp_path / "o.json")
        assert p.returncode == 2, (args, p.stdout, p.stderr)
        assert "device" not in p.stderr and len(p.stderr.strip()) > 20 and p.stdout == ""
    assert not out.exists() and not (tmp_path / "o.json").exists()


@pytest.mark.parametrize("args", [("--render_gt", "gt.ply", "--scan", "scan", "--out", "OUT"),
                                  ("--dense_folder", "scan", "--gt_cloud", "gt.ply"),
                                  ("--cloud", "rec.ply", "--gt", "gt.ply", "--scan", "scan", "--visible_views", 2,
                                   "--splat", 1, "--occlusion_tol", 0.02)])
def test_valid_invocations_reach_the_device(files, tmp_path, args):
    """Everything parses, so the tool goes on to the device and fails THERE (status 1, not 2) on a
    machine with no visible GPU."""
    args = [tmp_path / "OUT" if a == "OUT" else files / a if isinstance(a, str) and not a.startswith("--") else a
            for a in args]
    p = run_eval(*args)
    assert p.returncode == 1, (p.stdout, p.stderr)
    assert "device" in p.stderr


def test_help_names_the_new_options_and_keeps_the_caveat():
    p = run_eval("--help")
    assert p.returncode == 0
    for word in ("--render_gt", "--scan", "--out", "--splat", "--gt_cloud", "--visible_views", "--occlusion_tol",
                 "--gt_depth", "--against", "visibility", "z-buffer", "NOT ETH3D's free-space model", "NOT modelled"):
        assert word in p.stdout, word


def test_library_exports_the_render_entries():
    assert all(s in A.EVAL_EXPORTS for s in NEW_SYMBOLS)
    lib = A.load_library()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s), s
    assert lib.apd_eval_render_depth.argtypes[4]._type_ is A.ApdCamera
    # a NULL context is refused without touching a device
    assert lib.apd_eval_render_depth(None, 0, None, 0, None, 0, None, None) == -1
    assert lib.apd_eval_visibility(None, 0, None, 0, None, None, 0.0, None, None) == -1
    assert lib.apd_eval_get_render_timing(None, None, None) == -1


def test_camera_from_values_round_trip():
    sc = synth.make_scene(48, 36, 2)
    v = synth.camera_struct_values(sc.cameras[1], 48, 36)
    cam = A.camera_from_values(v)
    assert np.array_equal(np.array(cam.K[:], f32), v["K"]) and np.array_equal(np.array(cam.R[:], f32), v["R"])
    assert np.array_equal(np.array(cam.t[:], f32), v["t"]) and np.array_equal(np.array(cam.c[:], f32), v["c"])
    assert (cam.width, cam.height) == (48, 36) and cam.depth_num == v["depth_num"]
