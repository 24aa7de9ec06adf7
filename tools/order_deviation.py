#!/usr/bin/env python3
"""Gauss-Seidel vs Jacobi on one synthetic scan, measured with apd_eval.

Writes a synthetic scan (default: C1 shape, 640x480, N = 4), runs `apd` on two copies of it with
`--ordering sequential` and `--ordering jacobi` (fusion on), then runs `apd_eval`:
  depth mode  sequential --against jacobi, and each run --gt_depth the rendered ground truth;
  cloud mode  each run's APD.ply against synth.gt_cloud, and the two clouds against each other.
The collected JSON goes to --out (profiles/order_deviation_c1.json is the committed C1 result).

  python tools/order_deviation.py --out profiles/order_deviation_c1.json
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "apde-mvs_amd"))
import synth  # noqa: E402

BUILD = os.path.join(REPO, "apde-mvs_amd", "host", "build")
APD, APD_EVAL = os.path.join(BUILD, "apd"), os.path.join(BUILD, "apd_eval")


def run(cmd, limit):
    t0 = time.time()
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
    if p.returncode != 0:
        sys.exit(f"{' '.join(cmd)} -> {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
    return time.time() - t0


def evaluate(args, tmp, limit):
    out = os.path.join(tmp, "eval.json")
    run([APD_EVAL, *args, "--json", out], limit)
    with open(out) as fh:
        return json.load(fh)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--num_src", type=int, default=4)
    ap.add_argument("--seed", type=int, default=20251114)
    ap.add_argument("--gpu", default="0")
    ap.add_argument("--limit", type=int, default=600, help="time limit of each child process, seconds")
    ap.add_argument("--out", required=True)
    a = ap.parse_args()

    scene = synth.make_scene(a.width, a.height, a.num_src, seed=a.seed)
    res = {"scan": {"width": a.width, "height": a.height, "views": a.num_src + 1, "seed": a.seed,
                    "scene": "synth.make_scene"},
           "definition": "apd_eval: plain nearest-neighbour cloud metrics; depth validity = depth > 0 and "
                         "weak != UNKNOWN", "apd_seconds": {}}
    with tempfile.TemporaryDirectory() as tmp:
        gt_ply, gt_depth = os.path.join(tmp, "gt.ply"), os.path.join(tmp, "gt_depth")
        synth.write_ply(gt_ply, synth.gt_cloud(scene))
        synth.write_gt_depths(scene, gt_depth)
        folders = {}
        for order in ("sequential", "jacobi"):
            folders[order] = os.path.join(tmp, order)
            synth.write_scan(scene, folders[order], ext=".png")  # PGM bytes: apd's decoders go by content
            res["apd_seconds"][order] = round(run(
                [APD, "--dense_folder", folders[order], "--dataset", "ETH3D", "--memory_cache", "false",
                 "--gpus", a.gpu, "--ordering", order], a.limit), 2)
        seq, jac = folders["sequential"], folders["jacobi"]
        res["depth_sequential_vs_jacobi"] = evaluate(["--dense_folder", seq, "--against", jac], tmp, a.limit)["depth"]
        for order, f in folders.items():
            r = evaluate(["--dense_folder", f, "--gt_depth", gt_depth, "--cloud", os.path.join(f, "APD", "APD.ply"),
                          "--gt", gt_ply, "--gpu_index", a.gpu.split(",")[0]], tmp, a.limit)
            res[f"depth_{order}_vs_gt"] = r["depth"]
            res[f"cloud_{order}_vs_gt"] = r["cloud"]
        res["cloud_sequential_vs_jacobi"] = evaluate(
            ["--cloud", os.path.join(seq, "APD", "APD.ply"), "--gt", os.path.join(jac, "APD", "APD.ply"),
             "--gpu_index", a.gpu.split(",")[0]], tmp, a.limit)["cloud"]
    for k in list(res):  # temporary paths say nothing about the result
        if isinstance(res[k], dict):
            res[k].pop("a", None)
            res[k].pop("b", None)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    t = res["depth_sequential_vs_jacobi"]["total"]
    print(json.dumps({"apd_seconds": res["apd_seconds"], "seq_vs_jac_total": t,
                      "f1_sequential": res["cloud_sequential_vs_gt"]["f1"],
                      "f1_jacobi": res["cloud_jacobi_vs_gt"]["f1"]}))


if __name__ == "__main__":
    main()
