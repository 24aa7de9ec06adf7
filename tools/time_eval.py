#!/usr/bin/env python3
"""Time apd_eval's device library on surface-like clouds of growing size.

Each case: a ground-truth cloud of n points on a wavy sheet (x, y uniform over a square, millimetre
noise) and a reconstruction of n points on the same sheet with centimetre noise plus 2 % outliers
spread through the volume, i.e. points with no neighbour within max_dist, which is the case a ring
search over a fine grid degenerates on. Reports the device-event times of set_target / distances (both
directions) / voxel_downsample, and for sizes up to --host_max the wall time of scipy's cKDTree on
the host (16 workers, distance_upper_bound = max_dist) on the same clouds with its finite-count
checked against the device's.

  python tools/time_eval.py --sizes 100000,1000000,10000000 --out profiles/eval_timing.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "apde-mvs_amd"))
import apd_abi as A  # noqa: E402

TOL = list(A.ETH3D_TOLERANCES)


def sheet(rng, n, noise, side=10.0):
    xy = rng.uniform(-side / 2, side / 2, (n, 2))
    z = 6.0 + 0.3 * np.sin(xy[:, 0]) * np.cos(0.7 * xy[:, 1]) + rng.normal(0, noise, n)
    return np.column_stack([xy, z]).astype(np.float32)


def clouds(n, seed=1):
    rng = np.random.default_rng(seed)
    gt = sheet(rng, n, 0.001)
    rec = sheet(rng, n, 0.01)
    k = n // 50
    rec[rng.choice(n, k, replace=False)] = rng.uniform([-5, -5, 2], [5, 5, 10], (k, 3)).astype(np.float32)
    return rec, gt


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default="100000,1000000,10000000")
    ap.add_argument("--max_dist", type=float, default=0.5)
    ap.add_argument("--voxel", type=float, default=0.02)
    ap.add_argument("--host_max", type=int, default=1000000)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    eng = A.EvalEngine(0)
    rows = []
    for n in [int(s) for s in a.sizes.split(",")]:
        rec, gt = clouds(n)
        row = {"points": n, "max_dist": a.max_dist, "tolerances": TOL}
        for name, q, t in (("accuracy", rec, gt), ("completeness", gt, rec)):
            build, query = [], []
            for _ in range(a.repeat):  # the first repeat also grows the context's buffers
                t0 = time.perf_counter()
                eng.set_target(t)
                dist, within = eng.distances(q, a.max_dist, TOL)
                wall = (time.perf_counter() - t0) * 1e3
                tm = eng.timing()
                build.append(tm["build_ms"])
                query.append(tm["query_ms"])
            row[name] = {"build_ms": sorted(build)[len(build) // 2], "query_ms": sorted(query)[len(query) // 2],
                         "wall_ms_last": wall, "within": [int(w) for w in within],
                         "inf": int(np.isinf(dist).sum()),
                         "mquery_per_s": n / sorted(query)[len(query) // 2] / 1e3}
            if n <= a.host_max:
                from scipy.spatial import cKDTree
                t0 = time.perf_counter()
                tree = cKDTree(t)
                tb = time.perf_counter()
                hd, _ = tree.query(q, k=1, distance_upper_bound=a.max_dist, workers=16)
                row[name]["host_ckdtree"] = {"build_ms": (tb - t0) * 1e3, "query_ms": (time.perf_counter() - tb) * 1e3,
                                             "workers": 16, "inf": int(np.isinf(hd).sum())}
        vox = []
        for _ in range(a.repeat):
            keep = eng.voxel_downsample(rec, a.voxel)
            vox.append(eng.timing()["voxel_ms"])
        row["voxel"] = {"voxel": a.voxel, "kept": int(len(keep)), "voxel_ms": sorted(vox)[len(vox) // 2]}
        rows.append(row)
        print(json.dumps(row), flush=True)
    eng.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump({"tool": "tools/time_eval.py", "device_times": "hipEvent, median of %d" % a.repeat,
                       "cases": rows}, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
