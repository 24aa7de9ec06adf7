#!/usr/bin/env python3
"""Time apd_eval's free-gap test and voxel scores on surface-like clouds of growing size.

Each case: a ground-truth cloud of n points on the wavy sheet of tools/time_eval.py (x, y uniform over
a 10 x 10 square, z about 6, millimetre noise) seen by two scanner positions above it, and a
reconstruction of n points on the same sheet with centimetre noise.

  free_gap      the reconstruction against the 12 cube-map faces (--cube_size, 2048) of the two
                scanners, rendered from the ground truth at --splat (the render time is reported too)
  voxel_scores  the reconstruction with its distances to the ground truth, 6 tolerances, at voxel 0.01
                and 0.05, with and without the gap
  voxel_downsample  on the same cloud and voxel: it shares the key-and-sort path, so the difference is
                what the per-tolerance scans and sums cost

Device-event times, median of --repeat after a warm-up call that grows the context's buffers. For sizes
up to --host_max the numpy restatement of tests/protocol_lib.py is timed on the host on the same input
and the device results are checked against it (bits, integers).

  python tools/time_eval_protocol.py --out profiles/eval_protocol_timing.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "apde-mvs_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))
import apd_abi as A  # noqa: E402
from protocol_lib import free_gap_ref, scores_equal, voxel_scores_ref  # noqa: E402
from render_lib import sheet  # noqa: E402

ORIGINS = [(-2.0, -1.0, 1.0), (2.5, 1.5, 2.0)]


def median(v):
    return sorted(v)[len(v) // 2]


def timed(repeat, call, read):
    """median of `read()` over `repeat` calls after one warm-up; the last result"""
    out, ms = None, []
    for _ in range(repeat + 1):
        out = call()
        ms.append(read())
    return out, median(ms[1:]), ms[1:]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default="100000,1000000,10000000")
    ap.add_argument("--cube_size", type=int, default=2048)
    ap.add_argument("--splat", type=int, default=1)
    ap.add_argument("--voxels", default="0.01,0.05")
    ap.add_argument("--host_max", type=int, default=1000000)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    tol = A.ETH3D_TOLERANCES
    eng = A.EvalEngine(0)
    cams = [c for o in ORIGINS for c in A.cube_cameras(o, a.cube_size, eng.lib)]
    rows = []
    for n in [int(s) for s in a.sizes.split(",")]:
        gt = sheet(np.random.default_rng(1), n)
        rec = sheet(np.random.default_rng(2), n, noise=0.01)
        row = {"points": n, "faces": len(cams), "cube_size": a.cube_size, "splat": a.splat, "tolerances": len(tol)}
        maps, row["render_ms"], _ = timed(a.repeat, lambda: eng.render_depth(gt, cams, a.splat),
                                          lambda: eng.render_timing()["render_ms"])
        gap, row["free_gap_ms"], row["free_gap_ms_runs"] = timed(a.repeat, lambda: eng.free_gap(rec, cams, maps),
                                                                 lambda: eng.protocol_timing()["free_gap_ms"])
        row["points_per_s_free_gap"] = n / row["free_gap_ms"] * 1e3
        row["gap_finite"] = int(np.isfinite(gap).sum())
        eng.set_target(gt)
        dist, _ = eng.distances(rec, max(tol))
        row["voxel"] = []
        host = {}
        for voxel in [float(v) for v in a.voxels.split(",")]:
            v = {"voxel": voxel}
            keep, v["voxel_downsample_ms"], _ = timed(a.repeat, lambda: eng.voxel_downsample(rec, voxel),
                                                      lambda: eng.timing()["voxel_ms"])
            v["voxels_occupied"] = int(len(keep))
            for name, g in (("with_gap", gap), ("without_gap", None)):
                sc, ms, runs = timed(a.repeat, lambda: eng.voxel_scores(rec, voxel, dist, g, tol),
                                     lambda: eng.protocol_timing()["scores_ms"])
                v[name] = {"scores_ms": ms, "scores_ms_runs": runs, "over_downsample": ms / v["voxel_downsample_ms"],
                           "good": [int(x) for x in sc["good"]], "bad": [int(x) for x in sc["bad"]],
                           "voxels": [int(x) for x in sc["voxels"]], "score": sc["score"]}
                host[(voxel, name)] = sc
            row["voxel"].append(v)
        if n <= a.host_max:
            t0 = time.perf_counter()
            want_gap = free_gap_ref(rec, cams, maps)
            t1 = time.perf_counter()
            ok = bool(np.array_equal(want_gap.view(np.uint32), gap.view(np.uint32)))
            hs = {"free_gap_ms": (t1 - t0) * 1e3}
            for v in row["voxel"]:
                t0 = time.perf_counter()
                want = voxel_scores_ref(rec, v["voxel"], dist, gap, tol)
                hs["scores_ms_voxel_%g" % v["voxel"]] = (time.perf_counter() - t0) * 1e3
                ok = ok and scores_equal(host[(v["voxel"], "with_gap")], want)
            hs["matches_device"] = ok
            row["host_numpy"] = hs
        rows.append(row)
        print(json.dumps(row), flush=True)
    eng.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump({"tool": "tools/time_eval_protocol.py", "device_times": "hipEvent, median of %d" % a.repeat,
                       "scanner_origins": ORIGINS, "cases": rows}, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
