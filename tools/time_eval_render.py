#!/usr/bin/env python3
"""Time apd_eval's z-buffer renderer and visibility count on surface-like clouds of growing size.

Each case: n points on the wavy sheet of tools/time_eval.py (x, y uniform over a 10 x 10 square, z about
6, millimetre noise) rendered into one 6048 x 4032 view that looks straight at the sheet, at splat 0, 1
and 2, with the points offered to the splat kernel in input order and in Morton order (a fresh
context per order: APD_EVAL_RENDER_ORDER is read when the context is created). Reports the
device-event render_ms (sort, where there is one, + clear + splat + resolve) and visibility_ms
(against the map just rendered), median of --repeat, and the rates they imply. The same view rendered
four times in one call separates what a further view costs from what a call costs (the sort):

  offered   = pixels of all footprints inside the image, the key updates the kernel considers
  covered   = pixels that end up covered: each needed at least one atomic
The atomics actually issued lie between the two (the plain load in front of the atomic skips a key
that cannot win), so offered / time bounds the atomic rate from above and covered / time from below.

For sizes up to --host_max the float32 numpy reference of tests/render_lib.py is timed on the host
on the same input and the device maps are checked against it bit for bit.

  python tools/time_eval_render.py --out profiles/eval_render_timing.json
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
from render_lib import make_cam, project_ref, render_ref, sheet, visible_ref  # noqa: E402


def median(v):
    return sorted(v)[len(v) // 2]


def offered_updates(cloud, cam, splat, W, H):
    kept, d, u, v = project_ref(cloud, cam)
    u, v = u[kept], v[kept]
    nx = np.clip(np.minimum(u + splat, W - 1) - np.maximum(u - splat, 0) + 1, 0, None)
    ny = np.clip(np.minimum(v + splat, H - 1) - np.maximum(v - splat, 0) + 1, 0, None)
    return int((nx * ny).sum())


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default="100000,1000000,10000000")
    ap.add_argument("--width", type=int, default=6048)
    ap.add_argument("--height", type=int, default=4032)
    ap.add_argument("--splats", default="0,1,2")
    ap.add_argument("--rel_tol", type=float, default=0.01)
    ap.add_argument("--host_max", type=int, default=1000000)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    W, H = a.width, a.height
    f = 3500.0 * W / 6048.0
    cam = make_cam([[f, 0, W / 2], [0, f, H / 2], [0, 0, 1]], np.eye(3), [0, 0, 0], W, H)
    splats = [int(s) for s in a.splats.split(",")]
    rows = []
    for n in [int(s) for s in a.sizes.split(",")]:
        cloud = sheet(np.random.default_rng(1), n)
        for splat in splats:
            row = {"points": n, "width": W, "height": H, "views": 1, "splat": splat,
                   "offered_updates": offered_updates(cloud, cam, splat, W, H)}
            maps = {}
            for order in ("input", "morton"):
                os.environ["APD_EVAL_RENDER_ORDER"] = order
                eng = A.EvalEngine(0)
                rt, vt, r4 = [], [], []
                for _ in range(a.repeat + 1):  # the first pass grows the context's buffers and is dropped
                    dep = eng.render_depth(cloud, [cam], splat)[0]
                    seen, n_any = eng.visibility(cloud, [cam], [dep], a.rel_tol, want_any=True)
                    tm = eng.render_timing()
                    rt.append(tm["render_ms"])
                    vt.append(tm["visibility_ms"])
                    eng.render_depth(cloud, [cam] * 4, splat)  # the same view four times in one call
                    r4.append(eng.render_timing()["render_ms"])
                eng.close()
                maps[order] = dep
                r, v = median(rt[1:]), median(vt[1:])
                covered = int((dep > 0).sum())
                per_view = (median(r4[1:]) - r) / 3  # what a further view costs; the rest is per call (the sort)
                row[order] = {"render_ms": r, "visibility_ms": v, "render_ms_runs": rt[1:], "render_ms_4_views": median(r4[1:]),
                              "per_further_view_ms": per_view, "per_call_ms": r - per_view,
                              "covered_pixels": covered, "visible_points": n_any,
                              "offered_updates_per_s": row["offered_updates"] / r * 1e3,
                              "covered_pixels_per_s": covered / r * 1e3, "points_per_s_visibility": n / v * 1e3}
            row["orders_agree"] = bool(np.array_equal(maps["input"].view(np.uint32), maps["morton"].view(np.uint32)))
            if n <= a.host_max:
                t0 = time.perf_counter()
                rd, _ = render_ref(cloud, cam, splat)
                t1 = time.perf_counter()
                vis = visible_ref(cloud, cam, rd, a.rel_tol)
                t2 = time.perf_counter()
                row["host_numpy"] = {"render_ms": (t1 - t0) * 1e3, "visibility_ms": (t2 - t1) * 1e3,
                                     "matches_device": bool(np.array_equal(rd.view(np.uint32),
                                                                           maps["morton"].view(np.uint32))
                                                            and int(vis.sum()) == row["morton"]["visible_points"])}
            rows.append(row)
            print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump({"tool": "tools/time_eval_render.py", "device_times": "hipEvent, median of %d" % a.repeat,
                       "cases": rows}, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
