#!/usr/bin/env python3
"""Time apd_prep (include/apd_prep.h) on synthetic sparse models of growing size.

Each case: n images on a ring, points seen by a window of neighbouring images whose length is
Poisson(8) (mean track length about 8), observations grouped by image. One more case has a few very
long tracks (points seen by every image) on top of ordinary ones, and one has few images and many
points (every pair of neighbours shares thousands of points: the same-address case).

  tracks   apd_prep_set_model: keys, radix sort, heads, scans (the upload is outside the events)
  pairs    apd_prep_pair_counts with per-workgroup LDS aggregation and with plain global atomics:
           the record kernel alone (records_ms) and the whole call's device time (clear, records,
           mirror)
  ranks    apd_prep_depth_ranks for the fractions 0.01 and 0.99

Device-event times, median of --repeat after a warm-up call that grows the context's buffers. For cases
of up to --host_max pair records the numpy restatement of tests/prep_lib.py is timed on the host on the
same input and the device results are checked against it (integers equal, doubles bit for bit).

  python tools/time_prep.py --out profiles/prep_timing.json
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
import prep_lib as P  # noqa: E402


def median(v):
    return sorted(v)[len(v) // 2]


def ring_arrays(n_images, n_points, rng, long_tracks=0):
    """(rot, trans, centres, xyz, obs_offset, obs_point) without Python loops over the points."""
    a = 2 * np.pi * np.arange(n_images) / n_images
    cen = np.column_stack([4 * np.cos(a), 4 * np.sin(a), 0.3 * np.sin(3 * a)])
    fwd = -cen / np.linalg.norm(cen, axis=1, keepdims=True)
    right = np.cross(fwd, [0, 0, 1.0])
    right /= np.linalg.norm(right, axis=1, keepdims=True)
    rot = np.stack([right, np.cross(fwd, right), fwd], 1)
    trans = -np.einsum("nij,nj->ni", rot, cen)
    centres = np.stack([-((rot[:, 0, k] * trans[:, 0] + rot[:, 1, k] * trans[:, 1]) + rot[:, 2, k] * trans[:, 2])
                        for k in range(3)], 1)
    xyz = rng.normal(scale=0.5, size=(n_points, 3))
    L = np.minimum(rng.poisson(8.0, n_points), n_images)
    L[:long_tracks] = n_images
    start = rng.integers(0, n_images, n_points)
    pt = np.repeat(np.arange(n_points), L)
    im = (np.repeat(start, L) + (np.arange(len(pt)) - np.repeat(np.cumsum(L) - L, L))) % n_images
    order = np.argsort(im, kind="stable")
    off = np.zeros(n_images + 1, np.int64)
    off[1:] = np.cumsum(np.bincount(im, minlength=n_images))
    return rot, trans, centres, xyz, off, pt[order].astype(np.int32)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--images", type=int, nargs="+", default=[100, 1000, 5000])
    ap.add_argument("--points_per_image", type=int, default=100)
    ap.add_argument("--long", type=int, nargs=3, default=[2000, 20000, 16], metavar=("IMAGES", "POINTS", "LONG"),
                    help="the long-track case: LONG of the POINTS are seen by all IMAGES")
    ap.add_argument("--dense", type=int, nargs=2, default=[40, 50000], metavar=("IMAGES", "POINTS"),
                    help="the few-images case: every pair of neighbours shares thousands of points")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--host_max", type=int, default=20_000_000)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    lib = A.load_library()
    gate = A.prep_cos_gate(1.0, lib)
    eng = A.PrepEngine(args.device, lib)
    cases = [(args.dense[0], args.dense[1], 0)] + [(n, n * args.points_per_image, 0) for n in args.images] + \
        [tuple(args.long)]
    out = {"tool": "tools/time_prep.py", "device_times": "hipEvent, median of %d after a warm-up" % args.repeat,
           "cases": []}
    for n_images, n_points, n_long in cases:
        rng = np.random.default_rng(n_images)
        rot, trans, cen, xyz, off, pts = ring_arrays(n_images, n_points, rng, n_long)
        case = {"images": n_images, "points": n_points, "long_tracks": n_long, "observations": int(len(pts))}
        runs = {"tracks_ms": [], "ranks_ms": [], "lds": {"records_ms": [], "pairs_ms": []},
                "global": {"records_ms": [], "pairs_ms": []}}
        results = {}
        for it in range(args.repeat + 1):
            eng.set_model(rot, trans, cen, xyz, off, pts)
            t = eng.timing()["tracks_ms"]
            for name, mode in (("lds", A.PREP_ATOMICS_LDS), ("global", A.PREP_ATOMICS_GLOBAL)):
                results[name] = eng.pair_counts(gate, mode)
                tm = eng.timing()
                if it:
                    runs[name]["records_ms"].append(tm["records_ms"])
                    runs[name]["pairs_ms"].append(tm["pairs_ms"])
            z, cnt = eng.depth_ranks([0.01, 0.99])
            if it:
                runs["tracks_ms"].append(t)
                runs["ranks_ms"].append(eng.timing()["ranks_ms"])
        rec = eng.n_records
        case["pair_records"] = int(rec)
        case["tracks_ms"] = median(runs["tracks_ms"])
        case["ranks_ms"] = median(runs["ranks_ms"])
        for name in ("lds", "global"):
            r = median(runs[name]["records_ms"])
            case[name] = {"records_ms": r, "records_ms_runs": runs[name]["records_ms"],
                          "pairs_ms": median(runs[name]["pairs_ms"]), "records_per_s": rec / (r * 1e-3) if r else None}
        case["same_result"] = bool(np.array_equal(results["lds"][0], results["global"][0]) and
                                   np.array_equal(results["lds"][1], results["global"][1]))
        case["hottest_pair"] = int(results["lds"][0].max())
        if rec <= args.host_max:
            obs = [pts[off[i]:off[i + 1]].astype(np.int64) for i in range(n_images)]
            t0 = time.perf_counter()
            s, nar, nrec = P.pair_counts_ref(cen, xyz, obs, gate)
            t1 = time.perf_counter()
            zr, cr = P.depth_ranks_ref(rot, trans, xyz, obs, [0.01, 0.99])
            t2 = time.perf_counter()
            case["host_numpy"] = {"pairs_ms": (t1 - t0) * 1e3, "ranks_ms": (t2 - t1) * 1e3,
                                  "matches_device": bool(np.array_equal(s, results["lds"][0]) and
                                                         np.array_equal(nar, results["lds"][1]) and nrec == rec and
                                                         P.same_bits64(zr, z) and np.array_equal(cr, cnt))}
        print(json.dumps(case), flush=True)
        out["cases"].append(case)
    eng.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
