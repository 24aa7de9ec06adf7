#!/usr/bin/env python3
"""Times the DTU calls of include/apd_eval.h on the device.

radius_thin at n1 (default 10^6) and n2 (default 10^7) points of a noisy height field in raster order
with seeded ranks: sort time, rounds time and number of rounds (device events, one run after a
warm-up), points per occupied cell, and at n1 the host twin on one core with the check that it returns
the device's indices. The same at n1 with rank = NULL: the cost of a raster-order chain, the reason the
tool draws ranks. obs_mask, half_space and masked_stats at n2. The whole `apd_eval --dtu_gt` at n2
against n2 with file reading. With --bench JSON the headline of a `python bench.py` run (the JSON line
it printed, saved to a file) is recorded next to --bench_parent VALUE, the parent commit's figure.

usage: python tools/time_eval_dtu.py [n1 [n2]] [--out FILE.json] [--bench FILE --bench_parent VALUE] [--no_tool]
"""
import json, os, shutil, subprocess, sys, tempfile, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "apde-mvs_amd")); sys.path.insert(0, os.path.join(REPO, "tests"))
import numpy as np
import apd_abi as A, dtu_lib as DL, synth

ARGS = sys.argv[1:]
def opt(name, flag=False):
    if name not in ARGS: return None
    i = ARGS.index(name)
    v = True if flag else ARGS[i + 1]
    del ARGS[i:i + (1 if flag else 2)]
    return v
OUT, BENCH, BENCH_PARENT, NO_TOOL = opt("--out"), opt("--bench"), opt("--bench_parent"), opt("--no_tool", True)
N1 = int(float(ARGS[0])) if len(ARGS) > 0 else 10**6
N2 = int(float(ARGS[1])) if len(ARGS) > 1 else 10**7
RADIUS = 0.2
res = {"tool": "tools/time_eval_dtu.py", "device_times": "hipEvent, one run after a warm-up call",
       "host_times": "monotonic clock", "radius": RADIUS}

def surface(n, seed):
    """n points of a noisy height field in raster order at spacing 0.1 (millimetres: a quarter of them
    survives a thinning at 0.2), as a fused cloud comes"""
    side = int(np.ceil(np.sqrt(n)))
    u = np.arange(side) * 0.1
    x, y = np.meshgrid(u, u)
    rng = np.random.default_rng(seed)
    z = 3.0 * np.sin(x / 9.0) * np.cos(y / 7.0) + 0.05 * x
    p = np.stack([x, y, z], -1).reshape(-1, 3)[:n] + rng.normal(0, 0.03, (n, 3))
    return p.astype(np.float32), side * 0.1

def dump():
    if OUT:
        with open(OUT, "w") as f: json.dump(res, f, indent=1)

lib = A.load_library(); eng = A.EvalEngine(0, lib)
eng.radius_thin(surface(10**5, 9)[0], RADIUS, A.dtu_ranks(10**5, 0, lib))  # warm-up: loads the code objects

def thin_row(n, rank, host):
    pts, extent = surface(n, 1)
    c = np.floor(pts.astype(np.float64) / (2.0 * float(np.float32(RADIUS)))).astype(np.int64)
    c -= c.min(axis=0)
    cells = np.unique(c[:, 0] << 42 | c[:, 1] << 21 | c[:, 2])
    t0 = time.perf_counter(); keep = eng.radius_thin(pts, RADIUS, rank); wall = time.perf_counter() - t0
    t = eng.thin_timing()
    row = {"n": n, "extent": extent, "kept": int(len(keep)), "sort_ms": t["sort_ms"], "rounds_ms": t["rounds_ms"],
           "rounds": t["rounds"], "wall_ms_with_upload": wall * 1e3, "occupied_cells": int(len(cells)),
           "points_per_occupied_cell": n / len(cells)}
    if host:
        t0 = time.perf_counter(); hk = A.radius_thin_host(pts, RADIUS, rank, lib)
        row["host_twin_one_core_ms"] = (time.perf_counter() - t0) * 1e3
        row["host_twin_equals_device"] = bool(np.array_equal(hk, keep))
    return row

for name, n, ranked, host in (("thin_n1_ranks", N1, True, True), ("thin_n1_rank_null", N1, False, False),
                              ("thin_n2_ranks", N2, True, False)):
    res[name] = thin_row(n, A.dtu_ranks(n, 0, lib) if ranked else None, host)
    dump(); print(name, json.dumps(res[name]), flush=True)

# the three small kernels at n2
pts, extent = surface(N2, 2)
rng = np.random.default_rng(3)
mres = 0.5
dims = (int(extent / mres) + 2, int(extent / mres) + 2, 64)
mask = rng.uniform(size=dims) < 0.7
origin = [0.0, 0.0, -16.0]
dist = rng.uniform(0, 25, N2).astype(np.float32)
small = {"n": N2, "mask_dims": list(dims)}
for rep in range(2):  # the first call uploads the mask and loads the code
    inside = eng.obs_mask(pts, mask, origin, mres)
    above = eng.half_space(pts, [0.0, 0.0, 1.0, -0.5])
    st = eng.masked_stats(dist, inside, float(np.nextafter(np.float32(20), np.float32(0))))
    small.update(eng.dtu_timing())
small["selected"] = st["count"]
res["small_kernels_n2"] = small; dump(); print("small", json.dumps(small), flush=True)
eng.close()

if not NO_TOOL:  # the whole protocol through the tool, file reading included
    tmp = tempfile.mkdtemp(prefix="dtu_timing_")
    gt, extent = surface(N2, 4)
    synth.write_ply(os.path.join(tmp, "gt.ply"), gt); synth.write_ply(os.path.join(tmp, "rec.ply"), pts)
    DL.save_mat(os.path.join(tmp, "ObsMask.mat"), {"ObsMask": mask, "BB": np.array([origin, [extent, extent, 16.0]]),
                                                   "Res": mres}, compress=True)
    DL.save_mat(os.path.join(tmp, "Plane.mat"), {"P": np.array([0.0, 0.0, 1.0, 8.0]).reshape(4, 1)})
    del gt, pts
    t0 = time.perf_counter()
    p = subprocess.run([os.path.join(REPO, "apde-mvs_amd", "host", "build", "apd_eval"), "--cloud", os.path.join(tmp, "rec.ply"),
                        "--dtu_gt", os.path.join(tmp, "gt.ply"), "--dtu_mask", os.path.join(tmp, "ObsMask.mat"), "--dtu_plane",
                        os.path.join(tmp, "Plane.mat"), "--json", os.path.join(tmp, "o.json")], capture_output=True, text=True,
                       timeout=500)
    wall = time.perf_counter() - t0
    print(p.stdout[-2000:], p.stderr[-2000:], flush=True)
    if p.returncode == 0:
        r = json.load(open(os.path.join(tmp, "o.json")))["dtu"]
        r.pop("definition", None)
        res["tool_n2"] = {"n_cloud": N2, "n_gt": N2, "wall_s_with_file_io": wall, "result": r}
    else:
        res["tool_n2"] = {"error": p.stderr[-500:], "returncode": p.returncode}
    shutil.rmtree(tmp, ignore_errors=True)

if BENCH:  # no depth-engine source changed: the benchmark's headline next to the parent commit's
    line = [l for l in open(BENCH).read().splitlines() if l.startswith("{")][-1]
    res["bench"] = {"this_tree": json.loads(line), "parent_commit_headline": BENCH_PARENT}
dump(); print("done", flush=True)
