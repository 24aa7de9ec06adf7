#!/usr/bin/env python3
"""Times the registration calls of include/apd_eval.h on the device.

Size 1 (default 10^6 source against 10^6 target points, a noisy height field in raster order and
shuffled): per evaluation the fused kernel and the fold (device events), per update the host solve,
for three correspondence radii; apd_eval_nearest, crop_volume and transform; and one evaluation by
the host twin on one core, with the check that it returns the device's bits.
Size 2 (default 10^7 against 10^7): the whole three-stage protocol through `apd_eval --tat_gt`.

usage: python tools/time_eval_register.py [n1 [n2]] [--out FILE.json]
"""
import json, os, shutil, subprocess, sys, tempfile, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "apde-mvs_amd")); sys.path.insert(0, os.path.join(REPO, "tests"))
import numpy as np
import apd_abi as A, register_lib as RL, synth

ARGS = sys.argv[1:]
OUT = None
if "--out" in ARGS:
    OUT = ARGS[ARGS.index("--out") + 1]
    del ARGS[ARGS.index("--out"):ARGS.index("--out") + 2]
N1 = int(float(ARGS[0])) if len(ARGS) > 0 else 10**6
N2 = int(float(ARGS[1])) if len(ARGS) > 1 else 10**7
res = {"tool": "tools/time_eval_register.py", "device_times": "hipEvent, one run after a warm-up evaluation",
       "host_times": "monotonic clock"}

def surface(n, seed, shuffle):
    """n points on a height field over [-5, 5]^2, raster order (as a fused cloud comes) or shuffled"""
    side = int(np.ceil(np.sqrt(n)))
    u = np.linspace(-5, 5, side)
    x, y = np.meshgrid(u, u)
    rng = np.random.default_rng(seed)
    z = np.sin(x) * np.cos(0.7 * y) + 0.3 * np.sin(3 * x + y)
    p = np.stack([x, y, z], -1).reshape(-1, 3)[:n] + rng.normal(0, 0.2 * 10 / side, (n, 3))
    if shuffle: p = p[rng.permutation(n)]
    return p.astype(np.float32), 10.0 / side

def dump():
    if OUT:
        with open(OUT, "w") as f: json.dump(res, f, indent=1)

lib = A.load_library(); eng = A.EvalEngine(0, lib)
D = RL.similarity(0.5, [1, 0.5, -0.25], 1.002, [0.01, -0.01, 0.01])
for order in ("raster", "shuffled"):
    tgt, spacing = surface(N1, 1, order == "shuffled")
    src = RL.transform_ref(surface(N1, 2, order == "shuffled")[0], np.linalg.inv(D))
    tau = 3 * spacing
    eng.set_target(tgt)
    row = {"n_source": N1, "n_target": N1, "spacing": spacing, "build_ms": eng.timing()["build_ms"]}
    for name, mc in (("max_corr_2tau", 2 * tau), ("max_corr_20tau", 20 * tau), ("max_corr_80tau", 80 * tau)):
        eng.register_sums(src, mc)  # warm-up
        T, info, st = eng.register(src, mc, None, True, 10, 0.0, 0.0)
        t = eng.register_timing()
        row[name] = {"max_corr": mc, "evaluations": t["evaluations"], "eval_ms_per_evaluation": t["eval_ms"] / t["evaluations"],
                     "fold_ms_per_evaluation": t["fold_ms"] / t["evaluations"], "solve_ms_per_update": t["solve_ms"] / max(info["iterations"], 1),
                     "info": info, "max_abs_T_minus_truth": float(np.abs(T - D).max())}
    eng.nearest(src, 2 * tau); row["nearest_sorted_queries_ms"] = eng.timing()["query_ms"]
    for _ in range(2):  # the first call also loads the scan's code
        eng.crop_volume(src, 2, -2.0, 2.0, np.array([[-4, -4], [4, -4], [4, 4], [0, 1], [-4, 4.0]]))
    row["crop_ms"] = eng.register_timing()["crop_ms"]
    eng.transform(src, D); row["transform_ms"] = eng.register_timing()["transform_ms"]
    if order == "raster":
        t0 = time.perf_counter(); hs = A.register_sums_host(tgt, src, 2 * tau, None, lib=lib); row["host_twin_one_evaluation_one_core_ms"] = (time.perf_counter() - t0) * 1e3
        ds = eng.register_sums(src, 2 * tau)
        row["host_twin_equals_device"] = bool(np.array_equal(hs.view(np.uint64), ds.view(np.uint64)))
    res["size1_" + order] = row; dump(); print(order, json.dumps(row), flush=True)
eng.close()

# size 2: the whole protocol through the tool
tmp = tempfile.mkdtemp(prefix="tat_timing_")
tgt, spacing = surface(N2, 3, False)
src = RL.transform_ref(surface(N2, 4, False)[0], np.linalg.inv(D))
tau = 3 * spacing
synth.write_ply(os.path.join(tmp, "gt.ply"), tgt); synth.write_ply(os.path.join(tmp, "rec.ply"), src)
RL.write_crop_json(os.path.join(tmp, "crop.json"), {"axis_max": 3.0, "axis_min": -3.0, "orthogonal_axis": "Z",
                   "bounding_polygon": [[-4.5, -4.5, 0], [4.5, -4.5, 0], [4.5, 4.5, 0], [0, 3.5, 0], [-4.5, 4.5, 0]]})
del tgt, src
t0 = time.perf_counter()
p = subprocess.run([os.path.join(REPO, "apde-mvs_amd", "host", "build", "apd_eval"), "--cloud", os.path.join(tmp, "rec.ply"), "--tat_gt",
                    os.path.join(tmp, "gt.ply"), "--tat_crop", os.path.join(tmp, "crop.json"), "--tau", repr(tau), "--json",
                    os.path.join(tmp, "o.json")], capture_output=True, text=True, timeout=500)
wall = time.perf_counter() - t0
print(p.stdout[-2000:], p.stderr[-2000:], flush=True)
if p.returncode == 0:
    r = json.load(open(os.path.join(tmp, "o.json")))["tat"]
    res["size2_protocol"] = {"n_source": N2, "n_target": N2, "tau": tau, "wall_s_with_ply_io": wall, "result": r}
else:
    res["size2_protocol"] = {"error": p.stderr[-500:], "returncode": p.returncode}
shutil.rmtree(tmp, ignore_errors=True)
dump(); print("done", flush=True)
