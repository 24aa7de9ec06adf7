#!/usr/bin/env python3
"""Time apd_prep_undistort_bgr8 (include/apd_prep.h, k_pr_undistort) on full-size images.

Sizes 6048x4032 and 3024x2016; models SIMPLE_RADIAL, OPENCV and THIN_PRISM_FISHEYE with moderate
coefficients; the output camera is the source's (same size, same fx fy cx cy), as `apd_prepare
--undistort` uses it. Per case, the median of --repeat calls after a warm-up call that grows the
context's buffers:

  upload / kernel / download   device events of a call with host pointers
  kernel_resident              the kernel's events of a call with device-resident source and destination
  host_ms                      apd_prep_undistort_bgr8_host (one thread; the host version is not threaded)

and whether the device image equals the host image byte for byte. Every case runs in a process of its
own, which is ended after 60 s; after a case that fails nothing more is started.

  python tools/time_undistort.py --out profiles/undistort_timing.json
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "apde-mvs_amd"))
import apd_abi as A  # noqa: E402

CASE_TIMEOUT_S = 60
SIZES = [(6048, 4032), (3024, 2016)]
# coefficients after the intrinsics
MODELS = {"SIMPLE_RADIAL": [-0.12], "OPENCV": [-0.15, 0.05, 0.004, -0.003],
          "THIN_PRISM_FISHEYE": [0.05, -0.02, 0.004, -0.003, 0.004, -0.001, 0.002, -0.002]}


def median(v):
    return sorted(v)[len(v) // 2]


def run_case(w, h, model, repeat, device):
    import torch
    lib = A.load_library()
    f = 0.8 * w
    head = [f, 0.5 * w + 3.25, 0.5 * h - 2.5] if A.PREP_CAMERA_MODELS[model][1] in (4, 5) else \
        [f, 1.01 * f, 0.5 * w + 3.25, 0.5 * h - 2.5]
    params = np.array(head + MODELS[model])
    K = np.array(A.prep_pinhole_K(model, params))
    src = np.random.default_rng(w).integers(0, 256, (h, w, 3)).astype(np.uint8)
    dst = np.empty_like(src)
    d_src = torch.from_numpy(src).to("cuda:%d" % device)
    d_dst = torch.empty_like(d_src)
    torch.cuda.synchronize()
    eng = A.PrepEngine(device, lib)
    mid = A.prep_model_id(model)
    runs = {"upload_ms": [], "kernel_ms": [], "download_ms": [], "kernel_resident_ms": []}
    for it in range(repeat + 1):
        for s, d, resident in ((src.ctypes.data, dst.ctypes.data, False), (d_src.data_ptr(), d_dst.data_ptr(), True)):
            st = lib.apd_prep_undistort_bgr8(eng.ctx, mid, params.ctypes.data, len(params), w, h, s, K.ctypes.data, w, h, d)
            if st != 0:
                raise SystemExit("apd_prep_undistort_bgr8 -> %d" % st)
            t = eng.undistort_timing()
            if it and resident:
                runs["kernel_resident_ms"].append(t["kernel_ms"])
            elif it:
                for k in ("upload_ms", "kernel_ms", "download_ms"):
                    runs[k].append(t[k])
    eng.close()
    host = np.empty_like(src)
    host_runs = []
    for it in range(2):
        t0 = time.perf_counter()
        st = lib.apd_prep_undistort_bgr8_host(mid, params.ctypes.data, len(params), w, h, src.ctypes.data, K.ctypes.data, w, h,
                                              host.ctypes.data)
        host_runs.append((time.perf_counter() - t0) * 1e3)
        if st != 0:
            raise SystemExit("apd_prep_undistort_bgr8_host -> %d" % st)
    case = {"width": w, "height": h, "model": model, "params": params.tolist()}
    for k, v in runs.items():
        case[k] = median(v)
        case[k + "_runs"] = v
    case["host_one_thread_ms"] = min(host_runs)
    case["host_threads_16_ms"] = None  # the host version is not threaded
    case["kernel_pixels_per_s"] = w * h / (case["kernel_ms"] * 1e-3) if case["kernel_ms"] else None
    case["device_equals_host"] = bool(np.array_equal(dst, host) and np.array_equal(d_dst.cpu().numpy(), host))
    case["black_share"] = float((host.reshape(-1, 3).max(1) == 0).mean())
    return case


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default="")
    ap.add_argument("--case", nargs=3, metavar=("W", "H", "MODEL"), help="run one case in this process (internal)")
    args = ap.parse_args()
    if args.case:
        print(json.dumps(run_case(int(args.case[0]), int(args.case[1]), args.case[2], args.repeat, args.device)), flush=True)
        return 0
    out = {"tool": "tools/time_undistort.py",
           "device_times": "hipEvent, median of %d after a warm-up; one process per case, ended after %d s" %
                           (args.repeat, CASE_TIMEOUT_S), "cases": []}
    status = 0
    for w, h in SIZES:
        for model in MODELS:
            cmd = [sys.executable, os.path.abspath(__file__), "--case", str(w), str(h), model, "--repeat", str(args.repeat),
                   "--device", str(args.device)]
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=CASE_TIMEOUT_S)
            except subprocess.TimeoutExpired:
                print("%dx%d %s: no result after %d s; stopping" % (w, h, model, CASE_TIMEOUT_S), file=sys.stderr)
                status = 1
                break
            if r.returncode != 0:
                print("%dx%d %s: exit %d; stopping\n%s" % (w, h, model, r.returncode, r.stderr[-2000:]), file=sys.stderr)
                status = 1
                break
            case = json.loads(r.stdout.strip().splitlines()[-1])
            print(json.dumps(case), flush=True)
            out["cases"].append(case)
        if status:
            break
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")
    return status


if __name__ == "__main__":
    sys.exit(main())
