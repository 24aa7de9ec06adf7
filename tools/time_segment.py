#!/usr/bin/env python3
"""Time apd_seg_flat_zones_bgr8 and apd_seg_label_mask (include/apd_seg.h, csrc/apd_seg.hip) at full size.

Source size 6048x4032, at max_size 2560 (working size 2016x1344, s = 3) and at max_size 0 (s = 1). Inputs:

  patches   constant patches of 96 source pixels plus noise of +-2 levels: what the tool is for
  flat      one constant image: a single component of the whole working image, the worst case for the
            area atomics
  mask059   apd_seg_label_mask on a random mask of density 0.59 at the working size (near the percolation
            threshold of 4-connectivity): the worst case for the tile merge. A mask, not an image: no image
            gives independent flat pixels after the smoothing

Per case, the median of --repeat calls after a warm-up call that grows the context's buffers:

  <stage>_ms            device events of a call with host pointers (APD_SEG_T_* of include/apd_seg.h)
  resident_total_ms     the stages' sum, without upload and download, of a call with device-resident input and output
  host_one_thread_ms    the host twin (one thread; it is not threaded)

and whether device and host agree byte for byte. Every case runs in a process of its own, which is ended
after 180 s; after a case that fails nothing more is started.

  python tools/time_segment.py --out profiles/segment_timing.json
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

CASE_TIMEOUT_S = 180
SIZE = (6048, 4032)
MAX_SIZES = [2560, 0]
KINDS = ["patches", "flat", "mask059"]
STAGES = [k for k in A.SEG_TIMES if k not in ("upload_ms", "download_ms")]


def median(v):
    return sorted(v)[len(v) // 2]


def make_image(kind, w, h):
    if kind == "flat":
        return np.full((h, w, 3), 128, np.uint8)
    rng = np.random.default_rng(w)
    patch = 96
    base = rng.integers(20, 236, (-(-h // patch), -(-w // patch), 3), dtype=np.int16)
    img = np.repeat(np.repeat(base, patch, 0), patch, 1)[:h, :w]
    img = img + rng.integers(-2, 3, (h, w, 3), dtype=np.int16)
    return np.clip(img, 0, 255).astype(np.uint8)


def run_case(kind, max_size, repeat, device):
    import torch
    lib = A.load_library()
    w, h = SIZE
    s, W, H = A.seg_working_size(w, h, max_size, lib)
    eng = A.SegEngine(device, lib)
    dev = "cuda:%d" % device
    runs = {k: [] for k in A.SEG_TIMES}
    resident = []
    case = {"kind": kind, "width": w, "height": h, "max_size": max_size, "s": s, "working_width": W, "working_height": H}
    if kind == "mask059":
        mask = (np.random.default_rng(59).random((H, W)) < 0.59).astype(np.uint8)
        d_mask = torch.from_numpy(mask).to(dev)
        torch.cuda.synchronize()
        for it in range(repeat + 1):
            got = eng.label_mask(mask)
            t = eng.timing()
            d_got = eng.label_mask(d_mask)
            tr = eng.timing()
            if it:
                for k in A.SEG_TIMES:
                    runs[k].append(t[k])
                resident.append(sum(tr[k] for k in STAGES))
        t0 = time.perf_counter()
        want = A.seg_label_mask_host(mask, lib)
        case["host_one_thread_ms"] = (time.perf_counter() - t0) * 1e3
        case["device_equals_host"] = bool(np.array_equal(got, want) and np.array_equal(d_got.cpu().numpy(), want))
        sizes = np.bincount(want[want >= 0])
        case["components"] = int((sizes > 0).sum())
        case["largest_component"] = int(sizes.max())
    else:
        img = make_image(kind, w, h)
        d_img = torch.from_numpy(img).to(dev)
        torch.cuda.synchronize()
        for it in range(repeat + 1):
            got = eng.flat_zones(img, max_size)
            t = eng.timing()
            d_got = eng.flat_zones(d_img, max_size)
            tr = eng.timing()
            if it:
                for k in A.SEG_TIMES:
                    runs[k].append(t[k])
                resident.append(sum(tr[k] for k in STAGES))
        t0 = time.perf_counter()
        want = A.seg_flat_zones_host(img, max_size, lib=lib)
        case["host_one_thread_ms"] = (time.perf_counter() - t0) * 1e3
        case["device_equals_host"] = bool(np.array_equal(got[0], want[0]) and got[1:] == want[1:] and
                                          np.array_equal(d_got[0].cpu().numpy(), want[0]) and d_got[1:] == want[1:])
        case["survivors"], case["labels"] = want[1], want[2]
        case["labelled_share"] = float((want[0] > 0).mean())
    eng.close()
    for k, v in runs.items():
        case[k] = median(v)
        case[k + "_runs"] = v
    case["stages_total_ms"] = sum(case[k] for k in STAGES)
    case["resident_total_ms"] = median(resident)
    case["resident_total_ms_runs"] = resident
    case["host_over_resident"] = case["host_one_thread_ms"] / case["resident_total_ms"] if case["resident_total_ms"] else None
    return case


def parent_commit():
    try:
        return subprocess.run(["git", "-C", REPO, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or None
    except OSError:
        return None


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default="")
    ap.add_argument("--parent", default="", help="the commit the measured tree stands on (default: git's HEAD, if any)")
    ap.add_argument("--case", nargs=2, metavar=("KIND", "MAX_SIZE"), help="run one case in this process (internal)")
    args = ap.parse_args()
    if args.case:
        print(json.dumps(run_case(args.case[0], int(args.case[1]), args.repeat, args.device)), flush=True)
        return 0
    out = {"tool": "tools/time_segment.py", "parent_commit": args.parent or parent_commit(),
           "device_times": "hipEvent, median of %d after a warm-up; one process per case, ended after %d s" %
                           (args.repeat, CASE_TIMEOUT_S), "cases": []}
    status = 0
    for max_size in MAX_SIZES:
        for kind in KINDS:
            cmd = [sys.executable, os.path.abspath(__file__), "--case", kind, str(max_size), "--repeat", str(args.repeat),
                   "--device", str(args.device)]
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=CASE_TIMEOUT_S)
            except subprocess.TimeoutExpired:
                print("%s max_size %d: no result after %d s; stopping" % (kind, max_size, CASE_TIMEOUT_S), file=sys.stderr)
                status = 1
                break
            if r.returncode != 0:
                print("%s max_size %d: exit %d; stopping\n%s" % (kind, max_size, r.returncode, r.stderr[-2000:]), file=sys.stderr)
                status = 1
                break
            case = json.loads(r.stdout.strip().splitlines()[-1])
            print(json.dumps({k: v for k, v in case.items() if not k.endswith("_runs")}), flush=True)
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
