"""How many anchors and image lines the 64 lanes of a Weak-sweep workgroup share, by list order: runs
the bench's headline pass (final-round REFINE_ITER + APD + geom) on a small rendering of the same
scene through the oracle, takes the pass's anchors, and groups the WEAK pixels 64 at a time in
  (a) the per-colour tile order (one colour of about 16x8 per group),
  (b) the dense two-colour tile order, 4x4 micro-tiles row-major in the 16x16 tile (about 16x4),
  (c) the dense order with the micro-tiles in 2x2 blocks (about 8x8).
Per group and anchor slot k = 1..8 it counts the distinct anchor positions among the lanes and the
distinct 128-byte lines of a row-major 8-byte-per-pixel image that the slot's 3x3 step-5 windows touch
(in the reference image, as a proxy for the source views). The WEAK pixels are the input's (the sweep
lists drop the few that NeighbourUpdate demotes). CPU only.
Usage: python tools/weak_group_sharing.py [W H N]"""
import os, sys
from types import SimpleNamespace
import numpy as np
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "apde-mvs_amd"), os.path.join(REPO, "tests")]
import bench
import apd_abi as A
import oracle_lib

W, H, N = (int(x) for x in sys.argv[1:4]) if len(sys.argv) > 3 else (378, 252, 10)
TW = TH = 16      # list tile (apd_kernels.hip TILE_POS / tile_w)
SUPER = 128 // TW  # tiles per super-tile side (TILE_SUPER_PX)
lib = oracle_lib.load()
# TEXTURE_SCALE=16 renders the headline's texture per pixel (6048 / 378), so that the WEAK fraction is
# the headline's 0.94 instead of the small rendering's 0.18 (bench.py cpu_baseline samples the same way)
TS = float(os.environ.get("TEXTURE_SCALE", "1"))
sc = bench.make_scene(W, H, N, 1, os.environ.get("AB_TEXTURE", "smooth"), texture_scale=TS)
ids = [0] + [j for j, _ in sc.pairs[0]][:N]
priors = {}
for r in ids:
    out = oracle_lib.run(lib, A.scene_problem(sc, r, [j for j, _ in sc.pairs[r]][:N], seed=0x5EED ^ r))
    priors[r] = SimpleNamespace(planes=out.planes, weak_info=out.weak_info, confidence=out.confidence)
arr = bench.final_round_problem(sc, priors, 0, N)
out = oracle_lib.run(lib, arr)
nw = int(out.weak_count[0])
wpix = np.flatnonzero(arr.weak_info.reshape(-1) == A.WEAK)[:nw]  # anchors are indexed by the raster rank of the WEAK pixel
anc = out.anchors[:nw].astype(np.int64)
ok = (anc[..., 0] >= 0) & (anc[..., 1] >= 0)
y, x = wpix // W, wpix % W


def tile_key(quad):
    """Position of every WEAK pixel in the tile order (tile_coords + tile_pixel)."""
    tiles_x, tiles_y = -(-W // TW), -(-H // TH)
    tx, ty, lx, ly = x // TW, y // TH, x % TW, y % TH
    sy, sx = ty // SUPER, tx // SUPER
    rows = np.minimum(SUPER, tiles_y - SUPER * sy)
    cols = np.minimum(SUPER, tiles_x - SUPER * sx)
    tile = sy * SUPER * tiles_x + sx * rows * SUPER + (ty - SUPER * sy) * cols + (tx - SUPER * sx)
    mcol, mrow, mx = lx // 4, ly // 4, TW // 4
    micro = ((mrow // 2) * (mx // 2) + mcol // 2) * 4 + (mrow % 2) * 2 + mcol % 2 if quad else mrow * mx + mcol
    return (tile * 16 + micro) * 16 + (ly % 4) * 4 + lx % 4


def groups(order_name):
    """Lists of WEAK indices, 64 per sweep workgroup."""
    if order_name == "a":
        key = tile_key(False)
        gs = []
        for colour in (0, 1):
            sel = np.flatnonzero(((x + y) & 1) == colour)
            sel = sel[np.argsort(key[sel], kind="stable")]
            gs += [sel[i:i + 64] for i in range(0, sel.size, 64)]
        return gs
    sel = np.argsort(tile_key(order_name == "c"), kind="stable")
    return [sel[i:i + 64] for i in range(0, sel.size, 64)]


def lines_of(ax, ay):
    """Distinct 128-B lines (8 B per pixel, row-major) under the 3x3 step-5 windows at the anchors."""
    tx = np.clip(ax[:, None] + np.array([-5, 0, 5])[None, :], 0, W - 1)
    ty = np.clip(ay[:, None] + np.array([-5, 0, 5])[None, :], 0, H - 1)
    px = (ty[:, :, None] * W + tx[:, None, :]).reshape(-1)
    return np.unique(px * 8 // 128).size


print(f"{W}x{H} N={N} texture_scale {TS:g}: {nw} WEAK px ({nw / (W * H):.2f} of the image), {ok[:, 1:].sum(1).mean():.2f} anchors per px")
res = {}
for name, what in (("a", "per-colour, 16x8 of one colour"), ("b", "dense, 16x4"), ("c", "dense, 8x8")):
    gs = [g for g in groups(name) if g.size == 64]  # (full groups: the last of each list is partial)
    ext = np.array([[np.ptp(x[g]) + 1, np.ptp(y[g]) + 1] for g in gs])
    da = np.zeros((len(gs), 8))
    dl = np.zeros((len(gs), 8))
    for i, g in enumerate(gs):
        for k in range(1, 9):
            m = ok[g, k]
            q = anc[g, k][m]
            da[i, k - 1] = np.unique(q[:, 1] * W + q[:, 0]).size
            dl[i, k - 1] = lines_of(q[:, 0], q[:, 1]) if q.size else 0
    res[name] = (da.mean(), dl.mean())
    print(f"({name}) {what}: {len(gs)} full groups, median extent {np.median(ext[:, 0]):.0f}x{np.median(ext[:, 1]):.0f}")
    print("    distinct anchors per slot k=1..8: " + " ".join(f"{v:5.1f}" for v in da.mean(0)) + f" | mean {da.mean():5.2f}")
    print("    distinct 128-B lines per slot:    " + " ".join(f"{v:5.1f}" for v in dl.mean(0)) + f" | mean {dl.mean():5.2f}")
for name in ("b", "c"):
    print(f"({name}) against (a): distinct anchors {res[name][0] / res['a'][0]:.3f}x, lines {res[name][1] / res['a'][1]:.3f}x")
