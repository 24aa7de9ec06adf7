"""Helpers of the Strong-half known-answer tests (tests/test_oracle_kat_strong.py) and of their runs on
the HIP engine (tests/test_gpu_staged_parity.py). Test infrastructure only.

Everything here is either the construction of hand-built problems or a restatement of a reference
rule in numpy float64 / plain integers, written from the APD.cu lines cited per function. Nothing
here calls the oracle or the kernels.

The "exact seed" construction: reference and source cameras share K (f = 64, principal point at the
image centre) and R = I; a source translated along x by b sees a point at depth d shifted by
f * b / d pixels. With b = 0.5 and the source image the reference texture shifted by 4 px, the
fronto-parallel plane at d0 = 8 has disparity exactly 4: every bilinear tap lands on a texel, the two
NCC windows hold the same integers, var_ref = var_src = covar and the cost is exactly 0 wherever the
centre projects into the source (x >= 4). Clamp-to-edge addressing keeps the windows equal at the
borders: a clamp in y acts on both windows alike, and the texture is constant along x over columns
0..4 and from column W - 1 on, so a tap clamped in x reads the value its partner reads.
"""
import ctypes as C
from dataclasses import dataclass

import numpy as np

import apd_abi as A
import synth

W, H = 64, 48
F = 64.0
B = 0.5
D0 = 8.0
SHIFT = 4
DMIN, DMAX = 0.5, 20.0
TEX_SEED = 8
NEAR_DISP, FAR_DISP = 4.5, 7.0  # the near-miss and far-miss fronto-parallel fields
# exact-plane pixels of the footprint problems: centre, (2, 2), (W - 3, H - 4), both colours, every border
SEEDS = [(32, 24), (2, 2), (W - 3, H - 4), (33, 2), (20, H - 2), (W - 2, 3), (40, 0), (41, H - 2), (5, 30),
         (W - 1, 20)]
X_LO = SHIFT  # columns x >= X_LO see the exact plane at cost exactly 0; left of it the centre leaves the source


def ptr(a):
    return None if a is None else a.ctypes.data


def fptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _smooth(rng, h, w, passes=4):
    t = rng.normal(size=(h, w + 16))
    k = np.array([1.0, 2.0, 1.0]) / 4.0
    for _ in range(passes):
        t = np.apply_along_axis(lambda r: np.convolve(r, k, mode="same"), 1, t)
        t = np.apply_along_axis(lambda r: np.convolve(r, k, mode="same"), 0, t)
    return t[:, 8:8 + w]


def wide_texture(seed=TEX_SEED, w=W, h=H, margin=16):
    """Integer-valued band-limited texture, `margin` columns wider than the image on the right,
    constant along x over columns 0..SHIFT and from column w - 1 on."""
    rng = np.random.default_rng(seed)
    t = _smooth(rng, h, w + margin)
    t = (t - t.min()) / (t.max() - t.min())
    t = np.rint(t * 255.0).astype(np.float32)
    t[:, :SHIFT + 1] = t[:, SHIFT:SHIFT + 1]
    t[:, w - 1:] = t[:, w - 1:w]
    return t


def images(seed=TEX_SEED, shift=SHIFT):
    """(reference image, source image) with source(x) = reference(x + shift)."""
    t = wide_texture(seed)
    return np.ascontiguousarray(t[:, :W]), np.ascontiguousarray(t[:, shift:shift + W])


def graded_source(seed=TEX_SEED, noise_seed=1032, lo_deg=50.0, hi_deg=100.0):
    """A source whose correlation with the shifted reference falls from cos(lo) to cos(hi) across the
    columns: the exact plane's cost then spans both sides of the view-selection thresholds (about 60 %
    of the pixels under 0.8, 25 % between 0.8 and 1.2, 15 % above; the noise seed is one that puts the
    four pixels (61..62, 0) and (61..62, H - 1) between the two)."""
    t = wide_texture(seed)
    s = t[:, SHIFT:SHIFT + W].astype(np.float64)
    u = wide_texture(noise_seed)[:, :W].astype(np.float64)
    s0 = (s - s.mean()) / s.std()
    u0 = (u - u.mean()) / u.std()
    th = np.deg2rad(np.linspace(lo_deg, hi_deg, W))[None, :]
    g = np.cos(th) * s0 + np.sin(th) * u0
    g = (g - g.min()) / (g.max() - g.min())
    return np.rint(g * 255.0).astype(np.float32)


@dataclass(frozen=True)
class Rig:
    """A rig that is the exact-seed rig to every restatement here, and a general one to the code
    under test: the world moved rigidly (X' = Rg X + cg, so every camera has R' = R Rg^T and
    t' = t - R' cg), fy != fx in all views, and the sources' principal point moved by `m` whole
    pixels in x (Ks != Kr). A source at baseline b then sees depth d at x - (F b / d - m): with the
    baseline baseline(e, rig) the plane at D0 keeps the effective disparity e, the images stay those
    of images(), and every float64 answer in terms of effective disparities is the identity rig's."""
    Rg: tuple
    cg: tuple
    fy: float
    m: int


def _rodrigues(axis, deg):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = np.deg2rad(deg)
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)


# 25 degrees about (1, 2, 3): no zero entry, not symmetric
MOVED = Rig(tuple(map(tuple, _rodrigues((1.0, 2.0, 3.0), 25.0))), (0.3, -1.1, 2.0), 80.0, 2)


def baseline(eff_disparity=SHIFT, rig=None):
    """The baseline at which the plane at D0 has the given effective disparity."""
    return D0 * (eff_disparity + (rig.m if rig else 0)) / F


def depth_of(eff_disparity, rig=None):
    """Depth of the fronto-parallel plane with the given effective disparity under baseline(SHIFT, rig)."""
    m = rig.m if rig else 0
    return F * baseline(SHIFT, rig) / (np.asarray(eff_disparity, np.float64) + m)


def camera(b=0.0, rig=None, source=False):
    fy = rig.fy if rig else F
    m = rig.m if rig and source else 0
    K = np.array([[F, 0, W / 2.0 + m], [0, fy, H / 2.0], [0, 0, 1.0]])
    R, t = np.eye(3), np.array([-b, 0.0, 0.0])
    if rig:
        R = R @ np.asarray(rig.Rg).T
        t = t - R @ np.asarray(rig.cg)
    return synth.Camera(K, R, t, DMIN, DMAX)


def problem(srcs, baselines=None, rig=None, **params):
    """ProblemArrays with the reference image of images() and the given source images; baselines
    default to baseline(SHIFT, rig) (B on the identity rig) for every source."""
    ref, _ = images()
    baselines = baselines or [baseline(SHIFT, rig)] * len(srcs)
    cams = [camera(0.0, rig)] + [camera(b, rig, source=True) for b in baselines]
    vals = [synth.camera_struct_values(c, W, H) for c in cams]
    p = A.default_params(1 + len(srcs), DMIN, DMAX)
    for k, v in params.items():
        setattr(p, k, v)
    return A.ProblemArrays(W, H, [ref] + list(srcs), vals, p)


def plane_field(disparity, rig=None):
    """H x W x 4 fronto-parallel planes at the given (effective) disparity (scalar or H x W): normal
    (0, 0, -1); w is the distance to the origin in the sweep's form (= the depth, APD.cu:218-223) and,
    on the identity rig, the depth in the input form (world normal, depth) alike."""
    d = np.broadcast_to(np.asarray(depth_of(disparity, rig), np.float32), (H, W))
    pl = np.zeros((H, W, 4), np.float32)
    pl[..., 2] = -1.0
    pl[..., 3] = d
    return pl


def input_plane_field(disparity, rig=None):
    """The same field in the input form: (world normal, depth), world normal = Rg n_ref."""
    pl = plane_field(disparity, rig)
    if rig:
        pl[..., :3] = (np.asarray(rig.Rg) @ np.array([0.0, 0.0, -1.0])).astype(np.float32)
    return pl


# ------------------------------------------------------------------------------------------------
# ComputeBilateralNCCOld for fronto-parallel planes of this camera pair, APD.cu:596-663
# ------------------------------------------------------------------------------------------------
def ncc_shift(ref, src, disparity, dtype=np.float64):
    """Cost of every pixel for the plane whose homography is x' = x - disparity, y' = y (sa label 0):
    2 where the centre leaves the source (APD.cu:613-616); 36 taps at -5..5 step 2 with weight 1, the
    reference tap a clamped texel, the source tap bilinear with clamp-to-edge (APD.cu:629-643);
    variances and covariance of the means, 2 under the 1e-5 variance floor, else
    max(0, min(2, 1 - covar / sqrt(var_ref var_src))) (APD.cu:644-662)."""
    ref = ref.astype(dtype)
    src = src.astype(dtype)
    ys, xs = np.mgrid[0:H, 0:W]
    sr = np.zeros((H, W), dtype)
    srr, ss, sss, srs = sr.copy(), sr.copy(), sr.copy(), sr.copy()
    disparity = dtype(disparity)
    for i in range(-5, 6, 2):
        for j in range(-5, 6, 2):
            ry = np.clip(ys + j, 0, H - 1)
            r = ref[ry, np.clip(xs + i, 0, W - 1)]
            sx = (xs + i).astype(dtype) - disparity
            x0 = np.floor(sx)
            a = (sx - x0).astype(dtype)
            x0 = x0.astype(int)
            v0 = src[ry, np.clip(x0, 0, W - 1)]
            v1 = src[ry, np.clip(x0 + 1, 0, W - 1)]
            v = v0 + a * (v1 - v0)
            sr += r
            srr += r * r
            ss += v
            sss += v * v
            srs += r * v
    n = dtype(36.0)
    sr, srr, ss, sss, srs = sr / n, srr / n, ss / n, sss / n, srs / n
    var_r = srr - sr * sr
    var_s = sss - ss * ss
    cov = srs - sr * ss
    with np.errstate(invalid="ignore", divide="ignore"):
        c = np.clip(1.0 - cov / np.sqrt(var_r * var_s), 0.0, 2.0)
    c = np.where((var_r < 1e-5) | (var_s < 1e-5), 2.0, c)
    cx = xs.astype(dtype) - disparity
    return np.where((cx < 0) | (cx >= W), 2.0, c)


def ncc_tolerance(disparity):
    """Tolerance for a float32 NCC against the float64 restatement: four times the largest difference
    between the float32 and the float64 evaluation of the restatement itself over the image (about
    4e-5 for the near-miss field)."""
    ref, src = images()
    d = np.abs(ncc_shift(ref, src, disparity, np.float32).astype(np.float64) - ncc_shift(ref, src, disparity))
    return 4.0 * float(d.max())


# ------------------------------------------------------------------------------------------------
# CheckerboardPropagationStrong's eight regions, APD.cu:1127-1316
# ------------------------------------------------------------------------------------------------
def regions(x, y, w=W, h=H, far_first=3, far_samples=11, near_levels=3):
    """The eight regions of pixel (x, y) in the order of the reference's cost_array rows (0 up_near,
    1 up_far, 2 down_near, 3 down_far, 4 left_near, 5 left_far, 6 right_near, 7 right_far): None for a
    region whose first position is outside the image, else its (x, y) positions in scan order.
    Far lines: the first position at distance 3, then every second pixel, 11 in all, each kept while
    inside (APD.cu:1137-1210). Near V-shapes: the 4-neighbour, then for i = 0, 1, 2 the two pixels
    i + 1 further out and i + 1 to either side, each under its own bounds (APD.cu:1213-1314)."""
    ff, fs, nl = far_first, far_samples, near_levels
    out = [None] * 8
    if y > ff - 1:
        out[1] = [(x, y - ff)] + [(x, y - ff - 2 * i) for i in range(1, fs) if y > ff - 1 + 2 * i]
    if y < h - ff:
        out[3] = [(x, y + ff)] + [(x, y + ff + 2 * i) for i in range(1, fs) if y < h - ff - 2 * i]
    if x > ff - 1:
        out[5] = [(x - ff, y)] + [(x - ff - 2 * i, y) for i in range(1, fs) if x > ff - 1 + 2 * i]
    if x < w - ff:
        out[7] = [(x + ff, y)] + [(x + ff + 2 * i, y) for i in range(1, fs) if x < w - ff - 2 * i]
    if y > 0:
        r = [(x, y - 1)]
        for i in range(nl):
            if y > 1 + i and x > i:
                r.append((x - (i + 1), y - 1 - (1 + i)))
            if y > 1 + i and x < w - 1 - i:
                r.append((x + (i + 1), y - 1 - (1 + i)))
        out[0] = r
    if y < h - 1:
        r = [(x, y + 1)]
        for i in range(nl):
            if y < h - 2 - i and x > i:
                r.append((x - (i + 1), y + 1 + (1 + i)))
            if y < h - 2 - i and x < w - 1 - i:
                r.append((x + (i + 1), y + 1 + (1 + i)))
        out[2] = r
    if x > 0:
        r = [(x - 1, y)]
        for i in range(nl):
            if x > 1 + i and y > i:
                r.append((x - 1 - (1 + i), y - (i + 1)))
            if x > 1 + i and y < h - 1 - i:
                r.append((x - 1 - (1 + i), y + (i + 1)))
        out[4] = r
    if x < w - 1:
        r = [(x + 1, y)]
        for i in range(nl):
            if x < w - 2 - i and y > i:
                r.append((x + 1 + (1 + i), y - (i + 1)))
            if x < w - 2 - i and y < h - 1 - i:
                r.append((x + 1 + (1 + i), y + (i + 1)))
        out[6] = r
    return out


def region_pick(reg, costs, strict=True):
    """The position a region hands on: the first one, replaced by a later one only when that one's
    cost is strictly lower (APD.cu:1145, 1221, ...)."""
    bx, by = reg[0]
    for (x, y) in reg[1:]:
        if (costs[y, x] < costs[by, bx]) if strict else (costs[y, x] <= costs[by, bx]):
            bx, by = x, y
    return bx, by


def colour_pixels(colour):
    """Pixels one checkerboard launch sweeps (black = 0: x and y of equal parity), row-major."""
    return [(x, y) for y in range(H) for x in range((y + colour) & 1, W, 2)]


def find_min_cost_index(fc):
    """FindMinCostIndex, APD.cu:60-71: `<=`, so the last minimum wins."""
    mi = 0
    for j in range(1, len(fc)):
        if fc[j] <= fc[mi]:
            mi = j
    return mi


def zero_footprint(costs, exact, c_exact, c_plain, colours=(0, 1), refine_init=False):
    """Pixels whose cost is exactly 0 after the given checkerboard launches over a field of one plain
    (non-exact) plane with a few exact-plane pixels, for ONE source view; also the pixels the
    restatement cannot decide (a candidate cost within 1e-3 of 1.2).

    costs: H x W state, the region scans' input. exact: pixels holding the exact plane. c_exact,
    c_plain: float64 cost of the exact / the plain plane at every pixel (ncc_shift). Per swept pixel p:
    * row j of cost_array is what the initialiser `= {2.0f}` leaves when region j is invalid: 0, except
      row 0, whose first entry is the 2.0 (APD.cu:1120); else the cost at p of the plane of the
      region's pick (strict `<` scans, NaN never wins and never yields);
    * three or more rows above 1.2 leave the only view without weight (APD.cu:1350-1360): every cost
      of p is then NaN, its plane stays, and so does its NaN cost (no comparison with NaN holds);
    * otherwise all 15 samples go to the view, final_costs = rows, mi = FindMinCostIndex; p adopts
      row mi's plane when region mi is valid and its cost is below p's own (APD.cu:1418-1427), in
      REFINE_INIT only when also below p's own cost - 0.1 (APD.cu:1430-1435; nothing the refinement
      finds beats an exact 0, and it cannot reach one from a positive cost);
    * a pixel that adopts nothing ends with some positive cost and a plane that is not exact."""
    costs = costs.astype(np.float64).copy()
    exact = exact.copy()
    unsure = np.zeros((H, W), bool)
    for colour in colours:
        upd = []
        for (x, y) in colour_pixels(colour):
            regs = regions(x, y)
            rows, picks = [], []
            for j, reg in enumerate(regs):
                if reg is None:
                    rows.append(2.0 if j == 0 else 0.0)
                    picks.append(None)
                    continue
                bx, by = region_pick(reg, costs)
                picks.append((bx, by))
                rows.append(c_exact[y, x] if exact[by, bx] else c_plain[y, x])
            if any(abs(r - 1.2) < 1e-3 for r in rows):
                unsure[y, x] = True
            own = c_exact[y, x] if exact[y, x] else c_plain[y, x]
            if sum(r > 1.2 for r in rows) >= 3:
                upd.append((x, y, np.nan, exact[y, x]))
                continue
            mi = find_min_cost_index(rows)
            adopt = regs[mi] is not None and rows[mi] < own and (not refine_init or rows[mi] < own - 0.1)
            if adopt and exact[picks[mi][1], picks[mi][0]]:
                upd.append((x, y, rows[mi], True))
            elif exact[y, x] and own == 0.0:
                upd.append((x, y, 0.0, True))
            else:
                upd.append((x, y, max(min(own, rows[mi]) if adopt else own, 1e-9), False))
        for (x, y, c, e) in upd:  # one launch: its pixels read the other colour only
            costs[y, x] = c
            exact[y, x] = e
    return costs == 0, unsure

# ------------------------------------------------------------------------------------------------
# Multi-hypothesis joint view selection, APD.cu:1323-1374, 174-188
# ------------------------------------------------------------------------------------------------
def cost_threshold(it, thr0=0.8):
    return thr0 * np.exp(it * it / -90.0)  # APD.cu:1340


def sampling_probs(ca, prior, it, count_gt=2, hi=1.2, thr0=0.8):
    """ca: 8 x N candidate costs -> the N unnormalised sampling probabilities (APD.cu:1339-1361): per
    view, over its eight costs c: those under the threshold 0.8 exp(-iter^2 / 90) contribute
    exp(-c^2 / 0.18) and are counted; with more than 2 of them and fewer than 3 costs above 1.2 the
    probability is their mean; with fewer than 3 above 1.2 otherwise exp(-thr^2 / 0.32); else 0; times
    the view's prior. (count_gt, hi, thr0: the rule's constants, for wrong restatements to test against.)"""
    thr = cost_threshold(it, thr0)
    n = ca.shape[1]
    sp = np.zeros(n)
    for i in range(n):
        c = ca[:, i]
        under = c < thr
        count, false = int(under.sum()), int((c > hi).sum())
        if count > count_gt and false < 3:
            sp[i] = np.exp(c[under] ** 2 / -0.18).sum() / count
        elif false < 3:
            sp[i] = np.exp(thr * thr / -0.32)
        sp[i] *= prior[i]
    return sp


def priors(sel, x, y, n, regs):
    """0.9 per near 4-neighbour (of a valid near region) whose selected views hold the view, else 0.1
    (APD.cu:1325-1337); neighbours in the order up, down, left, right = rows 0, 2, 4, 6."""
    pr = np.zeros(n)
    for k, (dx, dy) in enumerate([(0, -1), (0, 1), (-1, 0), (1, 0)]):
        if regs[2 * k] is not None:
            for j in range(n):
                pr[j] += 0.9 if (int(sel[y + dy, x + dx]) >> j) & 1 else 0.1
    return pr


def launch_view_probabilities(cv, sel, colour, it, swap_priors=False, row0_value=2.0, **rule):
    """Per pixel of one checkerboard launch over a field where every pixel holds the same plane: the
    probability that one of the 15 samples lands on each view, i.e. the normalised sampling
    probabilities (the CDF against a uniform draw, APD.cu:174-188, 1363-1374). cv: H x W x N cost of
    that plane per pixel and view. Row j of cost_array holds the pixel's own costs when region j is
    valid, else the zeros of the `= {2.0f}` initialiser (2.0 at [0][0], APD.cu:1120). All zeros where
    no view has any probability (the weights then stay 0); NaN off the launch's colour. Also returns
    the pixels with a cost within 2e-3 of a threshold of the rule (not decidable in float64)."""
    n = cv.shape[-1]
    P = np.full((H, W, n), np.nan)
    unsure = np.zeros((H, W), bool)
    thr = cost_threshold(it)
    for (x, y) in colour_pixels(colour):
        regs = regions(x, y)
        ca = np.zeros((8, n))
        for j, reg in enumerate(regs):
            if reg is not None:
                ca[j] = cv[y, x]
        if regs[0] is None:
            ca[0, 0] = row0_value
        pr = priors(sel, x, y, n, regs)
        sp = sampling_probs(ca, pr[::-1] if swap_priors else pr, it, **rule)
        P[y, x] = sp / sp.sum() if sp.sum() > 0 else 0.0
        unsure[y, x] = (np.abs(cv[y, x] - thr) < 2e-3).any() or (np.abs(cv[y, x] - 1.2) < 2e-3).any()
    return P, unsure


# ------------------------------------------------------------------------------------------------
# ComputeMultiViewInitialCostandSelectedViews, APD.cu:733-773
# ------------------------------------------------------------------------------------------------
def initial_cost_and_views(cv, top_k):
    """cv: the N view costs of one pixel -> (cost, bitmask): views under 2.0 are valid, top_k is capped
    by their number, the cost is the mean of the top_k smallest of ALL costs, the mask every view
    whose cost is <= the top_k-th smallest; no valid view gives (2.0, 0)."""
    cv = np.asarray(cv, np.float64)
    k = min(int((cv < 2.0).sum()), top_k)
    if k == 0:
        return 2.0, 0
    s = np.sort(cv)
    mask = 0
    for i, c in enumerate(cv):
        if c <= s[k - 1]:
            mask |= 1 << i
    return s[:k].sum() / k, mask


# ------------------------------------------------------------------------------------------------
# ComputeGeomConsistencyCost, APD.cu:865-902 (with Get3DPointonWorld_cu / ProjectonCamera_cu,
# APD.cu:831-863), for these cameras: R = I, the source centre at (b, 0, 0)
# ------------------------------------------------------------------------------------------------
def geom_cost(px, py, depth, src_depth_map, b=B, dtype=np.float64, pick=int):
    """Forward-backward reprojection error of the fronto-parallel hypothesis `depth` at (px, py): the
    source depth is read at the truncated source pixel ((int)x, (int)y); 0 there costs 3; the error is
    capped at 3."""
    t = dtype
    f, cx, cy, b = t(F), t(W / 2.0), t(H / 2.0), t(b)
    depth = t(depth)
    X = (depth * (t(px) - cx) / f, depth * (t(py) - cy) / f, depth)  # world = reference frame
    xs = (X[0] - b, X[1], X[2])  # source frame: t = -R C
    sx, sy = (f * xs[0] + cx * xs[2]) / xs[2], (f * xs[1] + cy * xs[2]) / xs[2]
    ix, iy = min(max(pick(sx), 0), W - 1), min(max(pick(sy), 0), H - 1)
    sd = t(src_depth_map[iy, ix])
    if sd == 0:
        return 3.0
    Q = (sd * (sx - cx) / f + b, sd * (sy - cy) / f, sd)  # back to the world
    bx, by = (f * Q[0] + cx * Q[2]) / Q[2], (f * Q[1] + cy * Q[2]) / Q[2]
    dx, dy = t(px) - bx, t(py) - by
    return float(min(t(3.0), np.sqrt(dx * dx + dy * dy)))


# ------------------------------------------------------------------------------------------------
# problems shared by the CPU known-answer tests and their runs on the HIP engine
# ------------------------------------------------------------------------------------------------
def seeded_field(disparity, seeds=SEEDS, rig=None, input_form=False):
    """(planes, exact mask): the fronto-parallel field at `disparity` with the exact plane at seeds."""
    pl = (input_plane_field if input_form else plane_field)(disparity, rig)
    exact = np.zeros((H, W), bool)
    for (x, y) in seeds:
        pl[y, x, 3] = np.float32(D0)
        exact[y, x] = True
    return pl, exact


def footprint_problem(disparity, state, rig=None):
    """One exact-shift source; the prior is the field at `disparity` with the SEEDS exact."""
    _, src = images()
    arr = problem([src], rig=rig, state=state)
    arr.init_planes, exact = seeded_field(disparity, rig=rig, input_form=True)
    return arr, exact


def field_costs(disparity=None):
    """float64 cost of (the exact plane, the plane at `disparity`) at every pixel, exact-shift source."""
    ref, src = images()
    c_exact = ncc_shift(ref, src, float(SHIFT))
    return c_exact, (ncc_shift(ref, src, float(disparity)) if disparity is not None else None)


def init_problem(top_k, kinds=("exact", "exact", "near", "flat"), rig=None):
    """RandomInitialization's problem: sources that see the d0 plane at cost 0 (exact shift), at the
    near-miss cost (the same image from a baseline that makes d0's disparity 4.5) or not at all (a
    constant image: variance floor, cost 2). Returns (problem, H x W x N float64 expected view costs)."""
    ref, src = images()
    c_exact, c_near = field_costs(NEAR_DISP)
    srcs, bl, cv = [], [], []
    for k in kinds:
        srcs.append(np.full((H, W), 90.0, np.float32) if k == "flat" else src)
        bl.append(baseline(NEAR_DISP if k == "near" else SHIFT, rig))
        cv.append({"exact": c_exact, "near": c_near, "flat": np.full((H, W), 2.0)}[k])
    arr = problem(srcs, bl, rig=rig, state=A.REFINE_ITER, top_k=top_k)
    arr.init_planes = input_plane_field(float(SHIFT), rig)
    return arr, np.stack(cv, -1)
