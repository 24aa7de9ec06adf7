"""Helpers of the Weak-sweep known-answer tests (tests/test_oracle_kat_weak.py) and of their runs on
the HIP engine (tests/test_gpu_weak_kat.py). Test infrastructure only.

As in strong_lib: constructions of hand-built problems and restatements of reference rules in numpy
float64 / plain integers, written from the APD.cu lines cited per function. Nothing here calls the
oracle or the kernels.

The construction is strong_lib's exact-seed rig (optionally moved, strong_lib.Rig): every plane is
fronto-parallel, so its homography is the shift x' = x - disparity for every window of NCC-New,
whichever pixel the window sits at. A WEAK pixel's NCC-New cost for the exact plane is exactly 0 (all
ten windows hold equal integers), and a STRONG anchor holding the exact plane is a candidate row of
zeros in CheckerboardPropagationWeak.
"""
import numpy as np

import apd_abi as A
import strong_lib as S
from strong_lib import H, W

# eight anchor offsets around a WEAK pixel (slots 1..8), and the sites of a 64 x 48 scene whose rings
# do not overlap: every anchor lies at x > X_LO, so its centre projects into the source
RING = [(6, 0), (4, 4), (0, 6), (-4, 4), (-6, 0), (-4, -4), (0, -6), (4, -4)]
SITES = [(x, y) for y in (8, 22, 36) for x in (12, 26, 40, 54)]


# ------------------------------------------------------------------------------------------------
# ComputeBilateralNCCNew for fronto-parallel planes of the rig, APD.cu:448-593
# ------------------------------------------------------------------------------------------------
_WINDOW_CACHE = {}


def window_ncc(ref, src, disparity, step, dtype=np.float64):
    """Memoised _window_ncc (the tests ask for the same few maps many times); read-only results."""
    key = (hash(ref.tobytes()), hash(src.tobytes()), float(disparity), step, np.dtype(dtype).name)
    if key not in _WINDOW_CACHE:
        m = _window_ncc(ref, src, disparity, step, dtype)
        m.setflags(write=False)
        _WINDOW_CACHE[key] = m
    return _WINDOW_CACHE[key]


def _window_ncc(ref, src, disparity, step, dtype=np.float64):
    """NCC of the window with taps at -5..5 step `step` (weight 1) around every pixel taken as the
    window's centre, for the shift x' = x - disparity: reference taps clamped texels, source taps
    bilinear with clamp-to-edge (APD.cu:519-545); 2 under the 1e-5 variance floor, else
    max(0, min(2, 1 - covar / sqrt(var_ref var_src)))."""
    ref = ref.astype(dtype)
    src = src.astype(dtype)
    ys, xs = np.mgrid[0:H, 0:W]
    sums = [np.zeros((H, W), dtype) for _ in range(5)]
    disparity = dtype(disparity)
    n = 0
    for i in range(-5, 6, step):
        for j in range(-5, 6, step):
            ry = np.clip(ys + j, 0, H - 1)
            r = ref[ry, np.clip(xs + i, 0, W - 1)]
            sx = (xs + i).astype(dtype) - disparity
            x0 = np.floor(sx)
            a = (sx - x0).astype(dtype)
            x0 = x0.astype(int)
            v0 = src[ry, np.clip(x0, 0, W - 1)]
            v1 = src[ry, np.clip(x0 + 1, 0, W - 1)]
            v = v0 + a * (v1 - v0)
            for k, t in enumerate((r, r * r, v, v * v, r * v)):
                sums[k] += t
            n += 1
    sr, srr, ss, sss, srs = [t / dtype(n) for t in sums]
    var_r = srr - sr * sr
    var_s = sss - ss * ss
    cov = srs - sr * ss
    with np.errstate(invalid="ignore", divide="ignore"):
        c = np.clip(1.0 - cov / np.sqrt(var_r * var_s), 0.0, 2.0)
    return np.where((var_r < 1e-5) | (var_s < 1e-5), 2.0, c).astype(dtype)


def ncc_new_shift(ref, src, disparity, anchors, sel=None, view=0, dtype=np.float64):
    """NCC-New cost of each WEAK pixel anchors[i, 0] for the plane whose homography is the shift by
    `disparity`, given its nine anchors (n x 9 x (x, y), (-1, -1) = missing): 2 where the pixel's
    centre leaves the source (APD.cu:470-473); the centre window (anchor 0, 6 x 6 taps, step 2) and
    one 3 x 3 window (step 5) per present anchor 1..8 (APD.cu:510-560); an anchor whose own centre
    leaves the source returns 2 if it is anchor 0, else counts as an entry of 2.0 only if its selected
    views hold the source (APD.cu:498-509); softmax weights over the anchors' costs (APD.cu:431-446,
    570-583), the weighted sum capped at 2; 0.25 centre + 0.75 anchors (APD.cu:586); no anchor entry
    at all leaves the centre cost."""
    t = dtype
    disparity = float(disparity)
    centre = window_ncc(ref, src, disparity, 2, dtype)
    around = window_ncc(ref, src, disparity, 5, dtype)
    out = np.zeros(len(anchors), dtype)
    for i, a9 in enumerate(np.asarray(anchors, int)):
        px, py = a9[0]
        if not (0 <= px - disparity < W):
            out[i] = 2.0
            continue
        cc, sc, dead = t(0), [], False
        for k, (ax, ay) in enumerate(a9):
            if ax == -1 or ay == -1:
                continue
            if not (0 <= ax - disparity < W):
                if k == 0:
                    dead = True
                    break
                if sel is not None and (int(sel[ay, ax]) >> view) & 1:
                    sc.append(t(2.0))
                continue
            if k == 0:
                cc = centre[ay, ax]
            else:
                sc.append(around[ay, ax])
        if dead:
            out[i] = 2.0
        elif not sc:
            out[i] = cc
        else:
            sc = np.array(sc, t)
            w = np.exp(sc - sc.max())
            w = w / w.sum(dtype=t)
            out[i] = t(0.25) * cc + t(0.75) * min((w * sc).sum(dtype=t), t(2.0))
    return out


def ncc_new_tolerance(ref, src, disparity, anchors, sel=None):
    """Four times the largest float32 - float64 difference of ncc_new_shift over the test's inputs."""
    d = np.abs(ncc_new_shift(ref, src, disparity, anchors, sel, dtype=np.float32).astype(np.float64) -
               ncc_new_shift(ref, src, disparity, anchors, sel))
    return 4.0 * float(d.max())


# ------------------------------------------------------------------------------------------------
# CheckerboardPropagationWeak for one pixel, APD.cu:1442-1615
# ------------------------------------------------------------------------------------------------
def candidate_rows(anchors8, strong8, ca):
    """(flag, cost_array): anchor k = 1..8 is a candidate only if present and STRONG (APD.cu:1471-1482);
    the other rows keep what `cost_array[8][32] = {2.0f}` leaves: zeros, 2.0 at [0][0] (APD.cu:1464)."""
    ca = np.asarray(ca, np.float64)
    flag = [a is not None and bool(s) for a, s in zip(anchors8, strong8)]
    rows = np.zeros((8, ca.shape[1]))
    rows[0, 0] = 2.0
    for j in range(8):
        if flag[j]:
            rows[j] = ca[j]
    return flag, rows


def weak_priors(anchors8, anchor_sel, n):
    """0.9 per anchor that is not (-1, -1) whose selected views hold the view, else 0.1, STRONG or not
    (APD.cu:1490-1503). strong_only: the wrong rule that counts candidates alone."""
    pr = np.zeros(n)
    for a, s in zip(anchors8, anchor_sel):
        if a is not None:
            for j in range(n):
                pr[j] += 0.9 if (int(s) >> j) & 1 else 0.1
    return pr


def weak_view_probs(rows, prior, it, **rule):
    """Probability of each of the 15 draws landing on each view (APD.cu:1505-1540 through
    strong_lib.sampling_probs); all zeros where no view has any probability."""
    sp = S.sampling_probs(rows, prior, it, **rule)
    return sp / sp.sum() if sp.sum() > 0 else np.zeros_like(sp)


def weak_sweep_answer(anchors8, strong8, ca, own, vw, depth_ok=None, geom=None, refine_init=False):
    """One WEAK pixel of CheckerboardPropagationWeak without the refinement, given the 15 draws.

    anchors8: the (x, y) of anchors 1..8, None where (-1, -1); strong8: whether each is STRONG; ca: 8 x N
    float64 NCC-New cost of each anchor's plane at the pixel (rows of non-candidates are ignored); own:
    the N costs of the pixel's own plane; vw: the N view weights drawn; depth_ok: whether each
    candidate's depth at the pixel lies in [depth_min, depth_max] (default: all); geom: None or
    (geom_factor, 8 x N reprojection costs of the anchors' planes at the pixel, N of the own plane).
    * final_costs[j] = sum over views of weight > 0 of w (cost_array[j] + geom_factor * g) / sum w, g = 3
      for a row that is no candidate (APD.cu:1554-1573); no weight at all: 0 / 0, every cost NaN;
    * min_cost_idx = FindMinCostIndex: the last minimum (APD.cu:60-71, 1575);
    * cost_now sums over ALL views (APD.cu:1581-1590);
    * the row is adopted if it is a candidate, its depth is in range and final_costs < cost_now,
      strictly (APD.cu:1594-1596); only then selected_views is written, with the mask of views of
      weight > 0 (APD.cu:1600);
    * REFINE_INIT writes plane and cost only if the result is below cost_now - 0.1 (APD.cu:1605-1610).
    Returns dict(flag, fc, mi, adopt (selected_views written), sel, plane_written, cost)."""
    flag, rows = candidate_rows(anchors8, strong8, ca)
    vw = np.asarray(vw, np.float64)
    own = np.asarray(own, np.float64)
    n = len(vw)
    wn = vw.sum()
    on = vw > 0
    gf = 0.0 if geom is None else geom[0]
    with np.errstate(invalid="ignore", divide="ignore"):
        fc = []
        for j in range(8):
            g = 0.0 if geom is None else (np.asarray(geom[1][j], np.float64) if flag[j] else np.full(n, 3.0))
            fc.append(float((vw[on] * (rows[j][on] + gf * (g[on] if geom is not None else 0.0))).sum() / wn))
        g_own = 0.0 if geom is None else np.asarray(geom[2], np.float64)
        cost_now = float((vw * (own + gf * g_own)).sum() / wn)
    mi = S.find_min_cost_index(fc)
    ok = True if depth_ok is None else bool(depth_ok[mi])
    adopt = bool(flag[mi] and ok and fc[mi] < cost_now)
    cost = fc[mi] if adopt else cost_now
    written = adopt and (not refine_init or cost < cost_now - 0.1)
    if refine_init and not written:
        cost = cost_now
    mask = sum(1 << i for i in range(n) if vw[i] > 0)
    return dict(flag=flag, fc=fc, mi=mi, adopt=adopt, sel=mask if adopt else None, plane_written=written, cost=cost,
                cost_now=cost_now)


# ------------------------------------------------------------------------------------------------
# ComputeGeomConsistencyCost for general cameras, APD.cu:831-902, and the float64 closed forms the
# moved-rig tests compare the geometry helpers with
# ------------------------------------------------------------------------------------------------
def _world_point(cam, x, y, depth, t):
    """Get3DPointonWorld_cu, APD.cu:831-851: R^T (depth K^-1 (x, y, 1)) + C, C = -R^T t."""
    K, R = cam.K.astype(t), cam.R.astype(t)
    X = np.array([depth * (x - K[0, 2]) / K[0, 0], depth * (y - K[1, 2]) / K[1, 1], depth], t)
    return R.T @ X + (-(R.T @ cam.t.astype(t)))


def _project(cam, X, t):
    """ProjectonCamera_cu, APD.cu:853-863."""
    K, R = cam.K.astype(t), cam.R.astype(t)
    c = R @ X + cam.t.astype(t)
    d = K[2] @ c
    return (K[0] @ c) / d, (K[1] @ c) / d, d


def plane_depth(cam, plane, px, py, t=np.float64):
    """Depth along the pixel's ray of the plane (n, w) of the camera frame, n . X + w = 0
    (ComputeDepthfromPlaneHypothesis, APD.cu:237-240, as its closed form)."""
    K = cam.K.astype(t)
    ray = np.array([(px - K[0, 2]) / K[0, 0], (py - K[1, 2]) / K[1, 1], 1.0], t)
    return -t(plane[3]) / (np.asarray(plane[:3], t) @ ray)


def geom_cost_cams(ref_cam, src_cam, px, py, plane, src_depth_map, dtype=np.float64):
    """Forward-backward reprojection error of the plane (sweep form) at (px, py) between two general
    cameras: the source depth is read at the truncated source pixel; 0 there costs 3; capped at 3."""
    t = dtype
    depth = plane_depth(ref_cam, plane, t(px), t(py), t)
    X = _world_point(ref_cam, t(px), t(py), depth, t)
    sx, sy, _ = _project(src_cam, X, t)
    ix, iy = min(max(int(sx), 0), W - 1), min(max(int(sy), 0), H - 1)
    sd = t(src_depth_map[iy, ix])
    if sd == 0:
        return 3.0
    Q = _world_point(src_cam, sx, sy, sd, t)
    bx, by, _ = _project(ref_cam, Q, t)
    return float(min(t(3.0), np.sqrt((t(px) - bx) ** 2 + (t(py) - by) ** 2)))


def map_through_plane(ref_cam, src_cam, plane, x, y, t=np.float64):
    """Where the source sees the point of the plane (reference frame, n . X + w = 0) that the
    reference sees at (x, y): the closed form a plane-induced homography (APD.cu:334-403) must equal."""
    d = plane_depth(ref_cam, plane, t(x), t(y), t)
    sx, sy, _ = _project(src_cam, _world_point(ref_cam, t(x), t(y), d, t), t)
    return sx, sy


# ------------------------------------------------------------------------------------------------
# problems shared by the CPU known-answer tests and their runs on the HIP engine
# ------------------------------------------------------------------------------------------------
class Scene:
    """A 64 x 48 state for one launch of the Weak sweep: a fronto-parallel field (sweep form) with
    WEAK pixels and hand-placed anchors. `sel` starts at SENTINEL at every pixel added, a value no
    launch writes (bit 7: the problems have at most three sources)."""
    SENTINEL = 0x80

    def __init__(self, n_src=1, rig=None, own=S.NEAR_DISP):
        self.n, self.rig = n_src, rig
        self.planes = S.plane_field(own, rig)
        self.weak = np.full((H, W), A.STRONG, np.uint8)
        self.sel = np.full((H, W), (1 << n_src) - 1, np.uint32)
        self.pix = {}

    def exact_plane(self):
        return np.array([0, 0, -1, S.D0], np.float32)

    def add(self, p, anchors8=None, exact=(), states=None, own=None, plane_at=None):
        """WEAK pixel p with anchors 1..8 (default: RING around p; None = missing); the anchors whose
        slots (1..8) are in `exact` hold the exact plane; states: slot -> pixel state of that anchor;
        plane_at: slot -> effective disparity of that anchor's plane; own: p's effective disparity."""
        x, y = p
        a8 = [(x + dx, y + dy) for dx, dy in RING] if anchors8 is None else list(anchors8)
        self.weak[y, x] = A.WEAK
        self.sel[y, x] = self.SENTINEL
        if own is not None:
            self.planes[y, x, 3] = np.float32(S.depth_of(own, self.rig))
        for k in exact:
            ax, ay = a8[k - 1]
            self.planes[ay, ax] = self.exact_plane()
        for k, d in (plane_at or {}).items():
            ax, ay = a8[k - 1]
            self.planes[ay, ax, 3] = np.float32(S.depth_of(d, self.rig))
        for k, st in (states or {}).items():
            ax, ay = a8[k - 1]
            self.weak[ay, ax] = st
        self.pix[p] = a8
        return self

    def order(self):
        return sorted(self.pix, key=lambda p: p[1] * W + p[0])

    def anchors(self):
        out = np.full((len(self.pix), 9, 2), -1, np.int16)
        for i, p in enumerate(self.order()):
            out[i, 0] = p
            for k, a in enumerate(self.pix[p]):
                if a is not None:
                    out[i, 1 + k] = a
        return out

    def anchors_of(self, p):
        return self.anchors()[self.order().index(p)][None]


def ring_points(cx, cy, r, skip=()):
    """The eight (or, with `skip`, fewer) points at multiples of 45 degrees on a ring around (cx, cy)."""
    pts = []
    for k in range(8):
        if k not in skip:
            a = 2 * np.pi * k / 8
            pts.append((int(round(cx + r * np.cos(a))), int(round(cy + r * np.sin(a)))))
    return pts


# ring centres of the engine problems: rings of radius 8 that keep two pixels between neighbours
RING_CENTRES = [(x, y) for y in (12, 34) for x in (15, 33, 51)]


def ring_problem(n_src, state, block, six=(1, 4), rig=None, own=S.NEAR_DISP, one_colour=False, srcs=None, **params):
    """An ordinary use_APD problem (input-form planes): UNKNOWN background and WEAK blocks holding the
    field at `own`, each block inside a ring of STRONG pixels that hold the exact plane. The rings
    listed in `six` have six points, so GenAnchors leaves the blocks' last two anchors missing.
    block: (half width, half height) of the WEAK block around each ring centre; one_colour keeps the
    pixels with x + y even only. Returns (problem, H x W mask of the WEAK pixels asked for)."""
    _, src = S.images()
    srcs = [src] * n_src if srcs is None else srcs
    arr = S.problem(srcs, rig=rig, state=state, use_APD=1, rotate_time=1, **params)
    planes = S.input_plane_field(own, rig)
    exact = S.input_plane_field(float(S.SHIFT), rig)
    weak = np.full((H, W), A.UNKNOWN, np.uint8)
    asked = np.zeros((H, W), bool)
    for i, (cx, cy) in enumerate(RING_CENTRES):
        for (x, y) in ring_points(cx, cy, 8, skip=(2, 6) if i in six else ()):
            weak[y, x] = A.STRONG
            planes[y, x] = exact[y, x]
        for dy in range(-block[1], block[1] + 1):
            for dx in range(-block[0], block[0] + 1):
                if not one_colour or (cx + dx + cy + dy) % 2 == 0:
                    weak[cy + dy, cx + dx] = A.WEAK
                    asked[cy + dy, cx + dx] = True
    arr.weak_info = weak
    arr.confidence = np.ones((H, W), np.uint8)
    arr.init_planes = planes
    arr.depths = [np.full((H, W), S.D0, np.float32)] * (1 + len(srcs))
    return arr, asked


def check_ring_run(a, b, asked, n_src, refine_init=False, own=S.NEAR_DISP):
    """The known answer of one prepare + iteration(0) over a ring_problem whose sources all see the
    exact plane at cost 0, from what was read back after prepare (a: states, anchors, selected views,
    costs) against what was read back after the iteration (b). Returns the numbers of pixels (adopted,
    blocked) it checked.

    After prepare a WEAK pixel either lost its state (too few directions: UNKNOWN, not swept by the
    Weak sweep) or has anchors on its ring. The ring points are STRONG and hold the exact plane, at
    cost exactly 0 in every view that is drawn: no strictly lower cost exists, so the Strong sweep
    leaves their planes alone (checked on b: the iteration changed none of them), and every candidate
    row of a WEAK pixel is the exact plane's: zeros in every drawn view, as are the rows of missing
    anchors (the 2.0 of [0][0] aside). With identical sources every view has the same costs and the
    same priors, so the 15 draws are arbitrary but sum to 15; a source that is the negative of the
    image (the exact plane correlates at -1: cost 2 in all its rows, more than two above 1.2) is
    never drawn, though RandomInitialization still selected it for the WEAK pixels (their near-miss
    plane costs just under 2 there): the written mask, 1, then differs from the initial one, 3. final_costs are all 0 (row 0 cannot be missing: the anchors are
    sorted present-first), min_cost_idx is 7, and the pixel adopts anchor 8's plane iff anchor 8 is
    present: cost exactly 0, the anchor's plane bit for bit, selected_views = the mask of views with
    weight > 0. Nothing the refinement tries is strictly below 0. If anchor 8 is missing nothing is
    adopted and selected_views keeps its value (the refinement never writes it). REFINE_INIT writes
    the adopted plane only if 0 < cost_now - 0.1, which the near-miss field (cost_now < 0.1) never
    meets: the planes stay bit for bit and the cost is the initial one, though selected_views is
    written all the same where anchor 8 is present (APD.cu:1600 comes before 1605)."""
    wc = int(a.weak_count[0])
    idx = np.flatnonzero((a.weak_info == A.WEAK).ravel())
    assert len(idx) > 0 and wc >= len(idx)
    slots = np.flatnonzero(asked.ravel())  # anchors follow the WEAK order of the input states
    adopted = blocked = 0
    exact = np.array([0, 0, -1, S.D0], np.float32)
    for c in idx:
        y, x = divmod(int(c), W)
        a9 = a.anchors[int(np.searchsorted(slots, c))]
        assert tuple(a9[0]) == (x, y)
        present = [(int(ax), int(ay)) for ax, ay in a9[1:] if ax != -1 and ay != -1]
        assert len(present) >= 6
        for ax, ay in present:  # what the Weak sweep saw: no Weak launch writes a STRONG pixel
            assert a.weak_info[ay, ax] == A.STRONG and np.abs(b.planes[ay, ax] - exact).max() <= 1e-6
            assert np.array_equal(b.planes[ay, ax].view(np.uint32), a.planes[ay, ax].view(np.uint32))
        vw = b.view_weights[:, y, x].astype(int)
        assert vw.sum() == 15
        last = a9[8]
        full = bool(last[0] != -1 and last[1] != -1)
        mask = sum(1 << i for i in range(n_src) if vw[i] > 0)
        if refine_init:
            # both costs are float32 means of one value below 0.1 taken n_src or 15 times: a few ulps apart
            assert np.array_equal(b.planes[y, x].view(np.uint32), a.planes[y, x].view(np.uint32))
            assert abs(float(b.costs[y, x]) - float(a.costs[y, x])) <= 1e-6 and 0 < b.costs[y, x] < 0.1
            assert int(b.selected_views[y, x]) == (mask if full else int(a.selected_views[y, x]))
            adopted, blocked = adopted + full, blocked + (not full)
        elif full:
            lx, ly = int(last[0]), int(last[1])
            assert b.costs[y, x] == 0
            assert np.array_equal(b.planes[y, x].view(np.uint32), b.planes[ly, lx].view(np.uint32))
            assert np.abs(b.planes[y, x] - exact).max() <= 1e-6
            assert int(b.selected_views[y, x]) == mask
            adopted += 1
        else:
            assert int(b.selected_views[y, x]) == int(a.selected_views[y, x])
            blocked += 1
    return adopted, blocked


# (name, sources, state, WEAK block, one colour only, rig): the ring problems of the engine tests
RING_CASES = [
    ("n3_54_weak", 3, A.REFINE_ITER, (1, 1), False, None),          # 54 WEAK pixels: one partial group
    ("n1_90_weak", 1, A.REFINE_ITER, (2, 1), False, None),          # 90: a full group and a partial one
    ("n3_72_weak_one_colour", 3, A.REFINE_ITER, (2, 2), True, None),
    ("n3_moved_rig", 3, A.REFINE_ITER, (1, 1), False, S.MOVED),
    ("n1_refine_init", 1, A.REFINE_INIT, (1, 1), False, None),
    ("n2_negative_view", 2, A.REFINE_ITER, (1, 1), False, None),    # selected_views after != before where adopted
]


RING_WEAK = {"n3_54_weak": 54, "n1_90_weak": 90, "n3_72_weak_one_colour": 72, "n3_moved_rig": 54, "n1_refine_init": 54,
             "n2_negative_view": 54}


def ring_case(name):
    _, n, state, block, one, rig = next(c for c in RING_CASES if c[0] == name)
    srcs = None
    if name == "n2_negative_view":
        _, src = S.images()
        srcs = [src, (255.0 - src).astype(np.float32)]
    arr, asked = ring_problem(n, state, block, rig=rig, one_colour=one, srcs=srcs)
    return arr, asked, n, state == A.REFINE_INIT
