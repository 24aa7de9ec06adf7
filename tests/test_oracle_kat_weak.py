"""Known-answer tests for the Weak sweep of the oracle and for the geometry under both sweeps (CPU only).

k_sweep_weak of oracle/apd_oracle.c is what every version of the HIP kernel k_sweep_weak_vm was
admitted against, bit for bit. These tests pin it to answers derived independently of it, from
CheckerboardPropagationWeak and PlaneHypothesisRefinementWeak (APD.cu:1442-1615, 1008-1096) restated
in numpy float64 / plain integers (tests/weak_lib.py, tests/strong_lib.py), on hand-built 64 x 48
states run through stage 8 of oracle_kat_stage_ex: one colour of the Weak sweep on caller state, the
fit plane an input (a zero fit normal makes the refinement drop out, APD.cu:1028-1030, so a launch
is deterministic but for the 15 view draws).

The second half runs on a moved rig (strong_lib.MOVED: the world rotated by 25 degrees about
(1, 2, 3) and shifted, fy = 80 != fx = 64, the sources' principal point 2 px off the reference's):
to every restatement it is the exact-seed rig, to the code under test a general camera pair, so
to_ref / to_world, R_relative, the reference centre, the K[0] / K[4] roles and Ks != Kr are
exercised away from the identity. Column X_LO is left out there (its centre projects to 0 minus
rounding), and planes are compared in sweep form or normals within 1e-6.

Tests that need exact ties between non-zero costs stay on the identity rig:
test_equal_cost_candidate_is_not_adopted and test_geometry_terms (its equal-cost site).
tools/mutate_oracle.py (WEAK_MUTATIONS, GEOMETRY_MUTATIONS) restates each rule wrongly in turn and
requires these tests to fail.
"""
import ctypes as C

import numpy as np
import pytest

import apd_abi as A
import cases
import oracle_lib
import strong_lib as S
import synth
import weak_lib as Wk
from strong_lib import H, W, ptr

RIGS = [pytest.param(None, id="identity"), pytest.param(S.MOVED, id="moved")]
EXACT = np.array([0, 0, -1, S.D0], np.float32)


@pytest.fixture(scope="module")
def lib():
    lib = oracle_lib.load()
    lib.oracle_ncc_new.restype = C.c_float
    lib.oracle_ncc_new.argtypes = [C.POINTER(A.ApdProblem), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float),
                                   C.POINTER(C.c_int16), C.POINTER(C.c_uint32)]
    return lib


def stage(lib, arr, stage_id, it=0, colour=0, sel=None, costs=None, planes=None, weak=None, anchors=None, vw=None,
          fit=None):
    pb = arr.build()
    st = lib.oracle_kat_stage_ex(C.byref(pb), stage_id, it, colour, ptr(sel), ptr(costs), ptr(planes), ptr(weak), None,
                                 None, ptr(anchors), None, ptr(vw), ptr(fit))
    assert st == 0


def weak_sweep(lib, arr, sc, colours=(0, 1), it=0, fit=None):
    """The given colours of the Weak sweep over a weak_lib.Scene -> (planes, costs, sel, view weights)."""
    n = len(arr.images) - 1
    planes, sel, weak, anchors = sc.planes.copy(), sc.sel.copy(), sc.weak.copy(), sc.anchors()
    costs = np.full((H, W), 0.5, np.float32)
    vw = np.zeros((n, H, W), np.uint8)
    fit = np.zeros((H, W, 4), np.float32) if fit is None else np.ascontiguousarray(fit, np.float32)
    for c in colours:
        stage(lib, arr, 8, it, c, sel=sel, costs=costs, planes=planes, weak=weak, anchors=anchors, vw=vw, fit=fit)
    return planes, costs, sel, vw


def problem(n_src=1, rig=None, srcs=None, **params):
    _, src = S.images()
    params.setdefault("state", A.REFINE_ITER)
    arr = S.problem([src] * n_src if srcs is None else srcs, rig=rig, use_APD=1, **params)
    arr.depths = [np.full((H, W), S.D0, np.float32)] * len(arr.images)  # use_APD problems carry depth maps
    return arr


def eff_disparity(depth, rig):
    return S.F * S.baseline(S.SHIFT, rig) / float(depth) - (rig.m if rig else 0)


def answer(sc, p, srcs, vw, sel=None, **kw):
    """weak_sweep_answer of pixel p of the scene for the given source images and drawn weights, the
    costs restated by ncc_new_shift from each plane's effective disparity."""
    ref, _ = S.images()
    a8 = sc.pix[p]
    a9 = sc.anchors_of(p)
    sel = sc.sel if sel is None else sel
    cost = lambda d: [float(Wk.ncc_new_shift(ref, s, d, a9, sel, v)[0]) for v, s in enumerate(srcs)]
    ca = [cost(eff_disparity(sc.planes[a[1], a[0], 3], sc.rig)) if a is not None else [0.0] * len(srcs) for a in a8]
    own = cost(eff_disparity(sc.planes[p[1], p[0], 3], sc.rig))
    strong = [a is not None and sc.weak[a[1], a[0]] == A.STRONG for a in a8]
    return Wk.weak_sweep_answer(a8, strong, ca, own, vw, **kw)


def is_exact(plane):
    return np.array_equal(plane.view(np.uint32), EXACT.view(np.uint32))


# ------------------------------------------------------------------------------------------------
# the construction itself, checked with the float64 restatement alone
# ------------------------------------------------------------------------------------------------
def test_construction_bounds():
    """What the known answers rest on, over every site of weak_lib.SITES with the full ring: the exact
    plane costs exactly 0 (no anchor window falls under the 1e-5 variance floor, which would cost 2);
    the near-miss costs are positive, below 0.1 and below the view-selection threshold of iterations
    0 and 2; the far-miss costs are above 0.1 + 1e-3 and below 1.2."""
    ref, src = S.images()
    sc = Wk.Scene()
    for p in Wk.SITES:
        sc.add(p)
    a = sc.anchors()
    assert (Wk.window_ncc(ref, src, float(S.SHIFT), 5)[:, S.X_LO + 1:] == 0).all()
    assert (Wk.ncc_new_shift(ref, src, float(S.SHIFT), a) == 0).all()
    near = Wk.ncc_new_shift(ref, src, S.NEAR_DISP, a)
    assert near.min() > 1e-3 and near.max() < 0.1 and near.max() < S.cost_threshold(2)
    far = Wk.ncc_new_shift(ref, src, S.FAR_DISP, a)
    assert far.min() > 0.1 + 1e-3 and far.max() < 1.2


@pytest.mark.parametrize("disparity", [S.NEAR_DISP, S.FAR_DISP])
def test_ncc_new_matches_restatement(lib, disparity):
    """oracle_ncc_new over the sites (full rings, and rings with two anchors missing) against
    ncc_new_shift, within four times the restatement's own float32 - float64 difference."""
    ref, src = S.images()
    arr = problem()
    sc = Wk.Scene()
    for i, p in enumerate(Wk.SITES):
        ring = [(p[0] + dx, p[1] + dy) for dx, dy in Wk.RING]
        sc.add(p, ring if i % 2 else ring[:6] + [None, None])
    arr.weak_info = sc.weak
    pb = arr.build()
    a = sc.anchors()
    want = Wk.ncc_new_shift(ref, src, disparity, a)
    tol = Wk.ncc_new_tolerance(ref, src, disparity, a)
    assert 0 < tol < 2e-4
    pl = np.array([0, 0, -1, S.depth_of(disparity)], np.float32)
    for i, p in enumerate(sc.order()):
        a9 = np.ascontiguousarray(a[i])
        got = lib.oracle_ncc_new(C.byref(pb), p[0], p[1], 1, S.fptr(pl), a9.ctypes.data_as(C.POINTER(C.c_int16)), None)
        assert abs(got - want[i]) <= tol, (p, got, want[i])


# ------------------------------------------------------------------------------------------------
# a, b. candidate rows and the rows of `= {2.0f}`, APD.cu:1464-1482, 60-71, 1575, 1594
# ------------------------------------------------------------------------------------------------
def _rows_scene(rig):
    """Sites (near-miss own plane, near-miss anchors unless said):
    0 eight exact anchors; 1 all exact, slot 8 missing; 2 all exact, slot 3 missing; 3 exact at slot 6
    only, slot 3 missing; 4 exact at slot 3 only, slot 6 missing; 5 exact at slot 8 only, but that
    anchor is UNKNOWN; 6 exact at slot 8 only, that anchor STRONG; 7 exact at slot 2 only, anchor 8
    UNKNOWN and near-miss."""
    sc = Wk.Scene(rig=rig)
    ring = lambda p, missing=(): [None if k + 1 in missing else (p[0] + dx, p[1] + dy) for k, (dx, dy) in enumerate(Wk.RING)]
    P = Wk.SITES
    sc.add(P[0], exact=range(1, 9))
    sc.add(P[1], ring(P[1], (8,)), exact=range(1, 8))
    sc.add(P[2], ring(P[2], (3,)), exact=[1, 2, 4, 5, 6, 7, 8])
    sc.add(P[3], ring(P[3], (3,)), exact=[6])
    sc.add(P[4], ring(P[4], (6,)), exact=[3])
    sc.add(P[5], exact=[8], states={8: A.UNKNOWN})
    sc.add(P[6], exact=[8])
    sc.add(P[7], exact=[2], states={8: A.UNKNOWN})
    return sc


@pytest.mark.parametrize("rig", RIGS)
def test_candidate_and_flagless_rows(lib, rig):
    """One source, both colours. An anchor is a candidate only if present and STRONG; any other row is
    all zeros, so its final cost is 0, FindMinCostIndex's `<=` takes the last minimum, and a flagless
    row that is the last minimum blocks the adoption: site 0 adopts the exact plane at cost exactly
    0, selected_views = 1; site 1 (slot 8 missing, after every exact anchor) adopts nothing and keeps
    its selected_views; site 2 (slot 3 missing, exact anchors after it) adopts; site 3 adopts slot 6's
    exact plane over the earlier zero row; site 4 (exact at 3, missing at 6) is blocked; site 5's exact
    anchor is not STRONG: its row is zeros and blocks; site 6 adopts; site 7's non-STRONG anchor 8
    blocks slot 2's exact plane. Blocked sites keep their plane bit for bit, at the near-miss cost."""
    arr = problem(rig=rig)
    sc = _rows_scene(rig)
    _, src = S.images()
    planes, costs, sel, vw = weak_sweep(lib, arr, sc)
    adopts = {0: True, 1: False, 2: True, 3: True, 4: False, 5: False, 6: True, 7: False}
    ref, _ = S.images()
    for k, want in adopts.items():
        p = Wk.SITES[k]
        x, y = p
        assert vw[0, y, x] == 15
        ans = answer(sc, p, [src], [15])
        assert ans["adopt"] == want, (k, ans)
        if want:
            assert costs[y, x] == 0 and is_exact(planes[y, x]) and sel[y, x] == 1, k
        else:
            assert sel[y, x] == Wk.Scene.SENTINEL, k
            assert np.array_equal(planes[y, x].view(np.uint32), sc.planes[y, x].view(np.uint32)), k
            tol = Wk.ncc_new_tolerance(ref, src, S.NEAR_DISP, sc.anchors_of(p))
            assert abs(costs[y, x] - ans["cost"]) <= tol and ans["cost"] > 1e-3, (k, costs[y, x], ans["cost"])
    strong = sc.weak != A.WEAK
    assert np.array_equal(planes[strong].view(np.uint32), sc.planes[strong].view(np.uint32))


def test_row0_missing_holds_the_2(lib):
    """Row 0 of a missing anchor 1 holds the 2.0 of `= {2.0f}` in view 0 (APD.cu:1464). One source:
    with anchors 2 and 3 holding the plane at depth_min (its centre leaves the source: cost 2), the
    2.0 is the third cost above 1.2, the view gets no weight and the cost turns NaN; with anchor 1
    present (exact) there are two and the pixel adopts. Two identical sources: row 0's final cost is
    2 w0 / (w0 + w1), not 0; own plane far-miss, anchors 2..8 near-miss: anchor 8's plane is adopted
    iff w0 > 0; with w0 = 0 row 0 costs 0, the only minimum, and blocks."""
    _, src = S.images()
    arr = problem()
    sc = Wk.Scene()
    d_out = float(S.F * S.B / S.DMIN)
    for k, p in enumerate(Wk.SITES[:2]):
        ring = [(p[0] + dx, p[1] + dy) for dx, dy in Wk.RING]
        sc.add(p, ([None] if k == 0 else ring[:1]) + ring[1:], exact=[4, 5, 6, 7, 8] + ([1] if k else []),
               plane_at={2: d_out, 3: d_out})
    planes, costs, sel, vw = weak_sweep(lib, arr, sc)
    (x0, y0), (x1, y1) = Wk.SITES[:2]
    assert vw[0, y0, x0] == 0 and np.isnan(costs[y0, x0]) and sel[y0, x0] == Wk.Scene.SENTINEL
    assert np.array_equal(planes[y0, x0].view(np.uint32), sc.planes[y0, x0].view(np.uint32))
    assert vw[0, y1, x1] == 15 and costs[y1, x1] == 0 and is_exact(planes[y1, x1])
    # two sources: anchors' selected views favour view 1, so w0 = 0 occurs among the seeds
    arr = problem(2)
    seen = set()
    for seed in range(1, 13):
        arr.seed = seed
        sc = Wk.Scene(2, own=S.FAR_DISP)
        for p in Wk.SITES:
            ring = [(p[0] + dx, p[1] + dy) for dx, dy in Wk.RING]
            sc.add(p, [None] + ring[1:], plane_at={k: S.NEAR_DISP for k in range(2, 9)})
            for (ax, ay) in ring[1:]:
                sc.sel[ay, ax] = 2
        planes, costs, sel, vw = weak_sweep(lib, arr, sc)
        for p in Wk.SITES:
            x, y = p
            w = vw[:, y, x].astype(int)
            assert w.sum() == 15
            ans = answer(sc, p, [src, src], w)
            assert abs(ans["fc"][0] - 2.0 * w[0] / 15.0) < 1e-12
            assert ans["adopt"] == (w[0] > 0)
            seen.add(bool(w[0] > 0))
            if w[0] > 0:
                near = np.float32(S.depth_of(S.NEAR_DISP))
                assert planes[y, x, 3] == near and sel[y, x] == sum(1 << i for i in range(2) if w[i] > 0)
            else:
                assert planes[y, x, 3] == sc.planes[y, x, 3] and sel[y, x] == Wk.Scene.SENTINEL
    assert seen == {True, False}


# ------------------------------------------------------------------------------------------------
# c. priors, APD.cu:1490-1503
# ------------------------------------------------------------------------------------------------
def _lattice(n_src, rig=None, x_from=S.X_LO + 8, every=2):
    """WEAK pixels at even x, even y with anchors at odd offsets (never WEAK themselves)."""
    offs = [(3, 0), (1, 1), (0, 3), (-1, 1), (-3, 0), (-1, -1), (0, -3), (1, -1)]
    sc = Wk.Scene(n_src, rig, own=float(S.SHIFT))
    for y in range(4, H - 4, every):
        for x in range(x_from + (x_from % 2), W - 4, every):
            sc.add((x, y), [(x + dx, y + dy) for dx, dy in offs])
    return sc


@pytest.mark.parametrize("layout,p_rule,p_wrong", [("mixed", 0.5, 0.9), ("all view 0", 0.9, 0.1)])
def test_priors_count_every_present_anchor(lib, layout, p_rule, p_wrong):
    """Two identical sources, every plane exact: all costs are 0 in both views, so the probabilities
    are in the ratio of the priors. "mixed": anchors 1..4 are STRONG with selected views {0}, anchors
    5..8 UNKNOWN with selected views {1}: the reference sums over every anchor that is not (-1, -1)
    (APD.cu:1490-1503), priors (4.0, 4.0), p0 = 0.5; counting candidates only would give (3.6, 0.4),
    p0 = 0.9. "all view 0": eight STRONG anchors with selected views {0}: (7.2, 0.8), p0 = 0.9; 0.9 and
    0.1 swapped would give 0.1. The weight of view 0 summed over the pixels is within 4.5 binomial
    sigma of 15 n p0 and not of the wrong rule's. Deterministic end: all anchors missing leaves every
    prior 0 and no view is drawn (test_no_view_drawn)."""
    arr = problem(2)
    sc = _lattice(2, every=4)
    for p, a8 in sc.pix.items():
        for k, (ax, ay) in enumerate(a8):
            mixed = layout == "mixed" and k >= 4
            sc.sel[ay, ax] = 2 if mixed else 1
            if mixed:
                sc.weak[ay, ax] = A.UNKNOWN
    _, _, _, vw = weak_sweep(lib, arr, sc)
    pts = sc.order()
    n = len(pts)
    assert n >= 100
    w0 = sum(int(vw[0, y, x]) for x, y in pts)
    assert all(int(vw[:, y, x].sum()) == 15 for x, y in pts)
    a8 = sc.pix[pts[0]]
    pr = Wk.weak_priors(a8, [sc.sel[ay, ax] for ax, ay in a8], 2)
    assert abs(pr[0] / pr.sum() - p_rule) < 1e-12
    for p0, inside in ((p_rule, True), (p_wrong, False)):
        assert (abs(w0 - 15 * n * p0) <= 4.5 * np.sqrt(15 * n * p0 * (1 - p0))) == inside, (w0, n, p0)


# ------------------------------------------------------------------------------------------------
# d. thresholds at this call site, APD.cu:1506-1540
# ------------------------------------------------------------------------------------------------
def _within(got, P, sigmas=4.5):
    want = 15.0 * float(P.sum())
    sd = np.sqrt(15.0 * float((P * (1 - P)).sum()))
    return abs(got - want) <= sigmas * sd + 1e-9, got, want, sd


@pytest.mark.parametrize("it", [0, 2])
def test_view_selection_thresholds(lib, it):
    """Views (exact copy, graded source), every plane exact, every anchor present, STRONG and holding
    both views: view 0's eight costs are 0, view 1's the pixel's NCC-New cost c under the graded
    source, spread over 0.05 .. 1.4 by the lattice of WEAK pixels. Deterministic: c > 1.2 means eight
    costs above 1.2, view 1 gets weight 0 and view 0 all 15. By groups, each within 4.5 sigma of
    15 sum P: c under the threshold 0.8 exp(-iter^2 / 90) (exp(-c^2 / 0.18), count = 8 > 2), c from the
    threshold to 1.2 (the fallback exp(-thr^2 / 0.32)). For each wrong constant (count > 8 cannot be
    told here; threshold 0.9; above 1.0; fallback 0.18; threshold without iter at iter 2) the pixels
    whose probability it moves by more than 0.05 form a group on which the wrong expectation must
    FAIL. Every pixel's weights sum to 15. Pixels within 2e-3 of a threshold are left out."""
    ref, src = S.images()
    g = S.graded_source()
    arr = problem(srcs=[src, g])
    sc = _lattice(2)
    sc.sel[:] = 3
    _, _, _, vw = weak_sweep(lib, arr, sc, it=it)
    pts = sc.order()
    c = Wk.ncc_new_shift(ref, g, float(S.SHIFT), sc.anchors())
    thr = S.cost_threshold(it)
    ok = (np.abs(c - thr) > 2e-3) & (np.abs(c - 1.2) > 2e-3) & (np.abs(c - 1.0) > 2e-3) & (np.abs(c - 0.9) > 2e-3)
    w = np.array([[int(vw[v, y, x]) for x, y in pts] for v in range(2)])
    assert (w.sum(0) == 15).all()

    def probs(**rule):
        out = np.zeros(len(pts))
        for i in range(len(pts)):
            rows = np.stack([np.zeros(8), np.full(8, c[i])], -1)
            out[i] = Wk.weak_view_probs(rows, np.array([8 * 0.9] * 2), it, **rule)[1]
        return out

    P = probs()
    dead = ok & (c > 1.2)
    assert dead.sum() >= 5 and (w[1][dead] == 0).all() and (w[0][dead] == 15).all()
    groups = {"under": ok & (c < thr), "fallback": ok & (c >= thr) & (c <= 1.2)}
    for name, gm in groups.items():
        assert gm.sum() >= 25, name
        good, *rest = _within(float(w[1][gm].sum()), P[gm])
        assert good, (name, rest)
    wrong = {"0.9 exp": dict(thr0=0.9), "above 1.0": dict(hi=1.0)}
    for name, rule in wrong.items():
        Pw = probs(**rule)
        gm = ok & (np.abs(Pw - P) > 0.05)
        assert gm.sum() >= 2, name
        good, *rest = _within(float(w[1][gm].sum()), P[gm])
        assert good, (name, rest)
        bad, *_ = _within(float(w[1][gm].sum()), Pw[gm])
        assert not bad, f"the group of '{name}' does not tell the rule from its wrong restatement"
    if it == 2:  # a threshold that ignores iter: costs between 0.8 exp(-4 / 90) and 0.8
        gm = ok & (c >= thr) & (c < 0.8)
        Pw = np.exp(-c ** 2 / 0.18) / (1 + np.exp(-c ** 2 / 0.18))
        assert gm.sum() >= 5
        good, *rest = _within(float(w[1][gm].sum()), P[gm])
        bad, *_ = _within(float(w[1][gm].sum()), Pw[gm])
        assert good and not bad, rest


def test_count_needs_more_than_two(lib):
    """`count > 2` (APD.cu:1520) with exactly two and exactly three costs under the threshold. Views
    (graded source, exact copy); the present anchors hold the exact plane, whose cost c under the
    graded source lies between the threshold and 1.2 at the pixels chosen, and the last `k` slots are
    missing (zero rows, under the threshold). k = 2: count = 2, fallback exp(-0.64 / 0.32) = 0.135 against view 1's 1; k = 3:
    count = 3, mean of three 1's = 1. Row 0 is never the missing one. Over the chosen pixels and
    seeds view 0's weight is within 4.5 sigma of the rule's expectation and not of the expectation
    with `count > 3`."""
    ref, src = S.images()
    g = S.graded_source()
    arr = problem(srcs=[g, src])
    offs = [(3, 0), (1, 1), (0, 3), (-1, 1), (-3, 0), (-1, -1), (0, -3), (1, -1)]
    cand = [(x, y) for y in range(6, H - 6, 4) for x in range(S.X_LO + 8, W - 4, 2)]
    got = {2: 0.0, 3: 0.0}
    P = {2: [], 3: []}
    Pw = {2: [], 3: []}
    for k in (2, 3):
        sc = Wk.Scene(2, own=float(S.SHIFT))
        sc.sel[:] = 3
        for (x, y) in cand:
            sc.add((x, y), [(x + dx, y + dy) for dx, dy in offs[:8 - k]] + [None] * k)
        c = Wk.ncc_new_shift(ref, g, float(S.SHIFT), sc.anchors())
        pts = sc.order()
        keep = [i for i in range(len(pts)) if 0.8 + 2e-3 < c[i] < 1.2 - 2e-3]
        assert len(keep) >= 8
        for seed in (1, 2, 3):
            arr.seed = seed
            _, _, _, vw = weak_sweep(lib, arr, sc)
            for i in keep:
                x, y = pts[i]
                rows = np.zeros((8, 2))
                rows[:8 - k, 0] = c[i]
                pr = np.array([(8 - k) * 0.9] * 2)
                P[k].append(Wk.weak_view_probs(rows, pr, 0)[0])
                Pw[k].append(Wk.weak_view_probs(rows, pr, 0, count_gt=3)[0])
                got[k] += int(vw[0, y, x])
                assert int(vw[:, y, x].sum()) == 15
    for k in (2, 3):
        good, *rest = _within(got[k], np.array(P[k]))
        assert good, (k, rest)
    bad, *_ = _within(got[3], np.array(Pw[3]))
    assert not bad and abs(np.mean(P[3]) - np.mean(Pw[3])) > 0.05


# ------------------------------------------------------------------------------------------------
# e. no view drawn, APD.cu:1529-1552, 1572, 1589
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_src", [1, 3])
def test_no_view_drawn(lib, n_src):
    """All eight anchors missing: every prior is 0, the CDF is 0 / 0, no draw lands, weight_norm is 0
    and every cost 0 / 0: the cost is NaN, the plane and selected_views stay. The same where the only
    view has three candidate costs above 1.2 (three anchors at depth_min, one source)."""
    arr = problem(n_src)
    sc = Wk.Scene(n_src)
    sc.add(Wk.SITES[0], [None] * 8)
    if n_src == 1:
        sc.add(Wk.SITES[1], exact=[4, 5, 6, 7, 8], plane_at={k: float(S.F * S.B / S.DMIN) for k in (1, 2, 3)})
    planes, costs, sel, vw = weak_sweep(lib, arr, sc)
    for (x, y) in sc.pix:
        assert (vw[:, y, x] == 0).all() and np.isnan(costs[y, x]) and sel[y, x] == Wk.Scene.SENTINEL
        assert np.array_equal(planes[y, x].view(np.uint32), sc.planes[y, x].view(np.uint32))
        assert np.isnan(answer(sc, (x, y), [S.images()[1]] * n_src, [0] * n_src)["cost"])


# ------------------------------------------------------------------------------------------------
# g. adoption, APD.cu:1594-1601
# ------------------------------------------------------------------------------------------------
def test_equal_cost_candidate_is_not_adopted(lib):
    """Identity rig (an exact tie between non-zero costs). Every anchor holds the pixel's own
    near-miss plane: final_costs equal cost_now bit for bit, `<` fails, selected_views keeps its
    value. With anchor 8 a hair better (the exact plane) it is written."""
    arr = problem()
    sc = Wk.Scene()
    sc.add(Wk.SITES[0])
    sc.add(Wk.SITES[1], exact=[8])
    planes, costs, sel, vw = weak_sweep(lib, arr, sc)
    (x0, y0), (x1, y1) = Wk.SITES[:2]
    assert vw[0, y0, x0] == 15 and sel[y0, x0] == Wk.Scene.SENTINEL
    assert not answer(sc, Wk.SITES[0], [S.images()[1]], [15])["adopt"]
    assert sel[y1, x1] == 1 and costs[y1, x1] == 0


@pytest.mark.parametrize("rig", RIGS)
@pytest.mark.parametrize("dmin,dmax,adopts", [(S.DMIN, 8.0, True), (S.DMIN, 7.999, False), (8.0, S.DMAX, True),
                                              (8.001, S.DMAX, False)])
def test_adoption_needs_the_depth_in_range(lib, rig, dmin, dmax, adopts):
    """The exact plane's depth at the pixel is 8 (to float32 rounding on the moved rig, hence the
    bounds 1e-3 off): adopted with depth_max = 8 + and depth_min = 8 - (the ends are included,
    APD.cu:1596), not with depth_max = 7.999 or depth_min = 8.001. Two sources, the second a constant
    image (cost 2 in all eight rows: no weight): selected_views is written only on adoption and is
    then the mask of views with weight > 0, 1, not 3."""
    _, src = S.images()
    inc = 1e-3 if rig else 0.0
    arr = problem(rig=rig, srcs=[src, np.full((H, W), 90.0, np.float32)],
                  depth_min=dmin - (inc if adopts else 0), depth_max=dmax + (inc if adopts else 0))
    sc = Wk.Scene(2, rig)
    sc.add(Wk.SITES[5], exact=range(1, 9))
    planes, costs, sel, vw = weak_sweep(lib, arr, sc)
    x, y = Wk.SITES[5]
    assert tuple(vw[:, y, x]) == (15, 0)
    if adopts:
        assert sel[y, x] == 1 and costs[y, x] == 0 and is_exact(planes[y, x])
    else:
        assert sel[y, x] == Wk.Scene.SENTINEL and costs[y, x] > 1e-3
        assert np.array_equal(planes[y, x].view(np.uint32), sc.planes[y, x].view(np.uint32))


# ------------------------------------------------------------------------------------------------
# h. refinement, APD.cu:1008-1096
# ------------------------------------------------------------------------------------------------
def test_refinement(lib):
    """The fit plane is tried first, under the same test (APD.cu:1026-1052): a far-miss pixel (anchors
    far-miss too) whose fit plane is the exact plane ends at cost exactly 0 with the fit plane's bits;
    with depth_max below the fit plane's depth it does not. A pixel at cost exactly 0 is never
    replaced, whatever its fit plane. A zero fit normal skips everything (APD.cu:1028-1030): the
    near-miss pixel keeps its plane bit for bit (with a fit plane equal to its own plane the five
    candidates run: 2 %, 0.02 pi perturbations of a plane half a pixel off find a better one at most
    sites). The five candidates are built from the plane and depth AFTER the fit step (APD.cu:1055-
    1067): far-miss pixels (disparity 7) whose fit plane is the near-miss plane (disparity 4.5) and
    is adopted; the perturbed depth is then within 2 % of the fit plane's, 4.41 .. 4.59 px, and
    lowers the cost whenever it falls on the side of 4; built from the old depth it would lie at
    6.86 .. 7.14 px, no better than the fit plane. So over the sites and seeds at least a quarter
    end strictly below the fit plane's cost with a depth within 2.1 % of the fit plane's."""
    arr = problem()
    far = {k: S.FAR_DISP for k in range(1, 9)}
    sc = Wk.Scene(own=S.FAR_DISP)
    fit = np.zeros((H, W, 4), np.float32)
    P = Wk.SITES
    sc.add(P[0], plane_at=far)                       # fit = exact
    fit[P[0][1], P[0][0]] = EXACT
    sc.add(P[1], own=float(S.SHIFT), plane_at=far)   # at cost 0, fit = near-miss
    fit[P[1][1], P[1][0]] = [0, 0, -1, S.depth_of(S.NEAR_DISP)]
    sc.add(P[2], own=S.NEAR_DISP)                    # zero fit
    planes, costs, sel, vw = weak_sweep(lib, arr, sc, fit=fit)
    (x0, y0), (x1, y1), (x2, y2) = P[:3]
    assert costs[y0, x0] == 0 and is_exact(planes[y0, x0]) and sel[y0, x0] == Wk.Scene.SENTINEL
    assert costs[y1, x1] == 0 and is_exact(planes[y1, x1])
    assert np.array_equal(planes[y2, x2].view(np.uint32), sc.planes[y2, x2].view(np.uint32))
    arr7 = problem(depth_max=7.999)
    p7, c7, _, _ = weak_sweep(lib, arr7, sc, fit=fit)
    assert c7[y0, x0] > 0 and not is_exact(p7[y0, x0])
    # candidates from the state after the fit step
    ref, src = S.images()
    better = total = 0
    d_fit = float(np.float32(S.depth_of(S.NEAR_DISP)))
    for seed in (1, 2, 3, 4):
        arr.seed = seed
        sc = Wk.Scene(own=S.FAR_DISP)
        fit = np.zeros((H, W, 4), np.float32)
        for p in P:
            sc.add(p, plane_at=far)
            fit[p[1], p[0]] = [0, 0, -1, d_fit]
        planes, costs, _, _ = weak_sweep(lib, arr, sc, fit=fit)
        c_fit = Wk.ncc_new_shift(ref, src, S.NEAR_DISP, sc.anchors())
        for i, (x, y) in enumerate(sc.order()):
            assert costs[y, x] <= c_fit[i] + 1e-4     # the fit plane, or something better
            d = float(Wk.plane_depth(S.camera(), planes[y, x], x, y))
            total += 1
            better += bool(costs[y, x] < c_fit[i] - 1e-4 and abs(d / d_fit - 1) <= 0.021)
    assert total == 48 and better >= total // 4, (better, total)


# ------------------------------------------------------------------------------------------------
# i. REFINE_INIT, APD.cu:1590, 1605-1610
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rig", RIGS)
def test_refine_init(lib, rig):
    """The result is written only if below costs[center] - 0.1, costs[center] being the cost_now just
    stored. Near-miss pixels (cost_now < 0.1) with eight exact anchors: planes stay bit for bit, the
    cost is cost_now, yet selected_views IS written (APD.cu:1600 precedes 1605). Far-miss pixels
    (cost_now > 0.1): the exact plane is adopted at cost 0."""
    _, src = S.images()
    ref, _ = S.images()
    arr = problem(rig=rig, state=A.REFINE_INIT)
    sc = Wk.Scene(rig=rig)
    for p in Wk.SITES[:6]:
        sc.add(p, exact=range(1, 9))
    for p in Wk.SITES[6:]:
        sc.add(p, exact=range(1, 9), own=S.FAR_DISP)
    planes, costs, sel, vw = weak_sweep(lib, arr, sc)
    for k, (x, y) in enumerate(Wk.SITES):
        ans = answer(sc, (x, y), [src], [15], refine_init=True)
        assert ans["adopt"] and sel[y, x] == 1
        assert ans["plane_written"] == (k >= 6)
        if k < 6:
            assert np.array_equal(planes[y, x].view(np.uint32), sc.planes[y, x].view(np.uint32))
            tol = Wk.ncc_new_tolerance(ref, src, S.NEAR_DISP, sc.anchors_of((x, y)))
            assert abs(costs[y, x] - ans["cost"]) <= tol and 1e-3 < ans["cost"] < 0.1
        else:
            assert costs[y, x] == 0 and is_exact(planes[y, x])


# ------------------------------------------------------------------------------------------------
# j. geometric consistency, APD.cu:1559-1565, 1582-1584
# ------------------------------------------------------------------------------------------------
def test_geometry_terms(lib):
    """geom_consistency with the source depth map at the true plane (D0 everywhere): the reprojection
    cost of a fronto-parallel plane is its disparity error, capped at 3: exact 0, near-miss 0.5,
    disparity 5.5 1.5, far-miss 3; geom_factor 0.2. Site 0: exact anchors with slot 8 missing; the
    missing row now costs 0 + 0.2 * 3 = 0.6, the exact rows 0: the missing anchor no longer blocks, the
    pixel adopts at cost 0 (to 1e-5: the float32 reprojection of the exact plane is not exactly 0).
    Site 1: all anchors near-miss and the own plane near-miss (identity rig: an exact tie): rows and
    cost_now both carry + 0.1, equal, no adoption; a flagged row without its geometric term would win.
    Site 2: far-miss own and anchors, slot 8 missing: rows 0.7 + 0.6 against the missing row's 0.6:
    blocked. Site 3: far-miss own plane, anchors at disparity 5.5 (cost about 0.2 + 0.3), slot 8
    missing: the rows lie between 0.4 and 0.6, under the missing row's 0.6 only because it adds
    geom_factor * 3 and not * 2: adopted. Restated through weak_sweep_answer with geom_cost_cams."""
    _, src = S.images()
    ref, _ = S.images()
    arr = problem(geom_consistency=1, geom_factor=0.2)
    flat = np.full((H, W), S.D0, np.float32)
    arr.depths = [flat, flat]
    sc = Wk.Scene()
    P = Wk.SITES
    ring = lambda p: [(p[0] + dx, p[1] + dy) for dx, dy in Wk.RING]
    sc.add(P[0], ring(P[0])[:7] + [None], exact=range(1, 8))
    sc.add(P[1])
    sc.add(P[2], ring(P[2])[:7] + [None], own=S.FAR_DISP, plane_at={k: S.FAR_DISP for k in range(1, 8)})
    sc.add(P[3], ring(P[3])[:7] + [None], own=S.FAR_DISP, plane_at={k: 5.5 for k in range(1, 8)})
    planes, costs, sel, vw = weak_sweep(lib, arr, sc)
    cams = (S.camera(), S.camera(S.B, source=True))
    adopts = {0: True, 1: False, 2: False, 3: True}
    for k, p in enumerate(P[:4]):
        x, y = p
        g = lambda q: [Wk.geom_cost_cams(*cams, x, y, sc.planes[q[1], q[0]], flat)]
        geom = (0.2, [g(a) if a is not None else [0.0] for a in sc.pix[p]], g(p))
        ans = answer(sc, p, [src], [15], geom=geom)
        assert vw[0, y, x] == 15
        assert ans["adopt"] == adopts[k], (k, ans)
        if k != 1:
            assert abs(ans["fc"][7] - 0.6) < 1e-12
        if k == 3:
            assert 0.4 + 0.02 < ans["fc"][6] < 0.6 - 0.02 and ans["mi"] == 6
        held = sc.pix[p][ans["mi"]] if ans["adopt"] else p
        tol = 1e-5 + Wk.ncc_new_tolerance(ref, src, eff_disparity(sc.planes[held[1], held[0], 3], None), sc.anchors_of(p))
        assert abs(costs[y, x] - ans["cost"]) <= tol, (k, costs[y, x], ans["cost"])
        assert np.array_equal(planes[y, x].view(np.uint32), sc.planes[held[1], held[0]].view(np.uint32))
        assert sel[y, x] == (1 if ans["adopt"] else Wk.Scene.SENTINEL)
    assert abs(answer(sc, P[1], [src], [15], geom=None)["cost_now"] + 0.1 - costs[P[1][1], P[1][0]]) < 1e-4


# ------------------------------------------------------------------------------------------------
# k. launch order, APD.cu:1617-1652
# ------------------------------------------------------------------------------------------------
def test_launches_sweep_weak_pixels_of_their_colour(lib):
    """Black (x + y even) then red; a launch touches the WEAK pixels of its colour only, in every row
    (at 48 rows the launch wrappers' row limit is the image height), and no STRONG pixel ever."""
    arr = problem()
    sc = Wk.Scene()
    sites = [(12, 8), (27, 8), (40, 22), (55, 22), (12, 36), (27, 41), (54, 6)]
    for p in sites:
        sc.add(p, exact=range(1, 9))
    for colours in ((0,), (1,), (0, 1)):
        planes, costs, sel, vw = weak_sweep(lib, arr, sc, colours=colours)
        for (x, y) in sites:
            swept = (x + y) % 2 in colours
            assert (costs[y, x] == 0 and is_exact(planes[y, x]) and vw[0, y, x] == 15) == swept
            assert swept or (costs[y, x] == 0.5 and sel[y, x] == Wk.Scene.SENTINEL and vw[0, y, x] == 0)
        m = sc.weak != A.WEAK
        assert np.array_equal(planes[m].view(np.uint32), sc.planes[m].view(np.uint32)) and (costs[m] == 0.5).all()
    assert {(x + y) % 2 for x, y in sites} == {0, 1}


@pytest.mark.parametrize("name", ["refine_init_apd_small"])
def test_hand_staged_iteration_equals_staged_run(lib, name):
    """Stages 5 (black, red), 6 and 8 (black, red) on the state after prepare reproduce
    oracle_run_staged's first iteration: the hook runs the sweep the oracle runs."""
    orun = lambda arr: oracle_lib.run(lib, arr)
    arr = cases.make_case(name, orun)
    a = oracle_lib.run_staged(lib, arr, 0)
    b = oracle_lib.run_staged(lib, arr, 1)
    h, w = arr.height, arr.width
    n = len(arr.images) - 1
    planes, costs, sel = a.planes.copy(), a.costs.copy(), a.selected_views.copy()
    weak, vw = a.weak_info.copy(), np.zeros((n, h, w), np.uint8)
    wc = int(a.weak_count[0])
    assert wc > 0 and (weak == A.WEAK).sum() > 0
    # anchors in the WEAK order of the states after prepare
    slots = np.flatnonzero((np.asarray(arr.weak_info) == A.WEAK).ravel())
    keep = np.flatnonzero((weak == A.WEAK).ravel())
    anchors = np.ascontiguousarray(a.anchors[np.searchsorted(slots, keep)])
    fit = np.zeros((h, w, 4), np.float32)
    for c in (0, 1):
        stage(lib, arr, 5, 0, c, sel=sel, costs=costs, planes=planes, weak=weak, vw=vw)
    stage(lib, arr, 6, 0, planes=planes, weak=weak, anchors=anchors, fit=fit)
    for c in (0, 1):
        stage(lib, arr, 8, 0, c, sel=sel, costs=costs, planes=planes, weak=weak, anchors=anchors, vw=vw, fit=fit)
    assert np.array_equal(planes.view(np.uint32), b.planes.view(np.uint32))
    assert np.array_equal(costs.view(np.uint32), b.costs.view(np.uint32))
    assert np.array_equal(sel, b.selected_views) and np.array_equal(vw, b.view_weights)


# ------------------------------------------------------------------------------------------------
# the moved rig: geometry helpers against float64 closed forms
# ------------------------------------------------------------------------------------------------
def _slanted(depth_at_centre=S.D0, n=(0.2, -0.1, -1.0)):
    """A slanted plane of the reference frame (sweep form) through the principal ray at the given depth."""
    n = np.asarray(n, np.float64) / np.linalg.norm(n)
    return np.array([*n, -(n @ np.array([0.0, 0.0, depth_at_centre]))], np.float64)


PLANES = [np.array([0.0, 0.0, -1.0, S.D0]), _slanted(), _slanted(5.0, (-0.3, 0.25, -1.0))]
PIXELS = [(7, 5), (32, 24), (50, 11), (61, 44), (20, 40)]


def _sigma_tol(f):
    """Four times the float32 - float64 difference of a restatement f(dtype) -> array."""
    return 4.0 * float(np.abs(np.asarray(f(np.float32), np.float64) - np.asarray(f(np.float64))).max())


@pytest.mark.parametrize("rig", RIGS)
def test_homography_maps_through_the_plane(lib, rig):
    """oracle_homography (ComputeHomography, APD.cu:334-394) on rotated cameras with fy != fx and
    Ks != Kr, for fronto-parallel and slanted planes: H applied to a reference pixel lands where the
    source sees the plane's point on that pixel's ray (float64 pinhole projection, no homography
    involved). Tolerance: four times the float32 - float64 difference of that closed form (plus the
    float32 resolution of a pixel coordinate near 64, 4e-6 ulp x 4 operations)."""
    _, src = S.images()
    arr = problem(rig=rig)
    pb = arr.build()
    cr, cs = S.camera(0.0, rig), S.camera(S.baseline(S.SHIFT, rig), rig, source=True)
    for pl in PLANES:
        H9 = np.zeros(9, np.float32)
        lib.oracle_homography(C.byref(pb), 1, S.fptr(pl.astype(np.float32)), S.fptr(H9))
        Hm = H9.astype(np.float64).reshape(3, 3)
        closed = lambda t: [Wk.map_through_plane(cr, cs, pl.astype(np.float32), x, y, t) for x, y in PIXELS]
        tol = _sigma_tol(closed) + 4 * 64 * 2.0 ** -23
        assert tol < 5e-4
        for (x, y), (sx, sy) in zip(PIXELS, closed(np.float64)):
            q = Hm @ np.array([x, y, 1.0])
            assert abs(q[0] / q[2] - sx) <= tol and abs(q[1] / q[2] - sy) <= tol, (pl, x, y, q[:2] / q[2], sx, sy)
    # a source turned against the reference (7 degrees about (2, -1, 1)): R_relative is no identity
    turned = S.camera(S.baseline(S.SHIFT, rig), rig, source=True)
    Rt = S._rodrigues((2.0, -1.0, 1.0), 7.0)
    centre = turned.center
    turned.R = Rt @ turned.R
    turned.t = -turned.R @ centre
    arr.cameras[1] = synth.camera_struct_values(turned, W, H)
    pb = arr.build()
    for pl in PLANES:
        H9 = np.zeros(9, np.float32)
        lib.oracle_homography(C.byref(pb), 1, S.fptr(pl.astype(np.float32)), S.fptr(H9))
        Hm = H9.astype(np.float64).reshape(3, 3)
        closed = lambda t: [Wk.map_through_plane(cr, turned, pl.astype(np.float32), x, y, t) for x, y in PIXELS]
        tol = _sigma_tol(closed) + 4 * 64 * 2.0 ** -23
        assert tol < 5e-4
        for (x, y), (sx, sy) in zip(PIXELS, closed(np.float64)):
            q = Hm @ np.array([x, y, 1.0])
            assert abs(q[0] / q[2] - sx) <= tol and abs(q[1] / q[2] - sy) <= tol, (pl, x, y, q[:2] / q[2], sx, sy)
    sx, sy = Wk.map_through_plane(cr, cs, PLANES[0], 40, 20)  # the exact plane is the shift by SHIFT on any rig
    assert abs(sx - (40 - S.SHIFT)) < 1e-9 and abs(sy - 20) < 1e-9


@pytest.mark.parametrize("rig", RIGS)
def test_depth_from_plane_and_distance_to_origin(lib, rig):
    """ComputeDepthfromPlaneHypothesis and GetDistance2Origin (APD.cu:237-240, 218-223) with fy != fx
    against their closed forms: depth = -w / (n . K^-1 (x, y, 1)), distance = -(n . depth K^-1 (x, y, 1)).
    Tolerance: four times the float32 - float64 difference of the closed form over the test's inputs."""
    cam = S.camera(0.0, rig)
    cs = A.camera_from_values(synth.camera_struct_values(cam, W, H))
    for pl in PLANES:
        p32 = pl.astype(np.float32)
        closed = lambda t: [Wk.plane_depth(cam, p32, t(x), t(y), t) for x, y in PIXELS]
        tol = _sigma_tol(closed) + 4 * 16 * 2.0 ** -23  # ... plus four float32 roundings of a depth below 16
        assert tol < 1e-4
        for (x, y), d in zip(PIXELS, closed(np.float64)):
            got = lib.oracle_depth_from_plane(C.byref(cs), S.fptr(p32), x, y)
            assert abs(got - d) <= tol, (pl, x, y, got, d)
            ray = np.array([(x - cam.K[0, 2]) / cam.K[0, 0], (y - cam.K[1, 2]) / cam.K[1, 1], 1.0])
            want = -(p32[:3].astype(np.float64) @ (ray * d))
            back = lib.oracle_dist2origin(C.byref(cs), x, y, np.float32(d), S.fptr(p32))
            assert abs(back - want) <= tol + 4e-6 and abs(want - float(p32[3])) < 1e-6


def _slanted_input(rig):
    """Input-form field (world normal, depth) of the slanted plane PLANES[1], and its sweep form."""
    cam = S.camera(0.0, rig)
    Rg = np.asarray(rig.Rg) if rig else np.eye(3)
    pl = PLANES[1]
    out = np.zeros((H, W, 4), np.float32)
    out[..., :3] = (Rg @ pl[:3]).astype(np.float32)
    for y in range(H):
        for x in range(W):
            out[y, x, 3] = Wk.plane_depth(cam, pl, x, y)
    return out, pl


@pytest.mark.parametrize("rig", RIGS)
def test_to_ref_and_to_world_through_a_staged_run(lib, rig):
    """TransformNormal2RefCam at the start and TransformNormal at the end (APD.cu:415-423, 405-413):
    a slanted input field with world normals Rg n. After prepare the sweep-form planes are (n, w) of
    the reference frame within 1e-6 (w = the plane's distance, 1e-5); after the finish of a run with
    no iteration the output normals are Rg n again within 1e-6."""
    _, src = S.images()
    arr = S.problem([src], rig=rig, state=A.REFINE_ITER)
    arr.init_planes, pl = _slanted_input(rig)
    a = oracle_lib.run_staged(lib, arr, 0)
    assert np.abs(a.planes[..., :3] - pl[:3]).max() <= 1e-6
    assert np.abs(a.planes[..., 3] - pl[3]).max() <= 1e-5
    b = oracle_lib.run_staged(lib, arr, 0, do_finish=True)
    assert np.abs(b.planes[..., :3] - arr.init_planes[..., :3]).max() <= 1e-6
    if rig:  # the transposed rotation is a different vector by far more than the tolerance
        Rg = np.asarray(rig.Rg)
        assert np.abs(Rg @ pl[:3] - Rg.T @ pl[:3]).max() > 0.05


# ------------------------------------------------------------------------------------------------
# the moved rig: the Strong half's known answers, restated for it
# ------------------------------------------------------------------------------------------------
def strong_sweep(lib, arr, planes, costs, colours=(0, 1)):
    n = len(arr.images) - 1
    planes, costs = planes.copy(), np.ascontiguousarray(costs, np.float32).copy()
    sel = np.full((H, W), (1 << n) - 1, np.uint32)
    vw = np.zeros((n, H, W), np.uint8)
    for c in colours:
        stage(lib, arr, 5, 0, c, sel=sel, costs=costs, planes=planes, vw=vw)
    return planes, costs, sel, vw


def test_moved_propagation_footprint(lib):
    """test_oracle_kat_strong.test_propagation_footprint on the moved rig: the same seeds, the same
    integer restatement of the regions, the costs of the effective disparities. Column X_LO is left
    out of the comparison and of the restatement's candidates (cost 2 there: its centre projects to
    0 minus rounding); the seeds do not depend on it."""
    rig = S.MOVED
    c_exact, c_near = (c.copy() for c in S.field_costs(S.NEAR_DISP))
    c_exact[:, S.X_LO] = 2.0
    c_near[:, S.X_LO] = 2.0
    arr, _ = S.footprint_problem(S.NEAR_DISP, A.REFINE_ITER, rig)
    planes, exact = S.seeded_field(S.NEAR_DISP, rig=rig)
    costs = np.where(exact, 0.0, c_near).astype(np.float32)
    p2, got, _, _ = strong_sweep(lib, arr, planes, costs)
    want, unsure = S.zero_footprint(costs, exact, c_exact, c_near)
    zero = (got == 0) & (p2.view(np.uint32) == EXACT.view(np.uint32)).all(-1)
    m = np.ones((H, W), bool)
    m[:, :S.X_LO + 1] = False
    assert not unsure[m].any() and want[m].sum() > 150
    assert np.array_equal(zero[m], want[m]), np.argwhere((zero != want) & m)[:10]


@pytest.mark.parametrize("top_k", [1, 2, 3, 4])
def test_moved_initial_cost_and_selected_views(lib, top_k):
    """test_initial_cost_and_selected_views on the moved rig, from input-form planes (world normal
    Rg n, depth): to_ref, the homography of rotated cameras and the near-miss baseline all enter."""
    arr, cv = S.init_problem(top_k, rig=S.MOVED)
    costs, sel = np.zeros((H, W), np.float32), np.zeros((H, W), np.uint32)
    planes = np.ascontiguousarray(arr.init_planes).copy()
    stage(lib, arr, 4, sel=sel, costs=costs, planes=planes)
    want = [[S.initial_cost_and_views(cv[y, x], top_k) for x in range(W)] for y in range(H)]
    wc = np.array([[w[0] for w in r] for r in want])
    wm = np.array([[w[1] for w in r] for r in want], np.uint32)
    m = np.ones((H, W), bool)
    m[:, S.X_LO:S.X_LO + 2] = False  # X_LO, and the near-miss view's edge column X_LO + 1 (4.5 rounds up)
    assert np.array_equal(sel[m], wm[m])
    assert np.abs(costs - wc)[m].max() <= S.ncc_tolerance(S.NEAR_DISP)
    assert (wm[:, S.X_LO + 2:] == (3 if top_k < 3 else 7)).all() and (costs[:, :S.X_LO] == 2).all()
    assert np.abs(planes[..., :3] - np.array([0, 0, -1])).max() <= 1e-6


def test_moved_geom_cost_known_values(lib):
    """test_geom_cost_known_values on the moved rig: the reprojection error of a fronto-parallel
    hypothesis at depth d' against the true depth map at d0 is fx b |1 / d' - 1 / d0| px, whatever the
    world frame, fy or the sources' principal point; the chain is restated for general cameras
    (weak_lib.geom_cost_cams: R^T and the centre on the way out, R, t and the full K on the way in)."""
    rig = S.MOVED
    _, src = S.images()
    arr = S.problem([src], rig=rig, geom_consistency=1)
    b = S.baseline(S.SHIFT, rig)
    cams = (S.camera(0.0, rig), S.camera(b, rig, source=True))
    px, py = 40, 20
    flat = np.full((H, W), S.D0, np.float32)
    pb_plane = lambda d: np.array([0, 0, -1, d], np.float32)
    probes = (6.0, 7.0, 9.0, 12.0, 2.0, 8.0)
    tol = 4 * max(abs(Wk.geom_cost_cams(*cams, px, py, pb_plane(d), flat, np.float32) -
                      Wk.geom_cost_cams(*cams, px, py, pb_plane(d), flat)) for d in probes)
    assert 0 < tol < 2e-4
    for d in probes:
        arr.depths = [flat, flat]
        want = Wk.geom_cost_cams(*cams, px, py, pb_plane(d), flat)
        assert abs(want - min(3.0, S.F * b * abs(1 / d - 1 / S.D0))) < 1e-9
        pb = arr.build()
        got = lib.oracle_geom_cost(C.byref(pb), px, py, 1, S.fptr(pb_plane(d)))
        assert abs(got - want) <= tol, (d, got, want)
    arr.depths = [flat, np.zeros((H, W), np.float32)]
    pb = arr.build()
    assert lib.oracle_geom_cost(C.byref(pb), px, py, 1, S.fptr(pb_plane(7.0))) == 3.0


@pytest.mark.parametrize("impetus", [1, 0])
def test_moved_sweep_adds_geom_factor_times_geom_cost(lib, impetus):
    """test_sweep_adds_geom_factor_times_geom_cost on the moved rig (a source depth map of holes: every
    plane's geometric cost is 3): 0 inside, geom_factor * 3 = 0.6 in the columns x >= W - 3 with
    use_impetus, 0 without."""
    rig = S.MOVED
    _, src = S.images()
    arr = S.problem([src], rig=rig, state=A.REFINE_ITER, geom_consistency=1, use_impetus=impetus, geom_factor=0.2)
    arr.depths = [np.full((H, W), S.D0, np.float32), np.zeros((H, W), np.float32)]
    planes = S.plane_field(float(S.SHIFT), rig)
    _, got, _, _ = strong_sweep(lib, arr, planes, np.zeros((H, W), np.float32))
    assert (got[3:H - 3, S.X_LO + 4:W - 3] == 0).all()
    assert np.abs(got[:, W - 3:] - (0.6 if impetus else 0.0)).max() <= 1e-6


# ------------------------------------------------------------------------------------------------
# the engine tests' ring problems (tests/test_gpu_weak_kat.py) on the oracle: whole runs
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c[0] for c in Wk.RING_CASES])
def test_ring_problems_satisfy_the_known_answer(lib, name):
    """prepare + one iteration of an ordinary use_APD problem (GenAnchors, RandomInitialization, the
    Strong sweep, the RANSAC fit and the Weak sweep with its refinement): weak_lib.check_ring_run's
    answer, from the anchors and costs after prepare. Both kinds of pixel occur: full rings that
    adopt, six-point rings whose missing anchors block."""
    arr, asked, n, refine_init = Wk.ring_case(name)
    a = oracle_lib.run_staged(lib, arr, 0)
    b = oracle_lib.run_staged(lib, arr, 1)
    adopted, blocked = Wk.check_ring_run(a, b, asked, n, refine_init)
    assert adopted >= 10 and blocked >= 5, (adopted, blocked)
    swept = a.weak_info == A.WEAK
    if name == "n2_negative_view":  # a blocked pixel keeps 3, an adopting one writes 1
        assert (a.selected_views[swept] == 3).all() and (b.view_weights[1][swept] == 0).all()
        assert sorted(np.unique(b.selected_views[swept])) == [1, 3]
    ys, xs = np.nonzero(swept)
    assert {int(v) for v in (xs + ys) % 2} == ({0} if "one_colour" in name else {0, 1})
    assert np.array_equal(b.weak_info, a.weak_info)


def test_ring_problem_without_a_view(lib):
    """One constant source: every cost is 2, no view is ever drawn: all costs NaN, planes unchanged."""
    arr, asked = Wk.ring_problem(1, A.REFINE_ITER, (1, 1), srcs=[np.full((H, W), 90.0, np.float32)])
    a = oracle_lib.run_staged(lib, arr, 0)
    b = oracle_lib.run_staged(lib, arr, 1)
    m = a.weak_info == A.WEAK
    assert m.sum() >= 30 and (a.costs == 2).all()
    assert np.isnan(b.costs[m]).all() and (b.view_weights[:, m] == 0).all()
    assert np.array_equal(b.planes[m].view(np.uint32), a.planes[m].view(np.uint32))
    assert np.array_equal(b.selected_views[m], a.selected_views[m])
