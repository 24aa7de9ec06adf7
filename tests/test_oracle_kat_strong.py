"""Known-answer tests for the Strong half of the oracle: the PatchMatch core (CPU only).

The HIP kernels are checked bit-for-bit against oracle/apd_oracle.c; these tests pin the oracle's
Strong-half rules to answers derived independently of it, from the APD.cu lines each test cites,
restated in numpy float64 or plain integers (tests/strong_lib.py) on hand-built 64 x 48 problems:

* CheckerboardPropagationStrong's eight regions, their strict `<` scans, the zero rows the
  `cost_array[8][32] = {2.0f}` initialiser leaves for invalid regions and FindMinCostIndex's `<=`
  (APD.cu:60-71, 1098-1322, 1388-1427): which pixels take over an exact (cost 0) plane;
* REFINE_INIT's -0.1 rule (APD.cu:1430-1435);
* ComputeMultiViewInitialCostandSelectedViews (APD.cu:723-774);
* the view selection (APD.cu:1323-1374, 174-188): priors, thresholds, fallback, 15 samples;
* the five refinement candidates (APD.cu:961-980, 242-305);
* ComputeGeomConsistencyCost (APD.cu:865-902) away from zero, and use_impetus in the sweep;
* RANSACToGetFitPlane (APD.cu:2486-2598); LocalRefine (APD.cu:2346-2432);
* oracle_run_staged(max_iterations, finish) == oracle_run_patchmatch.
tools/mutate_oracle.py restates each rule wrongly in turn and requires these tests to fail.
"""
import ctypes as C

import numpy as np
import pytest

import apd_abi as A
import cases
import oracle_lib
import strong_lib as S
from strong_lib import H, W, ptr


@pytest.fixture(scope="module")
def lib():
    return oracle_lib.load()


def stage(lib, arr, stage_id, it=0, colour=0, sel=None, costs=None, planes=None, weak=None, anchors=None, vw=None,
          fit=None):
    pb = arr.build()
    st = lib.oracle_kat_stage_ex(C.byref(pb), stage_id, it, colour, ptr(sel), ptr(costs), ptr(planes), ptr(weak), None,
                                 None, ptr(anchors), None, ptr(vw), ptr(fit))
    assert st == 0


def sweep(lib, arr, planes, costs, sel=None, colours=(0, 1), it=0):
    """The given colours of the Strong sweep on caller state -> (planes, costs, sel, view weights)."""
    n = len(arr.images) - 1
    planes, costs = planes.copy(), np.ascontiguousarray(costs, np.float32).copy()
    sel = np.full((H, W), (1 << n) - 1, np.uint32) if sel is None else sel.copy()
    vw = np.zeros((n, H, W), np.uint8)
    for c in colours:
        stage(lib, arr, 5, it, c, sel=sel, costs=costs, planes=planes, vw=vw)
    return planes, costs, sel, vw


@pytest.fixture(scope="module")
def fields():
    c_exact, c_near = S.field_costs(S.NEAR_DISP)
    _, c_far = S.field_costs(S.FAR_DISP)
    return c_exact, c_near, c_far


ncc_tolerance = S.ncc_tolerance


# ------------------------------------------------------------------------------------------------
# the construction itself, checked with the float64 restatement alone
# ------------------------------------------------------------------------------------------------
def test_construction_bounds(fields):
    """The exact plane costs exactly 0 wherever its centre stays in the source; the near-miss costs
    are positive, below 0.1 and below the view-selection threshold 0.8 exp(-iter^2 / 90) of every
    iteration used (APD.cu:1340); at most 2 % of the far-miss pixels have three or more of their eight
    candidates above 1.2 (the field has one plane: all valid candidates share the pixel's own cost)."""
    c_exact, c_near, c_far = fields
    assert (c_exact[:, S.X_LO:] == 0).all() and (c_exact[:, :S.X_LO] == 2).all()
    near = c_near[:, S.X_LO + 1:]
    assert near.min() > 1e-3 and near.max() < 0.1 and near.max() < S.cost_threshold(2)
    far = c_far[:, int(S.FAR_DISP):]
    assert (far > 1.2).mean() <= 0.02 and far.min() > 0.1 + 1e-3


# ------------------------------------------------------------------------------------------------
# a. propagation footprint, APD.cu:1098-1322 (regions), 1120 (zero rows), 60-71 (last minimum)
# ------------------------------------------------------------------------------------------------
def _zero_set(planes, costs):
    """Pixels at cost exactly 0 that hold the seeds' plane bit for bit. (The plane is part of the
    set's definition because max(0, .) in the NCC (APD.cu:661) also rounds a near-perfect match to an
    exact 0: a red pixel may take over a black neighbour's refined, slightly slanted plane at cost 0.)"""
    e = np.array([0, 0, -1, S.D0], np.float32)
    return (costs == 0) & (planes.view(np.uint32) == e.view(np.uint32)).all(-1)


def _state(disparity, c_plain, seeds=S.SEEDS):
    planes, exact = S.seeded_field(disparity, seeds)
    costs = np.where(exact, 0.0, c_plain).astype(np.float32)
    return planes, exact, costs


def test_propagation_footprint(lib, fields):
    """REFINE_ITER, near-miss prior with single exact pixels (strong_lib.SEEDS: the centre, (2, 2),
    (W - 3, H - 4), both colours, all four borders); one black and one red launch. The pixels whose
    cost comes out exactly 0 are those the integer restatement of the eight regions
    (APD.cu:1137-1314: far lines at 3, 5, ..., 23, near V-shapes of three levels, every bound),
    composed black then red, says take over an exact plane. Two quirks decide near the borders: an
    invalid region's row of cost_array stays at the zeros of `= {2.0f}` (only [0][0] is 2.0,
    APD.cu:1120) and FindMinCostIndex's `<=` lets the last minimum win (APD.cu:60-71), so a zero row
    after the exact region's row blocks the adoption. (2, 2) sees every plane at cost 2 (its centre
    leaves the source): its view gets no weight, its cost turns NaN, its plane stays, and a NaN at a
    scan's first position is never replaced."""
    c_exact, c_near, _ = fields
    arr, _ = S.footprint_problem(S.NEAR_DISP, A.REFINE_ITER)
    planes, exact, costs = _state(S.NEAR_DISP, c_near)
    p2, got, _, _ = sweep(lib, arr, planes, costs)
    want, unsure = S.zero_footprint(costs, exact, c_exact, c_near)
    assert not unsure[:, S.X_LO + 1:].any()
    assert 150 < want.sum() < H * W // 2
    assert np.array_equal(_zero_set(p2, got), want), np.argwhere(_zero_set(p2, got) != want)[:10]
    assert np.isnan(got[2, 2])


# ------------------------------------------------------------------------------------------------
# b. region argmin and ties, APD.cu:1145, 1221 (strict `<`: the first position of the scan stays)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first_holds_exact", [True, False])
def test_region_scan_keeps_first_of_equal_costs(lib, fields, first_holds_exact):
    """Two positions of one region with the same lowest cost, only one of them holding the exact
    plane: the pixel adopts it only when it is the first in scan order. A far region (up_far of
    (30, 30): (30, 27) before (30, 25)) and a near region (left_near of (50, 30): (49, 30) before
    (48, 29))."""
    c_exact, c_near, _ = fields
    arr, _ = S.footprint_problem(S.NEAR_DISP, A.REFINE_ITER)
    pairs = {(30, 30): [(30, 27), (30, 25)], (50, 30): [(49, 30), (48, 29)]}
    planes, exact, costs = _state(S.NEAR_DISP, c_near, seeds=[p[0 if first_holds_exact else 1] for p in pairs.values()])
    for p in pairs.values():
        for (x, y) in p:
            costs[y, x] = 1e-3
    p2, got, _, _ = sweep(lib, arr, planes, costs, colours=(0,))
    for (x, y) in pairs:
        assert (got[y, x] == 0) == first_holds_exact
    want, _ = S.zero_footprint(costs, exact, c_exact, c_near, colours=(0,))
    assert np.array_equal(_zero_set(p2, got), want)


# ------------------------------------------------------------------------------------------------
# c. REFINE_INIT, APD.cu:1414, 1430-1435
# ------------------------------------------------------------------------------------------------
def test_refine_init_keeps_planes_under_a_cost_of_0_1(lib, fields):
    """REFINE_INIT writes the new plane only if its cost is below the initial cost - 0.1. On the
    near-miss field (every initial cost < 0.1) nothing can be: every plane stays bit for bit, next to
    the exact pixels too, and costs is the initial cost (float32 sums of 15 x cost / 15; tolerance
    ncc_tolerance, about 4e-5)."""
    c_exact, c_near, _ = fields
    arr, _ = S.footprint_problem(S.NEAR_DISP, A.REFINE_INIT)
    planes, exact, costs = _state(S.NEAR_DISP, c_near)
    p2, got, _, _ = sweep(lib, arr, planes, costs)
    assert np.array_equal(p2.view(np.uint32), planes.view(np.uint32))
    m = np.ones((H, W), bool)
    m[:, :S.X_LO + 1] = False
    own = np.where(exact, c_exact, c_near)
    assert np.abs(got[m] - own[m]).max() <= ncc_tolerance(S.NEAR_DISP)


@pytest.mark.parametrize("colour", [0, 1])
def test_refine_init_adopts_the_footprint_on_a_far_miss_field(lib, fields, colour):
    """Far-miss field (initial costs about 0.7, all above 0.1): an exact plane beats cost - 0.1, so one
    launch adopts exactly the footprint of the regions, except at pixels with three or more
    candidates above 1.2, whose only view gets weight 0 (APD.cu:1350-1360): the restatement leaves
    them out by the same rule, and the test skips the pixels whose candidate cost is within 1e-3 of 1.2."""
    c_exact, _, c_far = fields
    arr, _ = S.footprint_problem(S.FAR_DISP, A.REFINE_INIT)
    planes, exact, costs = _state(S.FAR_DISP, c_far)
    p2, got, _, _ = sweep(lib, arr, planes, costs, colours=(colour,))
    want, unsure = S.zero_footprint(costs, exact, c_exact, c_far, colours=(colour,), refine_init=True)
    assert unsure.sum() < 10 and want.sum() > 60
    assert np.array_equal(_zero_set(p2, got) & ~unsure, want & ~unsure)


# ------------------------------------------------------------------------------------------------
# d. RandomInitialization's cost and selected views, APD.cu:723-774
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("top_k", [1, 2, 3, 4])
def test_initial_cost_and_selected_views(lib, top_k):
    """Four sources: two see the d0 plane at cost 0, one at the near-miss cost, one (constant image)
    at the invalid cost 2. The cost is the mean of the min(top_k, valid) smallest costs and the mask
    every view whose cost is <= the last of them: both zero-cost views already for top_k = 1;
    top_k = 4 exceeds the three valid views; columns 0..3 have no valid view (cost 2, mask 0), column
    4 loses the near-miss view. Tolerance: ncc_tolerance / top_k."""
    arr, cv = S.init_problem(top_k)
    costs, sel = np.zeros((H, W), np.float32), np.zeros((H, W), np.uint32)
    stage(lib, arr, 4, sel=sel, costs=costs, planes=None)
    want = [[S.initial_cost_and_views(cv[y, x], top_k) for x in range(W)] for y in range(H)]
    wc = np.array([[w[0] for w in r] for r in want])
    wm = np.array([[w[1] for w in r] for r in want], np.uint32)
    assert np.array_equal(sel, wm)
    assert np.abs(costs - wc).max() <= ncc_tolerance(S.NEAR_DISP)
    assert (wm[:, :4] == 0).all() and (costs[:, :4] == 2).all() and (costs[:, 5:] < 0.1).all()
    assert (wm[:, 5:] == (3 if top_k < 3 else 7)).all() and (wm[:, 4] == 3).all()


def test_initial_cost_all_views_invalid(lib):
    arr, cv = S.init_problem(4, kinds=("flat", "flat"))
    costs, sel = np.zeros((H, W), np.float32), np.ones((H, W), np.uint32)
    stage(lib, arr, 4, sel=sel, costs=costs)
    assert (costs == 2).all() and (sel == 0).all()


# ------------------------------------------------------------------------------------------------
# staged run == full run
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["first_tiny", "refine_init_apd_small", "first_n3_odd"])
def test_staged_run_with_finish_equals_full_run(lib, name):
    orun = lambda arr: oracle_lib.run(lib, arr)
    arr = cases.make_case(name, orun)
    full = oracle_lib.run(lib, arr)
    staged = oracle_lib.run_staged(lib, arr, arr.params.max_iterations, do_finish=True)
    assert all(v == 0 for v in cases.compare(full, staged).values())
    wc = int(full.weak_count[0])
    assert int(staged.weak_count[0]) == wc and np.array_equal(full.anchors[:wc], staged.anchors[:wc])
    # and the stages compose: the state after i iterations differs from the one after i + 1
    a, b = oracle_lib.run_staged(lib, arr, 0), oracle_lib.run_staged(lib, arr, 1)
    assert cases.compare(a, b)["planes"] > 0 and (a.view_weights == 0).all()


# ------------------------------------------------------------------------------------------------
# e. view selection, APD.cu:1323-1374 and TransformPDFToCDF, APD.cu:174-188
# ------------------------------------------------------------------------------------------------
def _within(vw_view, P_view, mask, sigmas=4.5):
    """Sum of a view's weights over `mask` against 15 sum P, within `sigmas` binomial deviations
    sqrt(15 sum P (1 - P)) (each weight is Binomial(15, P): 15 independent draws against the CDF)."""
    got = float(vw_view[mask].sum())
    want = 15.0 * float(P_view[mask].sum())
    sd = np.sqrt(15.0 * float((P_view[mask] * (1 - P_view[mask])).sum()))
    return abs(got - want) <= sigmas * sd + 1e-9, got, want, sd


@pytest.mark.parametrize("pattern,p0", [("all", 0.9), ("rows", 0.5)])
def test_view_selection_priors(lib, pattern, p0):
    """Two identical sources, every plane exact: every pair of candidate costs is equal, so the two
    sampling probabilities are in the ratio of the priors, 0.9 per near neighbour whose selected views
    hold the view and 0.1 otherwise (APD.cu:1325-1337). Neighbours all holding view 0 only: (3.6, 0.4),
    p = 0.9. Red rows alternating between view 0 only and view 1 only: every black pixel has two
    neighbours of each kind, (2.0, 2.0), p = 0.5. Over the >= 1000 black pixels with four neighbours
    (x >= 5): every pixel's weights sum to 15, and the mean weight of view 0 is within 4.5 sigma of
    15 p, sigma = sqrt(15 p (1 - p) / n)."""
    _, src = S.images()
    arr = S.problem([src, src], state=A.REFINE_ITER)
    planes = S.plane_field(float(S.SHIFT))
    ys, xs = np.mgrid[0:H, 0:W]
    sel = np.where(ys % 2 == 0, 1, 2).astype(np.uint32) if pattern == "rows" else np.ones((H, W), np.uint32)
    _, _, _, vw = sweep(lib, arr, planes, np.zeros((H, W), np.float32), sel=sel, colours=(0,))
    m = ((xs + ys) % 2 == 0) & (xs >= 5) & (xs <= W - 2) & (ys >= 1) & (ys <= H - 2)
    n = int(m.sum())
    assert n >= 1000
    assert (vw.sum(0)[m] == 15).all()
    sigma = np.sqrt(15 * p0 * (1 - p0) / n)
    assert abs(vw[0][m].mean() - 15 * p0) <= 4.5 * sigma
    # the same through the general restatement, all black pixels with a valid view
    cv = np.stack([S.field_costs()[0]] * 2, -1)
    P, _ = S.launch_view_probabilities(cv, sel, 0, 0)
    mb = ((xs + ys) % 2 == 0) & (xs >= S.X_LO)
    ok, got, want, sd = _within(vw[0], P[..., 0], mb)
    assert ok, (got, want, sd)


@pytest.mark.parametrize("it", [0, 2])
@pytest.mark.parametrize("colour", [0, 1])
def test_view_selection_thresholds(lib, it, colour):
    """Views (exact copy, graded source), every plane exact, every neighbour holding both views: view
    0's candidate costs are 0, view 1's the pixel's own cost c under the graded source, which spans
    0.03 .. 1.5. Deterministic: with three or more costs above 1.2 view 1 gets weight 0 and view 0 all
    15 (APD.cu:1350-1360). Statistical, by groups of pixels, each within 4.5 sigma of the rule's
    expectation: c under the threshold 0.8 exp(-iter^2 / 90) (probability exp(-c^2 / 0.18), iter 0 and
    2: 0.8 and 0.7652); c within 0.05 under and within 0.05 above it (a cost just either side); c above
    it up to 1.2 (the fallback exp(-thr^2 / 0.32)); border pixels with exactly three zero rows and c
    above the threshold (count > 2 holds through the zero rows alone). For each wrong restatement of a
    constant the pixels whose probability it changes by more than 0.05 form a group on which the
    wrong expectation must FAIL, so the groups are known to discriminate. Pixels with c within 2e-3 of
    a threshold are left out."""
    ref, src = S.images()
    g = S.graded_source()
    arr = S.problem([src, g], state=A.REFINE_ITER)
    planes = S.plane_field(float(S.SHIFT))
    sel = np.full((H, W), 3, np.uint32)
    _, _, _, vw = sweep(lib, arr, planes, np.zeros((H, W), np.float32), sel=sel, colours=(colour,), it=it)
    cv = np.stack([S.field_costs()[0], S.ncc_shift(ref, g, float(S.SHIFT))], -1)
    P, unsure = S.launch_view_probabilities(cv, sel, colour, it)
    ys, xs = np.mgrid[0:H, 0:W]
    m = ((xs + ys) % 2 == colour) & (xs >= S.X_LO) & ~unsure
    c, thr = cv[..., 1], S.cost_threshold(it)
    assert (vw.sum(0)[m] == 15).all()
    dead = m & (P[..., 1] == 0)
    assert dead.sum() > 100 and (vw[1][dead] == 0).all() and (vw[0][dead] == 15).all()
    groups = {"under": m & (c < thr), "just under": m & (c < thr) & (c > thr - 0.05),
              "just above": m & (c >= thr) & (c < thr + 0.05), "fallback": m & (c >= thr) & (c <= 1.2)}
    for name, gm in groups.items():
        assert gm.sum() >= 25, name
        ok, got, want, sd = _within(vw[1], P[..., 1], gm)
        assert ok, (name, got, want, sd)
    wrong = {"count > 3": dict(count_gt=3), "0.9 exp": dict(thr0=0.9), "above 1.0": dict(hi=1.0),
             "priors swapped": None}
    for name, rule in wrong.items():
        if rule is None:  # needs unequal priors: view 0 held by every neighbour, view 1 by none
            sel1 = np.ones((H, W), np.uint32)
            _, _, _, vw1 = sweep(lib, arr, planes, np.zeros((H, W), np.float32), sel=sel1, colours=(colour,), it=it)
            Pt, _ = S.launch_view_probabilities(cv, sel1, colour, it)
            Pw, _ = S.launch_view_probabilities(cv, sel1, colour, it, swap_priors=True)
        else:
            vw1, Pt = vw, P
            Pw, _ = S.launch_view_probabilities(cv, sel, colour, it, **rule)
        gm = m & (np.abs(Pw[..., 1] - Pt[..., 1]) > 0.05)
        assert gm.sum() >= 2, name
        ok, got, want, sd = _within(vw1[1], Pt[..., 1], gm)
        assert ok, (name, got, want, sd)
        bad, *_ = _within(vw1[1], Pw[..., 1], gm)
        assert not bad, f"the group of '{name}' does not tell the rule from its wrong restatement"


def test_view_selection_counts_the_2_of_an_invalid_up_near_row(lib):
    """`cost_array[8][32] = {2.0f}` (APD.cu:1120) leaves 2.0 in row 0, view 0 only; every other entry
    of an invalid region's row is 0 and counts as a cost under the threshold. At (61, 0) and (62, 0)
    up_near, up_far and right_far are invalid: view 0 has the 2.0 and two zeros, so with its five real
    costs between the threshold and 1.2 (the graded source as view 0) only two costs are under the
    threshold and it falls back to exp(-thr^2 / 0.32); with a zero in [0][0] it would have three and
    the probability 1. Eight RNG seeds x both colours give 16 pixel runs of 15 samples: the weight of
    view 0 summed over them is within 4.5 sigma of the rule's expectation and NOT within 4.5 sigma of
    the expectation with [0][0] = 0."""
    ref, src = S.images()
    g = S.graded_source()
    arr = S.problem([g, src], state=A.REFINE_ITER)
    sel = np.full((H, W), 3, np.uint32)
    cv = np.stack([S.ncc_shift(ref, g, float(S.SHIFT)), S.field_costs()[0]], -1)
    ys, xs = np.mgrid[0:H, 0:W]
    got = want = var = wrong = wvar = 0.0
    for colour in (0, 1):
        P, unsure = S.launch_view_probabilities(cv, sel, colour, 0)
        Pw, _ = S.launch_view_probabilities(cv, sel, colour, 0, row0_value=0.0)
        m = ((xs + ys) % 2 == colour) & (xs >= S.X_LO) & ~unsure & (np.abs(Pw[..., 0] - P[..., 0]) > 0.05)
        assert m.sum() >= 1 and (ys[m] == 0).all()
        for seed in range(1, 9):
            arr.seed = seed
            _, _, _, vw = sweep(lib, arr, S.plane_field(float(S.SHIFT)), np.zeros((H, W), np.float32), sel=sel,
                                colours=(colour,))
            assert (vw.sum(0)[m] == 15).all()
            got += float(vw[0][m].sum())
            want += 15 * float(P[..., 0][m].sum())
            var += 15 * float((P[..., 0][m] * (1 - P[..., 0][m])).sum())
            wrong += 15 * float(Pw[..., 0][m].sum())
            wvar += 15 * float((Pw[..., 0][m] * (1 - Pw[..., 0][m])).sum())
    assert abs(got - want) <= 4.5 * np.sqrt(var), (got, want, var)
    assert abs(got - wrong) > 4.5 * np.sqrt(wvar), (got, wrong, wvar)


def test_view_selection_three_costs_above_1_2_kill_the_view(lib):
    """count_false < 3 (APD.cu:1354-1357), one view: the exact plane everywhere except a plane at depth
    depth_min (disparity 64: its centre leaves the source, cost exactly 2) at single red pixels, whose
    state cost 0 makes every region that holds one hand it on. (30, 20) has three such regions (its
    up, down and left neighbours): three costs above 1.2, no weight, NaN cost. (40, 30) has two (up,
    down): all 15 samples, and it keeps the exact plane at cost 0."""
    _, src = S.images()
    arr = S.problem([src], state=A.REFINE_ITER)
    planes = S.plane_field(float(S.SHIFT))
    costs = np.full((H, W), 0.5, np.float32)
    for (x, y) in [(30, 19), (30, 21), (29, 20), (40, 29), (40, 31)]:
        planes[y, x, 3] = np.float32(S.DMIN)
        costs[y, x] = 0.0
    p2, got, _, vw = sweep(lib, arr, planes, costs, colours=(0,))
    assert vw[0, 20, 30] == 0 and np.isnan(got[20, 30])
    assert vw[0, 30, 40] == 15 and got[30, 40] == 0 and p2[30, 40, 3] == np.float32(S.D0)


# ------------------------------------------------------------------------------------------------
# f. refinement candidates, APD.cu:961-980 with GenerateRandomNormal / GeneratePerturbedNormal,
#    APD.cu:242-305
# ------------------------------------------------------------------------------------------------
def test_refinement_candidates(lib):
    """The five (depth, normal) pairs over 2000 (pixel, seed) pairs: (random depth, current normal),
    (current depth, random normal), (the same random depth and normal), (current depth, perturbed
    normal), (perturbed depth, current normal) (APD.cu:979-980). The random depth lies in [depth_min,
    depth_max] (APD.cu:968); the perturbed depth within +-2 % of the current one (APD.cu:961, 971-974),
    and the draws fill that range; every normal has unit length and faces the camera (n . view
    direction < 0, APD.cu:259-266, 299-303). Perturbation bound: the rotation is a product of three
    axis rotations by angles (u - 0.5) * 0.02 pi, |angle| <= 0.01 pi each (APD.cu:274-294, 976); the
    angle of a product of rotations is at most the sum of their angles, and a rotation moves no vector
    by more than its angle: the perturbed normal lies within 0.03 pi of the current one."""
    _, src = S.images()
    arr = S.problem([src])
    pb = arr.build()
    rng = np.random.default_rng(11)
    d5, n20 = np.zeros(5, np.float32), np.zeros(20, np.float32)
    rel, ang, rd = [], [], []
    for _ in range(2000):
        px, py = int(rng.integers(0, W)), int(rng.integers(0, H))
        vd = np.array([(px - W / 2) / S.F, (py - H / 2) / S.F, 1.0])
        vd /= np.linalg.norm(vd)
        n = rng.normal(size=3)
        n /= np.linalg.norm(n)
        if n @ vd > -0.2:
            n = -n if n @ vd > 0.2 else -vd
        depth = float(rng.uniform(1.0, 15.0))
        cur = np.array([*n, -(n @ (vd * depth / vd[2]))], np.float32)
        assert lib.oracle_refine_candidates(C.byref(pb), px, py, int(rng.integers(1, 2 ** 62)), S.fptr(cur), S.fptr(d5),
                                            S.fptr(n20)) == 0
        nn = n20.reshape(5, 4)[:, :3]
        assert d5[0] == d5[2] and S.DMIN <= d5[0] <= S.DMAX
        assert d5[1] == d5[3] and abs(d5[1] - depth) <= 2e-5 * depth
        assert np.array_equal(nn[0], cur[:3]) and np.array_equal(nn[4], cur[:3]) and np.array_equal(nn[1], nn[2])
        assert abs(d5[4] / d5[1] - 1) <= 0.02 + 1e-6
        for k in (1, 3):
            assert abs(np.linalg.norm(nn[k].astype(np.float64)) - 1) < 1e-5 and nn[k].astype(np.float64) @ vd < 0
        cosang = np.clip(nn[3].astype(np.float64) @ cur[:3].astype(np.float64), -1, 1)
        ang.append(np.arccos(cosang))
        rel.append(d5[4] / d5[1] - 1)
        rd.append(d5[0])
    assert max(ang) <= 0.03 * np.pi + 1e-3
    assert max(ang) > 0.008 * np.pi                     # ... and the perturbation is not a smaller one
    assert max(rel) > 0.019 and min(rel) < -0.019       # the +-2 % range is filled
    assert min(rd) < S.DMIN + 0.3 and max(rd) > S.DMAX - 0.3


# ------------------------------------------------------------------------------------------------
# g. ComputeGeomConsistencyCost, APD.cu:865-902
# ------------------------------------------------------------------------------------------------
def _geom(lib, arr, px, py, depth):
    pb = arr.build()
    pl = np.array([0, 0, -1, depth], np.float32)
    return lib.oracle_geom_cost(C.byref(pb), px, py, 1, S.fptr(pl))


def test_geom_cost_known_values(lib):
    """Source depth map = the true fronto-parallel plane at d0: a hypothesis at depth d' reprojects
    f b |1 / d' - 1 / d0| pixels away (1.333, 0.571, 0.444, 1.333 for d' = 6, 7, 9, 12), capped at 3
    (d' = 2 gives 12). A hole (depth 0) costs exactly 3. The source depth is read at the truncated
    pixel (APD.cu:885): over a one-texel step edge between columns 30 and 31 (depths 3.2 | 4.0), the
    hypotheses projecting to x = 30.75 and 31.25 read different sides (0.75 px each; rounding would
    give 1.25 for the first). Tolerance: four times the largest float32 - float64 difference of the
    restated chain over these inputs (about 1e-5)."""
    _, src = S.images()
    arr = S.problem([src], geom_consistency=1)
    px, py = 40, 20
    flat = np.full((H, W), S.D0, np.float32)
    step = np.where(np.arange(W)[None, :] <= 30, 3.2, 4.0).astype(np.float32) * np.ones((H, 1), np.float32)
    probes = [(flat, d) for d in (6.0, 7.0, 9.0, 12.0, 2.0, 8.0)] + [(step, 32.0 / 9.25), (step, 32.0 / 8.75)]
    tol = 4 * max(abs(S.geom_cost(px, py, d, m, dtype=np.float32) - S.geom_cost(px, py, d, m)) for m, d in probes)
    assert 0 < tol < 1e-4
    for m, d in probes:
        arr.depths = [flat, m]
        want = S.geom_cost(px, py, d, m)
        if m is flat:
            assert abs(want - min(3.0, S.F * S.B * abs(1 / d - 1 / S.D0))) < 1e-12
        assert abs(_geom(lib, arr, px, py, d) - want) <= tol, (d, want)
    assert S.geom_cost(px, py, 2.0, flat) == 3.0 and _geom(lib, arr, px, py, 2.0) == 3.0
    assert abs(S.geom_cost(px, py, 32.0 / 9.25, step) - 0.75) < 1e-6  # (3.2 is not a float32)
    assert abs(S.geom_cost(px, py, 32.0 / 9.25, step, pick=lambda v: int(round(v))) - 1.25) < 1e-6
    arr.depths = [flat, np.zeros((H, W), np.float32)]
    for d in (2.0, 7.0, 8.0):
        assert _geom(lib, arr, px, py, d) == 3.0


@pytest.mark.parametrize("impetus", [1, 0])
def test_sweep_adds_geom_factor_times_geom_cost(lib, fields, impetus):
    """use_impetus in the sweep (APD.cu:1406-1411, 990-995): with a source depth map of holes every
    plane's geometric cost is 3, so the exact plane costs 0 + geom_factor * 3 = 0.6 at a pixel that
    keeps its own cost. The propagated rows carry no geometric term (APD.cu:1388-1397), so a pixel
    with all eight regions valid takes a neighbour's (equal) plane at that row's 0; in columns
    x >= W - 3 the invalid right_far row is the last minimum (FindMinCostIndex, `<=`), nothing is
    taken and the cost is 0.6 (float32: fma(0.2f, 3, 0) * 15 / 15, within 1e-6). Without use_impetus
    it is 0 there too."""
    _, src = S.images()
    arr = S.problem([src], state=A.REFINE_ITER, geom_consistency=1, use_impetus=impetus, geom_factor=0.2)
    arr.depths = [np.full((H, W), S.D0, np.float32), np.zeros((H, W), np.float32)]
    planes = S.plane_field(float(S.SHIFT))
    _, got, _, _ = sweep(lib, arr, planes, np.zeros((H, W), np.float32))
    assert (got[3:H - 3, S.X_LO + 3:W - 3] == 0).all()
    edge = got[:, W - 3:]
    assert np.abs(edge - (0.6 if impetus else 0.0)).max() <= 1e-6


# ------------------------------------------------------------------------------------------------
# h. RANSACToGetFitPlane, APD.cu:2486-2598
# ------------------------------------------------------------------------------------------------
def _plane_through(pts, n, w, dtype):
    """The reference's plane through three pixels on the plane (n, w) (APD.cu:2518-2563): depth from
    the plane hypothesis (APD.cu:237-240), the 3D points (APD.cu:197-202), the cross product of A - C
    and B - C, normalised, w = -(normal . A); here turned to nz < 0."""
    t = dtype
    f, cx, cy = t(S.F), t(W / 2.0), t(H / 2.0)
    n = [t(v) for v in n]
    w = t(w)
    X = []
    for (x, y) in pts:
        d = -w * f / ((t(x) - cx) * n[0] + (f / f) * (t(y) - cy) * n[1] + f * n[2])
        X.append(np.array([d * (t(x) - cx) / f, d * (t(y) - cy) / f, d], dtype))
    a, b = X[0] - X[2], X[1] - X[2]
    cr = np.array([a[1] * b[2] - b[1] * a[2], -(a[0] * b[2] - b[0] * a[2]), a[0] * b[1] - b[0] * a[1]], dtype)
    cr = cr / np.sqrt((cr * cr).sum(dtype=dtype))
    out = np.array([*cr, -(cr * X[0]).sum(dtype=dtype)], dtype)
    return (-out if out[2] > 0 else out).astype(np.float64)


def test_ransac_fit_plane(lib):
    """Anchors on one slanted plane: the fit plane of a WEAK pixel inside their triangles is that
    plane, turned to face the camera (APD.cu:2582-2591), whatever triple the RANSAC drew -- for eight
    anchors on a ring and for exactly three (strong_count < 3 is the limit, APD.cu:2525). Fewer than
    three anchors keep the pixel's own plane; a pixel outside every anchor triangle gets the zero
    plane (APD.cu:2544, 2595-2596); a pixel that is not WEAK copies its plane (APD.cu:2497-2499).
    Tolerance: four times the largest float32 - float64 difference of the restated construction over
    all anchor triples of the test that contain their pixel (about 2e-5)."""
    import itertools
    _, src = S.images()
    arr = S.problem([src])
    n = np.array([0.2, -0.1, -1.0])
    n /= np.linalg.norm(n)
    w = float(-(n @ np.array([0.0, 0.0, S.D0])))
    planes = np.zeros((H, W, 4), np.float32)
    planes[...] = np.array([*n, w], np.float32)
    own = np.array([0, 0, -1, 5.0], np.float32)
    ring = [(8, 0), (6, 6), (0, 8), (-6, 6), (-8, 0), (-6, -6), (0, -8), (6, -6)]
    pix = {}  # pixel -> up to 8 anchors
    for (x, y) in [(12 + 6 * k, 12 + (5 * k) % 24) for k in range(8)]:
        pix[(x, y)] = [(x + dx, y + dy) for dx, dy in ring]
    pix[(56, 12)] = [(56, 4), (50, 18), (62, 18)]            # exactly three, around the pixel
    pix[(56, 36)] = [(56, 30), (50, 40)]                     # two: too few
    pix[(10, 40)] = [(22 + dx, 41 + dy // 2) for dx, dy in ring]  # all to the right, none collinear: no triangle holds it
    weak = np.full((H, W), A.STRONG, np.uint8)
    for (x, y) in pix:
        weak[y, x] = A.WEAK
        planes[y, x] = own
    order = sorted(pix, key=lambda p: p[1] * W + p[0])
    anchors = np.full((len(order), 9, 2), -1, np.int16)
    for i, p in enumerate(order):
        anchors[i, 0] = p
        for k, a in enumerate(pix[p]):
            anchors[i, 1 + k] = a
    fit = np.zeros((H, W, 4), np.float32)
    stage(lib, arr, 6, it=0, planes=planes, weak=weak, anchors=anchors, fit=fit)

    def inside(tri, p):
        (ax, ay), (bx, by), (cx, cy) = tri
        t1 = (ax - p[0]) * (by - p[1]) - (ay - p[1]) * (bx - p[0])
        t2 = (bx - p[0]) * (cy - p[1]) - (by - p[1]) * (cx - p[0])
        t3 = (cx - p[0]) * (ay - p[1]) - (cy - p[1]) * (ax - p[0])
        return t1 * t2 >= 0 and t1 * t3 >= 0

    truth = np.array([*n, w])
    tol, fitted = 0.0, 0
    for p, anc in pix.items():
        tris = [t for t in itertools.permutations(anc, 3) if inside(t, p)] if len(anc) >= 3 else []
        got = fit[p[1], p[0]].astype(np.float64)
        if len(anc) < 3:
            assert np.array_equal(fit[p[1], p[0]], own)
        elif not tris:
            assert (got == 0).all()
        else:
            tol = max(tol, 4 * max(np.abs(_plane_through(t, n, w, np.float32) - _plane_through(t, n, w, np.float64)).max()
                                   for t in tris))
            fitted += 1
    assert fitted == 9 and 0 < tol < 2e-4
    for p, anc in pix.items():
        if len(anc) >= 3 and p != (10, 40):
            got = fit[p[1], p[0]].astype(np.float64)
            assert np.abs(got - truth).max() <= tol, (p, got, truth)
            vd = np.array([(p[0] - W / 2) / S.F, (p[1] - H / 2) / S.F, 1.0])
            assert got[:3] @ vd < 0
    m = weak != A.WEAK
    assert np.array_equal(fit[m].view(np.uint32), planes[m].view(np.uint32))


# ------------------------------------------------------------------------------------------------
# i. LocalRefine, APD.cu:2346-2432
# ------------------------------------------------------------------------------------------------
def _local_refine_np(disp0):
    """Expected disparity after LocalRefine of a fronto-parallel field at disparity disp0, one
    selected view (baseline b): cost_now at disp0; samples at disp0 - 5 .. disp0 + 5 whose depth
    f b / disparity lies in [depth_min, depth_max], the first strictly lowest below 2.0 wins
    (APD.cu:2404-2428); the depth moves there iff cost_now - min_cost > 0.1 (APD.cu:2429). Also the
    pixels float64 cannot decide (margin 1e-3 on the 0.1, 1e-4 between the two best samples)."""
    ref, src = S.images()
    now = S.ncc_shift(ref, src, disp0)
    best_c = np.full((H, W), 2.0)
    second = np.full((H, W), 2.0)
    best_d = np.full((H, W), float(disp0))
    for pd in range(-5, 6):
        d = disp0 + pd
        if d <= 0 or not (S.DMIN <= S.F * S.B / d <= S.DMAX):
            continue
        c = S.ncc_shift(ref, src, d)
        better = c < best_c
        second = np.where(better, best_c, np.minimum(second, c))
        best_d = np.where(better, d, best_d)
        best_c = np.where(better, c, best_c)
    move = now - best_c > 0.1
    unsure = (np.abs(now - best_c - 0.1) < 1e-3) | (move & (second - best_c < 1e-4))
    return np.where(move, best_d, disp0), move, unsure


@pytest.mark.parametrize("disp0", [4.0, 4.5, 7.0, 9.0, 10.0])
def test_local_refine(lib, disp0):
    """Fields at disparity 4 (the exact plane: nothing is better by 0.1, every depth stays bit for
    bit), 4.5 (cost < 0.1: stays), 7 and 9 (the exact disparity 4 is one of the 11 samples: every
    pixel with x >= 4 moves to depth 8, a strictly better sample) and 10 (4 is out of the +-5 reach:
    the best of disparities 5..15, if better by 0.1). Pixels with no selected view or no view weight
    stay (APD.cu:2375, 2394). Moved depths match f b / disparity to 2e-6 relative (float32 division)."""
    _, src = S.images()
    arr = S.problem([src], state=A.REFINE_ITER)
    planes = S.plane_field(disp0)
    p0 = planes.copy()
    sel = np.ones((H, W), np.uint32)
    vw = np.full((1, H, W), 15, np.uint8)
    sel[10:14, 20:24] = 0
    vw[0, 30:34, 40:44] = 0
    stage(lib, arr, 7, sel=sel, planes=planes, vw=vw)
    want, move, unsure = _local_refine_np(disp0)
    off = (sel == 0) | (vw[0] == 0)
    assert np.array_equal(planes[off].view(np.uint32), p0[off].view(np.uint32))
    assert np.array_equal(planes[..., :3], p0[..., :3])
    ok = ~off & ~unsure
    stay = ok & ~move
    assert np.array_equal(planes[..., 3][stay].view(np.uint32), p0[..., 3][stay].view(np.uint32))
    mv = ok & move
    wd = S.F * S.B / want
    assert (np.abs(planes[..., 3][mv] - wd[mv]) <= 2e-6 * wd[mv] + 1e-6).all()
    assert unsure.sum() < 60
    if disp0 in (4.0, 4.5):
        assert not move[:, S.X_LO + 1:].any()
    if disp0 in (7.0, 9.0):
        zone = ok & (np.arange(W)[None, :] >= int(disp0))
        assert move[zone].all() and (want[zone] == 4.0).all() and (planes[..., 3][zone] != p0[..., 3][zone]).all()
    if disp0 == 10.0:
        assert 100 < mv.sum() and (want[mv] >= 5.0).all()
