"""GPU: the HIP engine's state between its stages, against the oracle stopped at the same point, and
the Strong-half known-answer problems (tests/test_oracle_kat_strong.py) on the engine.

The other GPU parity tests compare after apd_stage_finish only, where the filter, DepthToWeak and
LocalRefine have rewritten planes and costs. apd_get_results copies the live buffers and waits for
the stream, so the state after RandomInitialization and after every sweep iteration is readable: it
must equal oracle_run_staged bit for bit. Mid-run planes are in the sweep's form on both sides
(reference-frame normal, distance to the origin).

No field is exempt: the engine holds planes, costs, selected views (RandomInitialization's snapshot
is copied over them at the end of apd_stage_prepare), view weights (view-major, as the outputs) and
pixel states in the buffers apd_get_results reads; its tile-ordered side buffers (kept initial costs,
anchor candidates' costs) are not outputs.
"""
import numpy as np
import pytest

import apd_abi as A
import cases
import oracle_lib
import strong_lib as S
from strong_lib import H, W

pytestmark = pytest.mark.gpu

FIELDS = ("planes", "costs", "selected_views", "view_weights", "weak_info")


@pytest.fixture(scope="module")
def oracle():
    return oracle_lib.load()


@pytest.fixture(scope="module")
def engine():
    lib = A.load_library()
    if lib.apd_device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    eng = A.Engine(0, lib)
    yield eng
    eng.close()


def read(engine, arr):
    return engine.results(A.Outputs(arr.width, arr.height, len(arr.images) - 1))


def assert_equal(ref, got, what):
    diffs = cases.compare(ref, got, FIELDS)
    assert all(v == 0 for v in diffs.values()), f"{what}: differing elements {diffs}"


@pytest.mark.parametrize("name", ["first_tiny", "first_n3_odd", "refine_init_apd_small", "refine_iter_geom_sa0",
                                  "refine_iter_apd_geom_rt4"])
def test_staged_bit_exact(name, oracle, engine):
    """After apd_stage_prepare and after each of three apd_stage_iteration calls: planes, costs,
    selected views, view weights and pixel states equal the oracle's at the same point."""
    orun = lambda arr: oracle_lib.run(oracle, arr)
    arr = cases.make_case(name, orun)
    arr.params.max_iterations = 3
    engine.set_problem(arr)
    engine.prepare()
    assert_equal(oracle_lib.run_staged(oracle, arr, 0), read(engine, arr), f"{name} after prepare")
    for i in range(3):
        engine.iteration(i)
        assert_equal(oracle_lib.run_staged(oracle, arr, i + 1), read(engine, arr), f"{name} after iteration {i}")


def run_kat(engine, oracle, arr):
    """prepare + iteration(0) on the engine, each read back and equal to the oracle's stage."""
    engine.set_problem(arr)
    engine.prepare()
    a = read(engine, arr)
    assert_equal(oracle_lib.run_staged(oracle, arr, 0), a, "after prepare")
    engine.iteration(0)
    b = read(engine, arr)
    assert_equal(oracle_lib.run_staged(oracle, arr, 1), b, "after iteration 0")
    return a, b


def zero_set(out):
    e = np.array([0, 0, -1, S.D0], np.float32)
    return (out.costs == 0) & (out.planes.view(np.uint32) == e.view(np.uint32)).all(-1)


def test_kat_propagation_footprint(oracle, engine):
    """test_oracle_kat_strong.test_propagation_footprint as an ordinary problem: the near-miss prior
    with exact single pixels; RandomInitialization gives them cost exactly 0 (2.0 at (2, 2), whose
    centre leaves the source), and after one iteration the pixels that hold the exact plane at cost 0
    are those the restatement of the regions says, from the costs read back after prepare."""
    arr, exact = S.footprint_problem(S.NEAR_DISP, A.REFINE_ITER)
    c_exact, c_near = S.field_costs(S.NEAR_DISP)
    a, b = run_kat(engine, oracle, arr)
    seeds0 = exact & (a.costs == 0)
    assert seeds0.sum() == len(S.SEEDS) - 1 and a.costs[2, 2] == 2
    want, unsure = S.zero_footprint(a.costs, exact, c_exact, c_near)
    assert not unsure[:, S.X_LO + 1:].any() and want.sum() > 150
    assert np.array_equal(zero_set(b), want)
    assert np.isnan(b.costs[2, 2])


def test_kat_refine_init(oracle, engine):
    """REFINE_INIT on the near-miss field: every plane stays (initial costs < 0.1). On the far-miss
    field the black pixels (swept first, left alone by the red launch) adopt the footprint of the
    exact pixels."""
    arr, exact = S.footprint_problem(S.NEAR_DISP, A.REFINE_INIT)
    a, b = run_kat(engine, oracle, arr)
    assert np.array_equal(a.planes.view(np.uint32), b.planes.view(np.uint32))
    arr, exact = S.footprint_problem(S.FAR_DISP, A.REFINE_INIT)
    c_exact, c_far = S.field_costs(S.FAR_DISP)
    a, b = run_kat(engine, oracle, arr)
    want, unsure = S.zero_footprint(a.costs, exact, c_exact, c_far, colours=(0,), refine_init=True)
    ys, xs = np.mgrid[0:H, 0:W]
    black = ((xs + ys) % 2 == 0) & ~unsure
    assert (want & black).sum() > 60
    assert np.array_equal(zero_set(b) & black, want & black)


@pytest.mark.parametrize("top_k", [1, 2, 3, 4])
def test_kat_initial_cost_and_views(top_k, oracle, engine):
    """RandomInitialization with exact ties between views (two at cost exactly 0), an invalid view
    and columns with no valid view at all: costs and masks as the restatement says; the sweep over
    them equals the oracle's (weight sums of 0, NaN costs included)."""
    arr, cv = S.init_problem(top_k)
    a, _ = run_kat(engine, oracle, arr)
    want = [[S.initial_cost_and_views(cv[y, x], top_k) for x in range(W)] for y in range(H)]
    assert np.array_equal(a.selected_views, np.array([[w[1] for w in r] for r in want], np.uint32))
    assert np.abs(a.costs - np.array([[w[0] for w in r] for r in want])).max() <= S.ncc_tolerance(S.NEAR_DISP)
    assert (a.costs[:, :4] == 2).all() and (a.selected_views[:, :4] == 0).all()


def test_kat_all_views_invalid(oracle, engine):
    arr, _ = S.init_problem(4, kinds=("flat", "flat"))
    a, b = run_kat(engine, oracle, arr)
    assert (a.costs == 2).all() and (a.selected_views == 0).all()
    assert (b.view_weights == 0).all() and np.isnan(b.costs).all()


def test_kat_view_selection_dead_views(oracle, engine):
    """Views (exact copy, graded source): on the black pixels (first launch: every candidate is still
    the exact plane) a view with three or more costs above 1.2 gets weight 0 and the other all 15."""
    ref, src = S.images()
    g = S.graded_source()
    arr = S.problem([src, g], state=A.REFINE_ITER)
    arr.init_planes = S.plane_field(float(S.SHIFT))
    a, b = run_kat(engine, oracle, arr)
    cv = np.stack([S.field_costs()[0], S.ncc_shift(ref, g, float(S.SHIFT))], -1)
    P, unsure = S.launch_view_probabilities(cv, a.selected_views, 0, 0)
    ys, xs = np.mgrid[0:H, 0:W]
    m = ((xs + ys) % 2 == 0) & (xs >= S.X_LO) & ~unsure
    dead = m & (P[..., 1] == 0)
    assert dead.sum() > 100
    assert (b.view_weights[1][dead] == 0).all() and (b.view_weights[0][dead] == 15).all()
    assert (b.view_weights.sum(0)[m] == 15).all()
