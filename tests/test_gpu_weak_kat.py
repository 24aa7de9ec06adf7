"""GPU: the Weak-sweep known-answer problems (tests/test_oracle_kat_weak.py, tests/weak_lib.py) on the
HIP engine, as ordinary use_APD inputs.

The other GPU tests of the Weak path compare k_sweep_weak_vm with the oracle's k_sweep_weak only. Here
each run (prepare, then iteration 0, through test_gpu_staged_parity.run_kat) is bit-equal to
oracle_run_staged at both points AND itself satisfies the answer derived from CheckerboardPropagation-
Weak (weak_lib.check_ring_run), computed from the anchors, states and costs read back after prepare:
WEAK blocks inside hand-built rings of STRONG pixels that hold the exact plane. Where all eight
anchors are present the pixel adopts anchor 8's plane at cost exactly 0, bit for bit, and
selected_views is the mask of the views drawn; where the six-point rings leave the last anchors
missing, the zero row of `cost_array[8][32] = {2.0f}` is the last minimum, blocks the adoption and
selected_views stays untouched (with identical sources the mask drawn equals the initial one, so one
case adds a second source that is the negative image: selected at first, never drawn, and the value
written, 1, differs from the value kept, 3); REFINE_INIT keeps every plane of the near-miss field; a
problem without a usable view ends in NaN costs.

64 x 48; one, two and three sources; 54, 72 and 90 WEAK pixels (a partial group of the dense list, and a
group boundary); both colours and black pixels only; one case on the moved rig (rotated world,
fy != fx, Ks != Kr).
"""
import numpy as np
import pytest

import apd_abi as A
import oracle_lib
import strong_lib as S
import weak_lib as Wk
from strong_lib import H, W
from test_gpu_staged_parity import assert_equal

pytestmark = pytest.mark.gpu


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


def run_kat(engine, oracle, arr):
    """test_gpu_staged_parity.run_kat, reading the anchors back too."""
    read = lambda: engine.results(A.Outputs(W, H, len(arr.images) - 1, max_weak=H * W))
    engine.set_problem(arr)
    engine.prepare()
    a = read()
    ref = oracle_lib.run_staged(oracle, arr, 0)
    assert_equal(ref, a, "after prepare")
    wc = int(ref.weak_count[0])
    assert int(a.weak_count[0]) == wc and np.array_equal(a.anchors[:wc], ref.anchors[:wc])
    engine.iteration(0)
    b = read()
    assert_equal(oracle_lib.run_staged(oracle, arr, 1), b, "after iteration 0")
    return a, b


@pytest.mark.parametrize("name", [c[0] for c in Wk.RING_CASES])
def test_kat_ring_problem(name, oracle, engine):
    arr, asked, n, refine_init = Wk.ring_case(name)
    a, b = run_kat(engine, oracle, arr)
    adopted, blocked = Wk.check_ring_run(a, b, asked, n, refine_init)
    assert adopted >= 10 and blocked >= 5, (adopted, blocked)
    swept = a.weak_info == A.WEAK
    if name == "n2_negative_view":  # a blocked pixel keeps 3, an adopting one writes 1
        assert (a.selected_views[swept] == 3).all() and (b.view_weights[1][swept] == 0).all()
        assert sorted(np.unique(b.selected_views[swept])) == [1, 3]
    assert int(swept.sum()) == Wk.RING_WEAK[name]  # every WEAK pixel asked for kept its state
    ys, xs = np.nonzero(swept)
    assert {int(v) for v in (xs + ys) % 2} == ({0} if "one_colour" in name else {0, 1})


def test_kat_dense_list_sizes():
    """The cases cover a dense list of fewer than 64 WEAK pixels and of 65 or more."""
    counts = [int(Wk.ring_case(c[0])[1].sum()) for c in Wk.RING_CASES]
    assert counts == [Wk.RING_WEAK[c[0]] for c in Wk.RING_CASES] and min(counts) < 64 and max(counts) >= 65


def test_kat_no_view(oracle, engine):
    """One constant source: every cost is 2 and no view is ever drawn: NaN costs, planes unchanged."""
    arr, asked = Wk.ring_problem(1, A.REFINE_ITER, (1, 1), srcs=[np.full((H, W), 90.0, np.float32)])
    a, b = run_kat(engine, oracle, arr)
    m = a.weak_info == A.WEAK
    assert m.sum() >= 30 and (a.costs == 2).all()
    assert np.isnan(b.costs[m]).all() and (b.view_weights[:, m] == 0).all()
    assert np.array_equal(b.planes[m].view(np.uint32), a.planes[m].view(np.uint32))
    assert np.array_equal(b.selected_views[m], a.selected_views[m])
