"""The geometric tail of the Weak sweep's exact early exit (k_sweep_weak_vm, geometric passes).

In a geometric pass the sweep computes the geometric terms of the fit plane and of the five refinement
candidates for all weighted views before it samples a window (pre-passes before P3 and after P4), and
the early exit continues its prefix chain over the views still to come with fmaf(gf, g_v, 0.0f), an
exact lower bound of each view's cost. A slot it flags would have been rejected anyway, so every
result must stay what it was: equal to the oracle bit for bit (tolerance: none, see
test_gpu_parity.py) and equal to the path without the tail (APD_NO_GEOM_TAIL=1) array for array. The
terms live in the workgroup's own entries of the anchor candidates' cost buffer, so the path must hold
under every layout of that buffer (per-colour launches, costs by WEAK index, the 8x8 list order, the
centre windows finished in place by P1') and fall back without it (APD_NO_CAND_PAIRS=1). In a
non-geometric pass it must be inert. That it does something is read from the profiling counters: the
sweep issues strictly fewer windows and NCC-New evaluations with the tail.

Shapes: test_gpu_weak_dense.py's (partial last group, N = 1 -- the tail is empty after the first
fold --, N = 8, SA labels, fewer than 64 WEAK pixels) and cases.py's headline-parameter case (gf 0.2,
N = 10: three P3 batches and several P5 batches).
"""
import functools

import numpy as np
import pytest

import apd_abi as A
import cases
import oracle_lib
from test_gpu_weak_dense import run_fresh
from test_gpu_weak_fused import DENSE, HEADLINE, fused_case

NON_GEOM = "refine_init_apd"  # APD without geometric consistency (cases.py)
GEOM_CASES = DENSE + [HEADLINE]
SWITCH = "APD_NO_GEOM_TAIL"
ARRAYS = ("planes", "costs", "selected_views", "view_weights", "weak_info")


@functools.lru_cache(maxsize=None)
def tail_case(name):
    """(problem, oracle result) of a case; computed once and shared by the tests (never modified)."""
    if name != NON_GEOM:
        return fused_case(name)
    oracle = oracle_lib.load()
    orun = lambda arr: oracle_lib.run(oracle, arr)
    arr = cases.make_case(name, orun)
    return arr, orun(arr)


def assert_equals_oracle(name, got):
    arr, ref = tail_case(name)
    diffs = cases.compare(ref, got)
    assert all(v == 0 for v in diffs.values()), f"{name}: differing elements {diffs}"
    wc = int(ref.weak_count[0])
    assert int(got.weak_count[0]) == wc
    assert np.array_equal(ref.anchors[:wc], got.anchors[:wc])


def assert_same_arrays(name, x, y):
    for f in ARRAYS:
        u, w = getattr(x, f), getattr(y, f)
        assert np.array_equal(u.view(np.uint32) if u.dtype.kind == "f" else u,
                              w.view(np.uint32) if w.dtype.kind == "f" else w), f"{name}: {f} differs"


def run_counted(arr):
    """A profiled run on a context of its own -> the profiling counters."""
    lib = A.load_library()
    if lib.apd_device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    eng = A.Engine(0, lib)
    try:
        eng.set_problem(arr)
        eng.profile_reset(True)
        eng.run()
        return [int(c) for c in eng.profile_counters()]
    finally:
        eng.close()


def test_cases_cover_what_they_claim():
    """Refining WEAK pixels, geometric consistency where named, N = 1, 4, 8 and 10 (CPU)."""
    ns = set()
    for name in GEOM_CASES:
        arr, ref = tail_case(name)
        assert arr.params.geom_consistency == 1 and arr.params.use_APD == 1, name
        assert arr.params.geom_factor > 0, name
        wc = int(ref.weak_count[0])
        assert wc > 0 and wc == int((arr.weak_info == A.WEAK).sum()), name
        # refining pixels: WEAK pixels whose plane the pass changed (fit plane or refinement candidate
        # accepted, or an anchor hypothesis) and that are still WEAK afterwards
        yy, xx = np.nonzero((arr.weak_info == A.WEAK) & (ref.weak_info == A.WEAK))
        assert yy.size > 0, name
        moved = (ref.planes[yy, xx].view(np.uint32) != arr.init_planes[yy, xx].view(np.uint32)).any(axis=1)
        assert moved.any(), f"{name}: no WEAK pixel changed its plane"
        ns.add(len(arr.images) - 1)
    assert ns == {1, 4, 8, 10}
    arr, ref = tail_case(NON_GEOM)
    assert arr.params.geom_consistency == 0 and arr.params.use_APD == 1
    assert int(ref.weak_count[0]) > 0
    assert int(tail_case("apd_geom_101x67_n4")[1].weak_count[0]) % 64 != 0  # a partial last group
    assert 0 < int(tail_case("few_weak_96x72_n4")[1].weak_count[0]) < 64
    head = tail_case(HEADLINE)[0]
    assert abs(head.params.geom_factor - 0.2) < 1e-6 and len(head.images) - 1 == 10
    sa = tail_case("apd_geom_sa_96x72_n4")[0]
    assert sa.sa_mask is not None and (sa.sa_mask != 0).any()


@pytest.mark.gpu
@pytest.mark.parametrize("name", GEOM_CASES + [NON_GEOM])
def test_geom_tail_bit_exact(name):
    assert_equals_oracle(name, run_fresh(tail_case(name)[0]))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["apd_geom_101x67_n4", HEADLINE])
def test_geom_tail_equals_path_without(name, monkeypatch):
    arr = tail_case(name)[0]
    default = run_fresh(arr)
    monkeypatch.setenv(SWITCH, "1")
    without = run_fresh(arr)
    assert_same_arrays(name, default, without)
    assert_equals_oracle(name, without)


@pytest.mark.gpu
@pytest.mark.parametrize("var", ["APD_WEAK_PER_COLOUR", "APD_NO_CAND_GROUP_MAJOR", "APD_WEAK_QUAD", "APD_NO_CAND_PAIRS",
                                 "APD_CAND_CENTRE_IN_SWEEP"])
def test_geom_tail_under_switches(var, monkeypatch):
    monkeypatch.setenv(var, "1")
    name = "apd_geom_101x67_n4"
    assert_equals_oracle(name, run_fresh(tail_case(name)[0]))


@pytest.mark.gpu
def test_geom_tail_issues_fewer_windows(monkeypatch):
    """Counters 7 / 8: the sweep's centre / anchor windows; 1: NCC-New evaluations; 2: geometric terms."""
    arr = tail_case(HEADLINE)[0]
    with_tail = run_counted(arr)
    monkeypatch.setenv(SWITCH, "1")
    without = run_counted(arr)
    print(f"counters [1, 2, 7, 8] with the tail {[with_tail[i] for i in (1, 2, 7, 8)]}, "
          f"without {[without[i] for i in (1, 2, 7, 8)]}")
    assert without[7] > 0 and without[8] > 0
    assert with_tail[7] < without[7]
    assert with_tail[8] < without[8]
    assert with_tail[1] < without[1]


@pytest.mark.gpu
def test_geom_tail_inert_without_geometric_consistency(monkeypatch):
    arr = tail_case(NON_GEOM)[0]
    with_tail = run_counted(arr)
    monkeypatch.setenv(SWITCH, "1")
    without = run_counted(arr)
    assert with_tail[7] > 0 and with_tail[1] > 0
    assert with_tail == without, f"with the tail {with_tail}, without {without}"
