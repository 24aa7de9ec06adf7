"""The Weak sweep's single launch per iteration over the dense two-colour WEAK list.

The default path (one k_sweep_weak_vm launch over the tile-ordered list of both colours, the candidates'
costs laid out by that list's 64-entry groups) must equal the oracle bit for bit, as every path does
(tolerance: none, see test_gpu_parity.py); APD_WEAK_PER_COLOUR=1 (a launch per checkerboard colour over
the per-colour lists, costs by WEAK index) must equal the default array for array. The single launch
rests on one invariant, checked here on the oracle's anchors without a GPU: anchors 1..8 of a WEAK
pixel are STRONG pixels (anchor 0 is the pixel itself), so no workgroup of the sweep reads what another
writes.

Shapes: the smallest that still take every path -- 96x72 (several list tiles and 64-entry groups),
101x67 (sides that are no multiple of the 16x16 list tile: partial tiles, a last group with
count % 64 != 0), N = 1 and N = 8 (P2a's share_p switches at N >= 8; N = 1 packs 64 pixels per wave),
SA labels, a WEAK count below one group, and a WEAK set of one colour only.
"""
import functools

import numpy as np
import pytest

import apd_abi as A
import cases
import oracle_lib

# name: (w, h, scene views, n_src, SA, edit of the input WEAK mask)
DENSE_CASES = {
    "apd_geom_96x72_n4": (96, 72, 4, 4, False, None),
    "apd_geom_101x67_n4": (101, 67, 4, 4, False, None),
    "apd_geom_64x48_n1": (64, 48, 4, 1, False, None),
    "apd_geom_96x72_n8": (96, 72, 8, 8, False, None),
    "apd_geom_sa_96x72_n4": (96, 72, 4, 4, "zero_band", None),
    "few_weak_96x72_n4": (96, 72, 4, 4, False, "few"),
    "one_colour_96x72_n4": (96, 72, 4, 4, False, "black"),
}
FEW = 40  # WEAK pixels the "few" edit keeps (< 64: one partial group)


@functools.lru_cache(maxsize=None)
def _oracle():
    return oracle_lib.load()


@functools.lru_cache(maxsize=None)
def _priors(w, h, views, n):
    orun = lambda arr: oracle_lib.run(_oracle(), arr)
    return cases.first_pass(orun, cases.scene(w, h, views), n)


@functools.lru_cache(maxsize=None)
def dense_case(name):
    """(problem, oracle result) of a case; computed once and shared by the tests (never modified)."""
    w, h, views, n, sa, edit = DENSE_CASES[name]
    sc = cases.scene(w, h, views)
    arr = cases.refine_problem(sc, _priors(w, h, views, n), 0, n, state=A.REFINE_ITER, geom=True, apd=True, sa=sa)
    if edit:
        # WEAK pixels taken out of the WEAK set become STRONG (they keep their prior planes)
        weak = arr.weak_info.copy()
        yy, xx = np.nonzero(weak == A.WEAK)
        drop = np.arange(yy.size) >= FEW if edit == "few" else ((xx + yy) & 1) == 1
        weak[yy[drop], xx[drop]] = A.STRONG
        arr.weak_info = weak
    return arr, oracle_lib.run(_oracle(), arr)


def run_hip(eng, arr):
    eng.set_problem(arr)
    eng.run()
    return eng.results(A.Outputs(arr.width, arr.height, len(arr.images) - 1, max_weak=arr.width * arr.height))


def run_fresh(arr):
    """A run on a context of its own (the switches are read when a context is created)."""
    lib = A.load_library()
    if lib.apd_device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    eng = A.Engine(0, lib)
    try:
        return run_hip(eng, arr)
    finally:
        eng.close()


def assert_equals_oracle(name, got):
    arr, ref = dense_case(name)
    diffs = cases.compare(ref, got)
    assert all(v == 0 for v in diffs.values()), f"{name}: differing elements {diffs}"
    wc = int(ref.weak_count[0])
    assert int(got.weak_count[0]) == wc
    assert np.array_equal(ref.anchors[:wc], got.anchors[:wc])


def weak_pixels(arr):
    return np.nonzero(arr.weak_info == A.WEAK)


def test_cases_cover_what_they_claim():
    """The edited WEAK masks and the odd shape are what the cases are for (CPU)."""
    for name in DENSE_CASES:
        arr, ref = dense_case(name)
        yy, xx = weak_pixels(arr)
        assert yy.size > 0, name
        assert int(ref.weak_count[0]) == yy.size, name
        # WEAK pixels survive the pass in the swept rows, so the sweep has work
        assert int((ref.weak_info == A.WEAK).sum()) > 0, name
    yy, xx = weak_pixels(dense_case("few_weak_96x72_n4")[0])
    assert 0 < yy.size < 64
    yy, xx = weak_pixels(dense_case("one_colour_96x72_n4")[0])
    assert yy.size >= 64 and (((xx + yy) & 1) == 0).all()
    for name in ("apd_geom_96x72_n4", "apd_geom_101x67_n4"):
        yy, xx = weak_pixels(dense_case(name)[0])
        assert (((xx + yy) & 1) == 0).sum() >= 64 and (((xx + yy) & 1) == 1).sum() >= 64, name
    yy, xx = weak_pixels(dense_case("apd_geom_101x67_n4")[0])
    assert yy.size % 64 != 0 and 101 % 16 != 0 and 67 % 16 != 0


@pytest.mark.parametrize("name", list(DENSE_CASES))
def test_no_anchor_is_weak(name):
    """Anchors 1..8 of every WEAK pixel are STRONG pixels of the input state (anchor 0 is the pixel
    itself): the one-launch Weak sweep reads plane and selection at them only, and writes WEAK pixels only."""
    arr, ref = dense_case(name)
    wc = int(ref.weak_count[0])
    anc = ref.anchors[:wc].astype(np.int64)
    valid = (anc[..., 0] >= 0) & (anc[..., 1] >= 0)
    assert valid[:, 1:].any(), f"{name}: no anchors at all"
    state = arr.weak_info[np.clip(anc[..., 1], 0, arr.height - 1), np.clip(anc[..., 0], 0, arr.width - 1)]
    k18 = valid[:, 1:]
    assert (state[:, 1:][k18] != A.WEAK).all(), f"{name}: {(state[:, 1:][k18] == A.WEAK).sum()} WEAK anchors"
    assert (state[:, 1:][k18] == A.STRONG).all(), f"{name}: anchors that are not STRONG"
    # anchor 0: the pixel (raster order of the WEAK pixels, APD.cpp:627-640)
    yy, xx = weak_pixels(arr)
    assert valid[:, 0].all() and np.array_equal(anc[:, 0, 0], xx) and np.array_equal(anc[:, 0, 1], yy)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(DENSE_CASES))
def test_dense_one_launch_bit_exact(name):
    assert_equals_oracle(name, run_fresh(dense_case(name)[0]))


@pytest.mark.gpu
def test_dense_candidates_in_sweep_bit_exact(monkeypatch):
    """APD_NO_CAND_PAIRS=1: the single launch evaluates the anchor candidates itself (no pair table)."""
    monkeypatch.setenv("APD_NO_CAND_PAIRS", "1")
    name = "apd_geom_101x67_n4"
    assert_equals_oracle(name, run_fresh(dense_case(name)[0]))


@pytest.mark.gpu
@pytest.mark.parametrize("var", ["APD_NO_CAND_GROUP_MAJOR", "APD_WEAK_QUAD"])
def test_dense_layout_switches_bit_exact(var, monkeypatch):
    """The candidates' costs by WEAK index under the single launch, and the 8x8-block list order."""
    monkeypatch.setenv(var, "1")
    name = "apd_geom_101x67_n4"
    assert_equals_oracle(name, run_fresh(dense_case(name)[0]))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["apd_geom_101x67_n4", "apd_geom_sa_96x72_n4"])
def test_per_colour_switch_equals_default(name, monkeypatch):
    arr = dense_case(name)[0]
    default = run_fresh(arr)
    monkeypatch.setenv("APD_WEAK_PER_COLOUR", "1")
    per_colour = run_fresh(arr)
    for f in ("planes", "costs", "selected_views", "view_weights", "weak_info"):
        x, y = getattr(default, f), getattr(per_colour, f)
        assert np.array_equal(x.view(np.uint32) if x.dtype.kind == "f" else x,
                              y.view(np.uint32) if y.dtype.kind == "f" else y), f"{name}: {f} differs"
    assert_equals_oracle(name, per_colour)
