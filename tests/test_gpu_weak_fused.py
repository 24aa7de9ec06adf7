"""The anchor candidates' centre windows inside the Weak sweep (k_sweep_weak_vm's phase P1').

With APD_CAND_CENTRE_IN_SWEEP=1 k_weak_cand_comb leaves the focal term of every (WEAK pixel, candidate,
view) in the candidates' cost buffer, k_weak_cand_g is not launched, and the sweep evaluates the
candidates' centre windows itself and finishes the costs in place. The default keeps the centre
windows in k_weak_cand_g (the fused sweep measured slower at the headline shape). Both
must equal the oracle bit for bit, as every path does (tolerance: none, see test_gpu_parity.py), and
each other array for array. The switch must also hold under the switches it composes with: the
per-colour launches (costs by WEAK index), the costs by WEAK index under the single launch, the 8x8
list order, and APD_NO_CAND_PAIRS=1 (no pair table: the sweep's full P1, no P1').

Shapes: test_gpu_weak_dense.py's -- 96x72 and 101x67 (partial list tiles, a last group with
count % 64 != 0) at N = 4, 64x48 at N = 1 (8 tasks over 4 waves, 64 pixels per wave in P2a), 96x72 at
N = 8, SA labels with a label-0 band (filtered centre windows, unused anchor 0), fewer than 64 WEAK
pixels -- and cases.py's headline-parameter case at N = 10 (80 tasks, P2a packs 6 pixels per wave and
leaves 4 lanes over). Between them the cases hold WEAK pixels with none, some and all of their 8
candidates (checked on the oracle's anchors without a GPU).
"""
import functools

import numpy as np
import pytest

import apd_abi as A
import cases
import oracle_lib
from test_gpu_weak_dense import dense_case, run_fresh

DENSE = ["apd_geom_96x72_n4", "apd_geom_101x67_n4", "apd_geom_64x48_n1", "apd_geom_96x72_n8",
         "apd_geom_sa_96x72_n4", "few_weak_96x72_n4"]
HEADLINE = "refine_iter_eth3d_final_n10"
FUSED_CASES = DENSE + [HEADLINE]


@functools.lru_cache(maxsize=None)
def fused_case(name):
    """(problem, oracle result) of a case; computed once and shared by the tests (never modified)."""
    if name != HEADLINE:
        return dense_case(name)
    oracle = oracle_lib.load()
    orun = lambda arr: oracle_lib.run(oracle, arr)
    arr = cases.make_case(name, orun)
    return arr, orun(arr)


def assert_equals_oracle(name, got):
    arr, ref = fused_case(name)
    diffs = cases.compare(ref, got)
    assert all(v == 0 for v in diffs.values()), f"{name}: differing elements {diffs}"
    wc = int(ref.weak_count[0])
    assert int(got.weak_count[0]) == wc
    assert np.array_equal(ref.anchors[:wc], got.anchors[:wc])


def candidate_counts(name):
    """Per WEAK pixel, how many of its 8 anchor candidates exist (anchor h + 1 present and STRONG)."""
    arr, ref = fused_case(name)
    wc = int(ref.weak_count[0])
    anc = ref.anchors[:wc].astype(np.int64)
    valid = (anc[..., 0] >= 0) & (anc[..., 1] >= 0)
    state = arr.weak_info[np.clip(anc[..., 1], 0, arr.height - 1), np.clip(anc[..., 0], 0, arr.width - 1)]
    return (valid[:, 1:] & (state[:, 1:] == A.STRONG)).sum(axis=1)


def test_cases_cover_what_they_claim():
    """The shapes and candidate sets P1' has to get right are in the cases (CPU)."""
    none = some = full = 0
    for name in FUSED_CASES:
        arr, ref = fused_case(name)
        wc = int(ref.weak_count[0])
        assert wc > 0 and wc == int((arr.weak_info == A.WEAK).sum()), name
        assert int((ref.weak_info == A.WEAK).sum()) > 0, name
        nc = candidate_counts(name)
        none += int((nc == 0).sum())
        some += int(((nc > 0) & (nc < 8)).sum())
        full += int((nc == 8).sum())
    assert int(fused_case("apd_geom_101x67_n4")[1].weak_count[0]) % 64 != 0  # a partial last group
    assert 0 < int(fused_case("few_weak_96x72_n4")[1].weak_count[0]) < 64
    arr = fused_case(HEADLINE)[0]
    assert len(arr.images) - 1 == 10 and 64 // 10 == 6 and 64 % 10 == 4
    assert len(fused_case("apd_geom_64x48_n1")[0].images) - 1 == 1
    sa = fused_case("apd_geom_sa_96x72_n4")[0]
    yy, xx = np.nonzero(sa.weak_info == A.WEAK)
    lab = sa.sa_mask[yy, xx]
    assert (lab == 0).any() and (lab != 0).any()  # filtered and unfiltered centre windows
    assert none > 0, "no WEAK pixel without any anchor candidate"
    assert some > 0, "no WEAK pixel with some but not all of its 8 anchor candidates"
    assert full > 0, "no WEAK pixel with all 8 anchor candidates"


SWITCH = "APD_CAND_CENTRE_IN_SWEEP"


@pytest.mark.gpu
@pytest.mark.parametrize("name", FUSED_CASES)
def test_centre_windows_in_sweep_bit_exact(name, monkeypatch):
    monkeypatch.setenv(SWITCH, "1")
    assert_equals_oracle(name, run_fresh(fused_case(name)[0]))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["apd_geom_101x67_n4", "apd_geom_sa_96x72_n4"])
def test_centre_windows_in_sweep_equal_default(name, monkeypatch):
    arr = fused_case(name)[0]
    default = run_fresh(arr)
    monkeypatch.setenv(SWITCH, "1")
    fused = run_fresh(arr)
    for f in ("planes", "costs", "selected_views", "view_weights", "weak_info"):
        x, y = getattr(default, f), getattr(fused, f)
        assert np.array_equal(x.view(np.uint32) if x.dtype.kind == "f" else x,
                              y.view(np.uint32) if y.dtype.kind == "f" else y), f"{name}: {f} differs"
    assert_equals_oracle(name, default)


@pytest.mark.gpu
@pytest.mark.parametrize("var", ["APD_WEAK_PER_COLOUR", "APD_NO_CAND_GROUP_MAJOR", "APD_WEAK_QUAD", "APD_NO_CAND_PAIRS"])
def test_centre_windows_in_sweep_under_switches(var, monkeypatch):
    monkeypatch.setenv(SWITCH, "1")
    monkeypatch.setenv(var, "1")
    name = "apd_geom_101x67_n4"
    assert_equals_oracle(name, run_fresh(fused_case(name)[0]))
