"""Float64 known answers for the fusion oracle (oracle/fusion_oracle.c), CPU only.

The oracle is the checker of every GPU fusion test; here it is held to tests/fusion_ref.py, a float64
restatement written from APD.cpp, on the constructed problems of tests/fusion_kat_lib.py: rotated
cameras (R != R^T), non-zero t, fx != fy, cx != cy, one K[1] != 0, and column blocks that put every
rule on both sides of its cut. Every decision of these problems is farther from its cut than the
float32 error bound (test_construction_is_guarded), so the comparison is exact in every decision
(source pixels, skip maps, accepted set, order, TAT skip counts) and within the bound in every value.
tools/mutate_oracle.py (FUSION_MUTATIONS) checks that these tests reject wrong restatements.
"""
import numpy as np
import pytest

import fusion_kat_lib as KL
import fusion_lib as FL
import fusion_ref as FR

NAMES = list(KL.PROBLEMS)
RUNS = [(n, run) for n in NAMES for run in KL.PROBLEMS[n][1]]


@pytest.mark.parametrize("name", NAMES)
def test_construction_is_guarded(name):
    views, res, g = KL.problem(name)
    print(f"{name}: {g.total} decisions, {len(g.bad)} unguarded")
    assert g.total > 1000
    assert len(g.bad) == 0, g.bad[:5]
    for v in views:
        H, W = v["depth"].shape
        assert 16 <= W <= 48 and 12 <= H <= 36
    assert 2 <= len(views) <= 6


def _both(g, name, least=3):
    lo, hi = g.cov.get(name, [0, 0])
    assert lo >= least and hi >= least, f"{name}: {lo} false / {hi} true decisions"


def test_rules_on_both_sides():
    """Each cut is met from both sides by guarded decisions (the counts are the restatement's)."""
    _, _, g = KL.problem("geom")
    for rule in ("dist<2", "rel<0.01", "angle<0.1745", "sum>factor*n", "round in (-1,0)", "occl"):
        _both(g, rule)
    _, _, g = KL.problem("filter")
    for rule in ("view>80", "occl", "round in (-1,0)"):
        _both(g, rule)
    _, _, g = KL.problem("behind")
    _both(g, "proj<=0")
    _, _, g = KL.problem("tat")
    for rule in ("dist<k/4", "rel<k*base", "angle<k*grad+base"):
        _both(g, rule)
    for name in ("filter", "counts"):
        views, res, g = KL.problem(name)
        _both(g, "view>80")
        r = res[(0, True)]
        strong = np.concatenate([np.array(x) for x in r["strong"]])
        weak = np.concatenate([np.array(x) for x in r["weak"]])
        for arr, cut in ((strong, 2), (weak, 4)):  # the counters reach the threshold, and stop one short of it
            assert (arr == cut - 1).sum() >= 1 and (arr == cut).sum() >= 1, (cut, np.bincount(arr))
        assert ((weak >= 4) & (strong < 2)).sum() >= 1  # a pixel flagged by the WEAK count alone
        assert ((strong >= 2) & (weak < 4)).sum() >= 1


def test_cache_and_masks_matter():
    """The problems depend on the rules that only show over several pixels: the carried TAT cache,
    and the masks written by accepted pixels."""
    views, res, _ = KL.problem("tat")
    for variant in (1, 2):
        alt = FR.fuse(views, variant, False, reset_tat_cache=True, scene=res[(variant, False)]["scene"])
        assert abs(len(alt["order"]) - len(res[(variant, False)]["order"])) >= 10
    for name, run in (("geom", (0, False)), ("index", (0, False))):
        views, res, _ = KL.problem(name)
        assert sum(m.count(1) for m in res[run]["masks"]) > 20


@pytest.mark.parametrize("name", NAMES)
def test_oracle_candidates(name):
    """Source pixels exactly; dist / rel / angle / q within the bound."""
    views, _res, _g = KL.problem(name)
    sc = FR.Scene(views)
    g = FR.Guards()
    for ref in range(len(views)):
        src = list(range(len(views)))
        exp = FR.candidates(sc, ref, src, g)
        sp, dist, rel, ang, q = FL.oracle_candidates(views, ref, src)
        assert np.array_equal(sp, exp["sp"]), f"view {ref}: source pixels differ at {np.argwhere(sp != exp['sp'])[:3]}"
        live = exp["sp"] >= 0
        for got, key in ((dist, "dist"), (rel, "rel"), (ang, "angle"), (q, "q")):
            err = np.abs(got.astype(np.float64) - exp[key])[live]
            bound = exp["e_" + key][live]
            ok = (err <= bound) | ~np.isfinite(exp[key][live])
            assert ok.all(), f"view {ref} {key}: off by {err[~ok].max()} (bound {bound[~ok].max()})"
    assert not g.bad


@pytest.mark.parametrize("name", ["geom", "filter", "counts", "behind"])
def test_oracle_weak_filter(name):
    views, res, _g = KL.problem(name)
    r = [x for run, x in res.items() if run[1]][0]
    for i in range(len(views)):
        got = FL.oracle_weak_filter(views, i)
        exp = np.array(r["skips"][i], np.uint8).reshape(got.shape)
        assert np.array_equal(got, exp), f"view {i}: {np.argwhere(got != exp)[:4]}"
        assert not np.any(got[views[i]["weak"] != 0])
    if name == "behind":  # one STRONG occlusion and the view behind: flagged only if `proj_depth <= 0` were let through
        assert sum(sum(s) for s in r["skips"]) == 0 and sum(x.count(1) for x in r["strong"]) >= 8
    else:
        assert sum(sum(s) for s in r["skips"]) >= 4


@pytest.mark.parametrize("name,run", RUNS, ids=[f"{n}-{KL.DATASETS[r[0]]}-{'filter' if r[1] else 'nofilter'}"
                                                for n, r in RUNS])
def test_oracle_fusion(name, run):
    views, res, _g = KL.problem(name)
    xyz, _col = KL.check_oracle_fusion(views, run[0], run[1], res[run])
    assert len(xyz) >= 8


def test_nan_reference_depth_is_processed():
    """`ref_depth <= 0.0` is false for NaN: in the TAT variants the carried cache then decides the
    pixel, and a point with NaN coordinates is emitted."""
    views, res, _g = KL.problem("tat")
    holes = [(0, 0) + tuple(rc) for rc in np.argwhere(np.isnan(views[0]["depth"]))]
    for variant in (1, 2):
        r = res[(variant, False)]
        hit = [r["order"].index(h) for h in holes if h in r["order"]]
        assert hit and len(hit) < len(holes)  # some are accepted from the cache, some are not
        xyz, _, _, _ = FL.run_oracle(views, KL.DATASETS[variant], False)
        assert np.isnan(xyz[hit]).all() and np.isnan(xyz).any(axis=1).sum() == len(hit)
