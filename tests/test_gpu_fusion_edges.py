"""Fusion on the GPU, where the random scans of tests/test_fusion.py never go.

(a) The device entry points of include/apd_fusion.h against the float64 restatement
    (tests/fusion_ref.py) directly, without the oracle: on the constructed problems of
    tests/fusion_kat_lib.py every decision is guarded, so source pixels, skip flags, levels and the
    consistent / not decision must agree exactly and the values within the float32 bound; on one
    random scan decisions are compared where guarded (at most 1 % of the live candidates are not).
(b) `apd --only_fuse` against the oracle, byte-identical APD.ply and skip.png, on small scans built
    for the branches of the host commit (apde-mvs_amd/host/fusion.cpp) that no other scan reaches.
    Where the branch is a reference quirk (self-source, missing id, repeated id, the carried TAT
    cache) the oracle is also held to the restatement, so a shared misreading cannot pass.
(c) The argument checks of the C ABI.
"""
import ctypes as C
import os

import numpy as np
import pytest
from PIL import Image

import apd_abi as A
import fusion_kat_lib as KL
import fusion_lib as FL
import fusion_ref as FR
import test_fusion as TF

pytestmark = pytest.mark.gpu

AB, AG = np.float32(0.06981317007977318), np.float32(0.05235987755982988)


@pytest.fixture(scope="module")
def hl():
    return FL.hostlib()


@pytest.fixture(scope="module")
def cuts(hl):
    q_k = [1.0, 1.0] + [hl.apdhost_angle_cut_lt(float(np.float32(k) * AG + AB)) for k in range(2, 33)]
    return hl.apdhost_view_cut_deg(80.0), hl.apdhost_angle_cut_lt(float(np.float32(0.174533))), q_k


def _device_against_ref(views, cuts, skips=None, allowed_unguarded=0.0, filter_where_guarded=False):
    """Runs the three entry points for every view over its own source list and compares with the
    restatement. Returns (live candidates, unguarded candidates)."""
    q_view, q_angle, q_k = cuts
    sc = FR.Scene(views)
    eng = A.FusionEngine(0)
    eng.set_views(views)
    n_live = n_bad = 0
    try:
        for i in range(len(views)):
            got = eng.weak_filter(i, q_view)  # (a problem without a filter run has no guarded filter decisions)
            if skips is not None:
                exp = np.array(skips[i], np.uint8).reshape(got.shape)
                assert np.array_equal(got, exp), f"weak filter view {i}: {np.argwhere(got != exp)[:4]}"
            elif filter_where_guarded:  # compare the pixels with no (pixel, source) pair inside its error bound;
                # the pairs of WEAK pixels are this entry point's live candidates and count into the cap
                gf = FR.Guards()
                exp = np.array(FR.weak_vis_filter(sc, i, gf)[0], np.uint8).reshape(got.shape)
                pairs = {(w[1], w[2], w[3]) for _name, w, _v, _c, _b in gf.bad}
                sure_px = np.ones(got.shape, bool)
                for r, c, _s in pairs:
                    sure_px[r, c] = False
                n_live += int((views[i]["weak"] == 0).sum()) * (len(views) - 1)
                n_bad += len(pairs)
                bad = (got != exp) & sure_px
                assert not bad.any(), f"weak filter view {i}: {np.argwhere(bad)[:4]}"
            src = [sc.index_of(s) for s in sc.srcs[i]]
            if not src:
                continue
            g = FR.Guards()
            cand = FR.candidates(sc, i, src, g)
            cons, lv_i, lv_a = FR.decisions(sc, i, src, g)
            H, W = views[i]["depth"].shape
            unsure = np.zeros((H, W, len(src)), bool)  # candidates with a decision inside its error bound
            for _name, where, _v, _c, _b in g.bad:
                unsure[where[1], where[2], [j for j, s in enumerate(src) if s == where[3]]] = True
            live = ~(views[i]["depth"] <= 0)[..., None] & np.ones(len(src), bool)
            n_live += int(live.sum())
            n_bad += int((unsure & live).sum())
            sure = live & ~unsure
            pix, er, qq = eng.consistency(i, src, q_angle)
            exp_pix = np.where(cons, cand["sp"], -1)
            bad = (pix != exp_pix) & sure
            assert not bad.any(), f"consistency view {i}: {int(bad.sum())} differ, first {np.argwhere(bad)[:3]}"
            val = (cand["sp"] >= 0) & sure
            e64 = cand["dist"] + 200.0 * cand["rel"]
            e_b = cand["e_dist"] + 200.0 * cand["e_rel"] + FR.G[2] * np.abs(e64)  # 200 * rel, the sum: two more roundings
            fin = val & np.isfinite(e64)
            assert np.all(np.abs(er.astype(np.float64) - e64)[fin] <= e_b[fin]), f"err + 200 rel, view {i}"
            finq = val & np.isfinite(cand["q"])
            assert np.all(np.abs(qq.astype(np.float64) - cand["q"])[finq] <= cand["e_q"][finq]), f"q, view {i}"
            for tat_i, exp_lv, base in ((True, lv_i, FR.DEPTH_BASE[1]), (False, lv_a, FR.DEPTH_BASE[2])):
                tp, lv = eng.tat_levels(i, src, 0.25, base, q_k if tat_i else None)
                bad = (tp != cand["sp"]) & sure
                assert not bad.any(), f"tat source pixels view {i}: first {np.argwhere(bad)[:3]}"
                bad = (lv != exp_lv) & sure
                assert not bad.any(), f"tat levels view {i} tat_i={tat_i}: {int(bad.sum())} differ {np.argwhere(bad)[:3]}"
    finally:
        eng.close()
    assert n_bad <= allowed_unguarded * n_live, f"{n_bad} of {n_live} live candidates are unguarded"
    return n_live, n_bad


# ------------------------------------------------------------------------------------------------
# (a) device entry points against float64
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(KL.PROBLEMS))
def test_device_matches_float64_on_constructed_problems(name, cuts):
    views, res, _g = KL.problem(name)
    skips = next((r["skips"] for run, r in res.items() if run[1]), None)
    n_live, n_bad = _device_against_ref(views, cuts, skips)
    assert n_live > 500 and n_bad == 0


def test_device_matches_float64_on_a_random_scan(tmp_path, hl, cuts):
    """48x36, 4 views of tests/fusion_lib.make_fusion_scan. Live candidates are the (pixel, source)
    pairs that the three entry points decide: pairs of pixels with depth > 0 (or NaN) for consistency
    and tat_levels, pairs of WEAK pixels for weak_filter. A pair with a decision inside its error
    bound is unguarded and is not compared; at most 1 % of all live candidates may be. Counted by the
    restatement alone at seed 7, noise 0.0004: 93 of 19 893 candidate pairs and 114 of 9 663 filter
    pairs, 0.70 % together. (The filter's share, 1.2 %, cannot go under 1 % on its own at any seed: 3 % of
    this generator's depths are 0, the filter does not test the reference depth, and at depth 0 the
    point is the camera centre, so the view angle is acosf(0/0).)"""
    folder = str(tmp_path / "scan")
    FL.make_fusion_scan(folder, 48, 36, 3, seed=7, noise=0.0004)
    views = FL.load_views(folder, hl)
    assert len(views) == 4
    n_live, n_bad = _device_against_ref(views, cuts, None, allowed_unguarded=0.01, filter_where_guarded=True)
    print(f"random scan: {n_bad} of {n_live} live candidates unguarded")
    assert n_live > 25000


# ------------------------------------------------------------------------------------------------
# (b) the tool on the unreached branches
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def edge_scan(tmp_path_factory, hl):
    made = {}

    def get(name):
        if name not in made:
            folder = str(tmp_path_factory.mktemp(name))
            made[name] = (folder,) + KL.prepare_scan(folder, name, hl)
        return made[name]
    return get


def _tool_against_oracle(folder, views, dataset, weak_filter=True):
    out = TF._run_cli(folder, dataset, weak_filter)
    assert "Fusion done!" in out
    xyz, col, skips, counts = FL.run_oracle(views, dataset, weak_filter)
    got = open(os.path.join(folder, "APD", "APD.ply"), "rb").read()
    if got != FL.ply_bytes(xyz, col):
        head, rec = FL.read_ply(os.path.join(folder, "APD", "APD.ply"))
        pytest.fail(f"APD.ply differs: {len(rec)} points vs {len(xyz)} expected; head {head!r}")
    if weak_filter:
        for v, s in zip(views, skips):
            png = np.asarray(Image.open(os.path.join(folder, "APD", f"{v['ref']:08d}", "skip.png")))
            assert np.array_equal(png, s * 255)
    if dataset == "TaT_a":
        assert [int(ln.split()[-1]) for ln in out.splitlines() if ln.startswith("skip_weak:")] == list(counts)
    return xyz


DATASETS = ["ETH3D", "TaT_i", "TaT_a"]
VARIANT = {"ETH3D": 0, "TaT_i": 1, "TaT_a": 2}


@pytest.mark.parametrize("dataset", DATASETS)
@pytest.mark.parametrize("name", ["self_source", "missing_id", "duplicate_source"])
def test_tool_index_quirks(edge_scan, name, dataset):
    """A view listing itself (the single-chunk fallback of the TAT commit), an id absent from
    pair.txt (view 0: once a self-source, once not), the same id twice. The oracle must also agree
    with the float64 restatement in accepted set and order."""
    folder, views, res = edge_scan(name)
    KL.check_oracle_fusion(views, VARIANT[dataset], True, res[(VARIANT[dataset], True)])
    xyz = _tool_against_oracle(folder, views, dataset)
    assert len(xyz) > 100


@pytest.mark.parametrize("dataset", DATASETS)
def test_tool_three_map_sizes(edge_scan, dataset):
    folder, views, _ = edge_scan("three_sizes")
    assert [v["depth"].shape for v in views] == [(36, 48), (30, 40), (25, 33)]
    assert len(_tool_against_oracle(folder, views, dataset)) > 100


@pytest.mark.parametrize("dataset", DATASETS)
def test_tool_tiny_images(edge_scan, dataset):
    """15x9 (fewer pixels than one block), 64x1 (one row: one chunk) and 20x12 in one scan."""
    folder, views, _ = edge_scan("tiny")
    assert [v["depth"].shape for v in views] == [(9, 15), (1, 64), (12, 20)]
    xyz = _tool_against_oracle(folder, views, dataset)
    assert len(xyz) > (20 if dataset == "ETH3D" else 0)


@pytest.mark.parametrize("dataset", ["ETH3D", "TaT_i", "TaT_a"])
def test_tool_one_source(edge_scan, dataset):
    """N = 1: RunFusion fuses; the TAT variants have no level (k runs from 2 to N) and emit nothing."""
    folder, views, _ = edge_scan("one_source")
    xyz = _tool_against_oracle(folder, views, dataset)
    if dataset == "ETH3D":
        assert len(xyz) > 50
    else:
        assert len(xyz) == 0


@pytest.mark.parametrize("dataset", DATASETS)
def test_tool_max_sources(edge_scan, dataset):
    folder, views, _ = edge_scan("max_sources")
    assert len(views) == 33 and len(views[0]["srcs"]) == A.MAX_IMAGES == 32
    assert len(_tool_against_oracle(folder, views, dataset)) > 100


@pytest.mark.parametrize("dataset", ["TaT_i", "TaT_a"])
def test_tool_carried_tat_cache(edge_scan, dataset):
    """96 rows make 64 row chunks; view 2 is usable only in its top fifth, so the incoming cache of
    most chunks comes from chunks further up. The restatement first shows that the carry decides at
    least 50 points, then the oracle must agree with it and the tool with the oracle."""
    folder, views, res = edge_scan("carry")
    variant = VARIANT[dataset]
    r = res[(variant, False)]
    alt = FR.fuse(views, variant, False, reset_tat_cache=True, scene=r["scene"])
    assert len(r["order"]) - len(alt["order"]) >= 50
    assert views[0]["depth"].shape == (96, 64)
    KL.check_oracle_fusion(views, variant, False, r)
    assert len(_tool_against_oracle(folder, views, dataset, weak_filter=False)) == len(r["order"])


@pytest.mark.parametrize("dataset", DATASETS)
def test_tool_nonfinite_depths(edge_scan, dataset):
    """NaN and +-Inf depths and all-zero normals in reference and source views."""
    folder, views, _ = edge_scan("nonfinite")
    assert sum(int(np.isnan(v["depth"]).sum() + np.isinf(v["depth"]).sum()) for v in views) > 100
    assert len(_tool_against_oracle(folder, views, dataset)) > 100


# ------------------------------------------------------------------------------------------------
# (c) argument checks
# ------------------------------------------------------------------------------------------------
def test_argument_checks():
    views, _res, _g = KL.problem("index")
    eng = A.FusionEngine(0)
    lib, ctx = eng.lib, eng.ctx
    H, W = views[0]["depth"].shape
    pix = np.zeros((H, W, 40), np.int32)
    f1, f2 = np.zeros((H, W, 40), np.float32), np.zeros((H, W, 40), np.float32)
    lv = np.zeros((H, W, 40), np.uint8)
    skip = np.zeros((H, W), np.uint8)

    def cons(ref, src):
        s = np.asarray(src, np.int32)
        return lib.apd_fusion_consistency(ctx, ref, len(s), s.ctypes.data, 0.9, pix.ctypes.data, f1.ctypes.data,
                                          f2.ctypes.data)

    def tat(ref, src):
        s = np.asarray(src, np.int32)
        return lib.apd_fusion_tat_levels(ctx, ref, len(s), s.ctypes.data, 0.25, 0.0003, None, pix.ctypes.data,
                                         lv.ctypes.data)
    st = {v: k for k, v in A.STATUS.items()}
    try:
        # before set_views
        assert lib.apd_fusion_weak_filter(ctx, 0, 0.17, skip.ctypes.data) == st["APD_ESTATE"]
        assert cons(0, [1]) == st["APD_ESTATE"] and tat(0, [1]) == st["APD_ESTATE"]
        eng.set_views(views)
        assert cons(0, [1, 2]) == 0
        # source / reference index out of range
        for bad in ([4], [1, -1], [1, 2, 99]):
            assert cons(0, bad) == st["APD_EINVAL"] and tat(0, bad) == st["APD_EINVAL"]
        assert cons(4, [0]) == st["APD_EINVAL"] and cons(-1, [0]) == st["APD_EINVAL"]
        assert lib.apd_fusion_weak_filter(ctx, 4, 0.17, skip.ctypes.data) == st["APD_EINVAL"]
        assert b"out of range" in lib.apd_fusion_last_error(ctx)
        # more than APD_MAX_IMAGES sources
        assert cons(0, [1] * 33) == st["APD_ETOOMANYVIEWS"] and tat(0, [1] * 33) == st["APD_ETOOMANYVIEWS"]
        assert cons(0, [1] * 32) == 0
        # the context is still usable
        ref_pix, _, _ = eng.consistency(0, [1, 2], 0.9)
        # a second set_views with fewer views: the old indices are gone
        eng.set_views(views[:2])
        assert cons(0, [1]) == 0
        assert cons(0, [2]) == st["APD_EINVAL"] and cons(3, [0]) == st["APD_EINVAL"]
        assert lib.apd_fusion_weak_filter(ctx, 2, 0.17, skip.ctypes.data) == st["APD_EINVAL"]
        again, _, _ = eng.consistency(0, [1], 0.9)
        assert np.array_equal(again[..., 0], ref_pix[..., 0])
    finally:
        eng.close()
