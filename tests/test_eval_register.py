"""Crop volume, nearest neighbour with index, transform and registration on the device
(include/apd_eval.h, last section), bit for bit against their host twins, and `apd_eval --tat_gt` end to
end on a synthetic scene.

The end-to-end case (register_lib.tat_case on the 160x120 scene, tau = 0.1): the protocol restated with
the host twins on the CPU gives, without refinement, precision 0.7975 / recall 0.8023, and refined
0.9959 / 0.9953, so the residual of 2 degrees, 0.5 % scale and 0.3 tau lies inside the basin."""
import json
import subprocess

import numpy as np
import pytest

import apd_abi as A
import cases
import register_lib as RL
import synth
from eval_lib import APD_EVAL, f32, same_bits

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 3, 1023, 1024, 1025, 5000]
POLY = np.array([[-2.0, -2.0], [2.0, -2.0], [2.5, 0.0], [2.0, 2.0], [0.0, 0.25], [-2.0, 2.0], [-2.5, 0.5],
                 [-2.25, -1.0]])  # concave
SKEW = RL.similarity(7.0, [1.0, -2.0, 0.5], 1.1, [0.2, -0.1, 0.3])
TRUTH = RL.similarity(3.0, [0.3, -0.5, 0.8], 1.01, [0.03, -0.02, 0.04])


@pytest.fixture(scope="module")
def lib():
    return A.load_library()


@pytest.fixture(scope="module")
def eng(lib):
    e = A.EvalEngine(0, lib)
    yield e
    e.close()


def give(x, where):
    if where == "host":
        return x
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to(torch.device("cuda", 0))


def take(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else x


def cloud(n, seed=0):
    rng = np.random.default_rng(100 + seed + n)
    x = rng.uniform(-3.5, 3.5, (n, 3)).astype(f32)
    if n > 3:
        x[1] = [np.nan, 0, 0]
        x[n // 2, 2] = np.inf
    return x


def pair(n):
    """A source of n points and a target: the source under TRUTH, some of it duplicated (ties), a fifth of
    the source moved out of reach."""
    rng = np.random.default_rng(7 + n)
    src = rng.uniform(-4, 4, (n, 3)).astype(f32)
    tgt = RL.transform_ref(src, TRUTH)
    tgt = np.concatenate([tgt, tgt[: n // 3], rng.uniform(-4, 4, (257, 3)).astype(f32)])
    if n > 8:
        src[rng.random(n) < 0.2] += f32(100.0)
        src[2] = np.nan
        tgt[5] = np.nan
    return src, tgt


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("n", SIZES)
def test_crop_volume_equals_the_host_twin(eng, lib, n, where):
    x = cloud(n)
    for axis, T in ((0, None), (1, SKEW), (2, None)):
        got = take(eng.crop_volume(give(x, where), axis, -1.25, 1.5, POLY, T))
        want = A.crop_volume_host(x, axis, -1.25, 1.5, POLY, T, lib=lib)
        assert got.dtype == np.int32 and np.array_equal(got, want)
        if n >= 1023:
            assert 0 < len(want) < n
    if n == 5000 and where == "host":
        assert np.array_equal(want, RL.crop_ref(x, 2, -1.25, 1.5, POLY))
        with pytest.raises(A.ApdError, match="APD_EINVAL"):
            eng.crop_volume(x, 0, -1.0, 1.0, POLY[:2])
        with pytest.raises(A.ApdError, match="APD_EINVAL"):
            eng.crop_volume(x, 3, -1.0, 1.0, POLY)


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("n", SIZES)
def test_nearest_and_transform_equal_the_host_twins(eng, lib, n, where):
    src, tgt = pair(n)
    eng.set_target(give(tgt, where))
    moved = eng.transform(give(src, where), TRUTH)
    assert same_bits(take(moved), A.transform_host(src, TRUTH, lib=lib))
    assert same_bits(take(eng.transform(give(src, where))), src if n else np.zeros((0, 3), f32))
    for md in (np.inf, 0.25):
        dist, idx = eng.nearest(moved, md)
        wd, wi = A.nearest_host(tgt, take(moved), md, lib=lib)
        assert same_bits(take(dist), wd) and np.array_equal(take(idx), wi)
    if n >= 1023:  # the duplicated targets were hit at their first copy (target 5 is NaN: its second, n + 5)
        hit = wi[wi >= 0]
        assert len(hit) > n // 2 and (hit[hit >= n] == n + 5).all() and wi[5] == n + 5
    d_only, _ = eng.distances(take(moved), 0.25)
    assert same_bits(d_only, A.nearest_host(tgt, take(moved), 0.25, lib=lib)[0])


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("n", SIZES)
def test_register_equals_the_host_twin(eng, lib, n, where):
    src, tgt = pair(n)
    eng.set_target(tgt)
    sums = eng.register_sums(give(src, where), 0.6, SKEW)
    want = A.register_sums_host(tgt, src, 0.6, SKEW, lib=lib)
    assert np.array_equal(sums.view(np.uint64), want.view(np.uint64)), (sums, want)
    for with_scale in (1, 0):
        T, info, st = eng.register(give(src, where), 0.6, None, with_scale, 12, 1e-9, 1e-9, raise_on_state=False)
        Th, info_h, st_h = A.register_host(tgt, src, 0.6, None, with_scale, 12, 1e-9, 1e-9, lib=lib)
        assert st == st_h and info == info_h, (st, st_h, info, info_h)
        assert np.array_equal(T.view(np.uint64), Th.view(np.uint64)), np.abs(T - Th).max()
        if n >= 1023:
            assert st == 0 and info["n_corr"] > n // 2 and info["iterations"] >= 2
            if with_scale:
                assert np.abs(T - TRUTH).max() < 1e-4  # it converged on the known answer, too
        if n <= 1:
            assert A.STATUS[st] == "APD_ESTATE" and np.array_equal(T, np.eye(4))


def test_run_to_run_identity(eng):
    src, tgt = pair(5000)
    eng.set_target(tgt)
    a = eng.register(src, 0.6, SKEW @ np.linalg.inv(SKEW), 1, 8, 0.0, 0.0)
    sa = eng.register_sums(src, 0.6)
    na = eng.nearest(src, 0.6)
    eng.set_target(tgt[::-1].copy())  # other work in between
    eng.nearest(src, 0.1)
    eng.set_target(tgt)
    b = eng.register(src, 0.6, SKEW @ np.linalg.inv(SKEW), 1, 8, 0.0, 0.0)
    sb = eng.register_sums(src, 0.6)
    nb = eng.nearest(src, 0.6)
    assert np.array_equal(a[0].view(np.uint64), b[0].view(np.uint64)) and a[1] == b[1] and a[1]["iterations"] == 8
    assert np.array_equal(sa.view(np.uint64), sb.view(np.uint64))
    assert same_bits(na[0], nb[0]) and np.array_equal(na[1], nb[1])
    t = eng.register_timing()
    assert t["evaluations"] == 1 and t["eval_ms"] > 0 and t["fold_ms"] > 0


def test_status_codes(eng, lib):
    src, tgt = pair(64)
    fresh = A.EvalEngine(0, lib)
    try:
        with pytest.raises(A.ApdError, match="APD_ESTATE"):
            fresh.nearest(src, 0.5)
        with pytest.raises(A.ApdError, match="APD_ESTATE"):
            fresh.register(src, 0.5)
    finally:
        fresh.close()
    eng.set_target(tgt)
    for kw in [dict(max_corr=0.0), dict(max_corr=np.inf), dict(max_iter=0), dict(max_iter=1001), dict(eps_rmse=-1.0),
               dict(T0=np.full((4, 4), np.nan))]:
        args = dict(max_corr=0.5, T0=None, with_scale=True, max_iter=5, eps_fitness=0.0, eps_rmse=0.0)
        args.update(kw)
        with pytest.raises(A.ApdError, match="APD_EINVAL"):
            eng.register(src, **args)
    with pytest.raises(A.ApdError, match="APD_EINVAL"):
        eng.nearest(src, -1.0)
    with pytest.raises(A.ApdError, match="APD_EINVAL"):
        eng.transform(src, np.full((4, 4), np.inf))


# ---- apd_eval --tat_gt end to end ---------------------------------------------------------------------

TAU = 0.1
KEYS = {"definition", "tau", "with_scale", "refine", "stages", "transform", "source", "target", "within_precision",
        "within_recall", "precision", "recall", "fscore", "crop_ms", "voxel_ms", "transform_ms", "build_ms", "query_ms"}
STAGE_KEYS = {"voxel", "max_corr", "source_points", "target_points", "ok", "iterations", "n_corr", "n_finite", "fitness",
              "rmse", "evaluations", "eval_ms", "fold_ms", "solve_ms"}


@pytest.fixture(scope="module")
def tat(tmp_path_factory):
    d = tmp_path_factory.mktemp("tat")
    gt = synth.gt_cloud(cases.scene(160, 120, 4))
    rec, crop, trans, residual = RL.tat_case(gt, TAU)
    synth.write_ply(str(d / "rec.ply"), rec)
    synth.write_ply(str(d / "gt.ply"), gt)
    RL.write_crop_json(d / "crop.json", crop)
    RL.write_matrix(d / "trans.txt", trans)
    (d / "tau.txt").write_text(repr(TAU))
    return {"dir": d, "gt": gt, "rec": rec, "crop": crop, "trans": trans, "residual": residual}


def run_tat(tat, name, *extra):
    d = tat["dir"]
    out = d / (name + ".json")
    p = subprocess.run([APD_EVAL, "--cloud", str(d / "rec.ply"), "--tat_gt", str(d / "gt.ply"), "--tat_crop",
                        str(d / "crop.json"), "--tat_trans", str(d / "trans.txt"), "--tau",
                        (d / "tau.txt").read_text(), "--json", str(out), *map(str, extra)],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout, p.stderr)
    return json.loads(out.read_text())["tat"], p.stdout


def check_against_restatement(tat, res, lib):
    """The counts and shares the tool reports are those of the restated protocol under the tool's own T."""
    T = np.array(res["transform"]).reshape(4, 4)
    nn = lambda t, q, md: A.nearest_host(t, q, float(md), lib=lib)
    ref = RL.protocol_ref(tat["rec"], tat["gt"], tat["crop"], TAU, T, refine=False, nearest=nn)
    assert res["source"]["points"] == ref["source_points"] and res["target"]["points"] == ref["target_points"]
    assert res["precision"] == ref["precision"] and res["recall"] == ref["recall"] and res["fscore"] == ref["fscore"]
    return T


def test_cli_end_to_end(eng, lib, tat):
    d = tat["dir"]
    plain, out_plain = run_tat(tat, "plain", "--no_refine")
    fine, out_fine = run_tat(tat, "fine", "--aligned_cloud_out", d / "aligned.ply")
    for res in (plain, fine):
        assert set(res) == KEYS
        assert set(res["source"]) == set(res["target"]) == {"points_in", "points_cropped", "points"}
    assert plain["stages"] == [] and plain["refine"] is False and len(fine["stages"]) == 3 and fine["refine"] is True
    print("no refinement:", plain["precision"], plain["recall"], plain["fscore"])
    print("refined:", fine["precision"], fine["recall"], fine["fscore"], fine["stages"])
    assert np.array_equal(np.array(plain["transform"]).reshape(4, 4), tat["trans"])
    check_against_restatement(tat, plain, lib)
    T = check_against_restatement(tat, fine, lib)
    assert plain["fscore"] < fine["fscore"]
    assert fine["precision"] >= 0.99 and fine["recall"] >= 0.99
    tau32 = f32(TAU)
    want = [(tau32, f32(80) * tau32), (tau32 / f32(2), f32(20) * tau32), (tau32 / f32(2), f32(2) * tau32)]
    for s, (voxel, max_corr) in zip(fine["stages"], want):
        assert set(s) == STAGE_KEYS and s["ok"] is True and 1 <= s["iterations"] <= 20
        assert f32(s["voxel"]) == voxel and f32(s["max_corr"]) == max_corr and s["n_corr"] >= 0.9 * s["n_finite"] > 0
    # the far outliers (5 % of the input) never get past the crop
    n_gt, n_out = len(tat["gt"]), len(tat["gt"]) // 20
    for res in (plain, fine):
        assert res["source"]["points_in"] == n_gt + n_out and res["target"]["points_in"] == n_gt
        assert res["source"]["points_cropped"] <= n_gt and abs(res["source"]["points_cropped"] -
                                                                 res["target"]["points_cropped"]) < 0.02 * n_gt
    for line in ("precision:", "recall:", "f-score:", "stage 3:"):
        assert line in out_fine
    # the aligned cloud is apd_eval_transform of the whole input under the final T
    aligned = A_read_ply(d / "aligned.ply", lib)
    assert same_bits(aligned, eng.transform(tat["rec"], T)) and same_bits(aligned, A.transform_host(tat["rec"], T, lib=lib))


def test_cli_stage_table_and_rigid(tat, lib):
    res, _ = run_tat(tat, "custom", "--refine_stages", "0.2:4,0.1:1", "--no_scale", "--init_trans",
                     _write_init(tat))
    assert len(res["stages"]) == 2 and res["with_scale"] is False
    assert [f32(s["voxel"]) for s in res["stages"]] == [f32(0.2), f32(0.1)]
    T = check_against_restatement(tat, res, lib)
    scale = np.cbrt(np.linalg.det(T[:3, :3]))
    init_scale = np.cbrt(np.linalg.det((tat["residual"] @ tat["trans"])[:3, :3]))
    assert abs(scale - init_scale) < 1e-9  # rigid updates leave the scale of init * trans alone


def _write_init(tat):
    p = tat["dir"] / "init.txt"
    RL.write_matrix(p, tat["residual"])
    return p


def A_read_ply(path, lib):
    """xyz of the 15-byte-record PLY the tool writes (float x, y, z + three colour bytes)."""
    blob = open(path, "rb").read()
    head = blob.index(b"end_header\n") + 11
    n = int(blob[:head].split(b"element vertex ")[1].split()[0])
    rec = np.frombuffer(blob[head:], np.dtype([("p", "<f4", 3), ("c", "u1", 3)]))
    assert len(rec) == n
    return np.ascontiguousarray(rec["p"])
