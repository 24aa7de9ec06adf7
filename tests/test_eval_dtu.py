"""Radius thinning, observability mask, half-space and masked statistics on the device
(include/apd_eval.h, last section), bit for bit against their host twins, and `apd_eval --dtu_gt` end to
end on a synthetic scan (dtu_lib.dtu_scene: a height field of 40 800 ground-truth points, 120 000
reconstruction points with clutter beyond the mask and a slab under the plane)."""
import json
import subprocess

import numpy as np
import pytest

import apd_abi as A
import dtu_lib as D
import synth
from eval_lib import APD_EVAL, f32

pytestmark = pytest.mark.gpu

THIN = {name: (xyz, radius) for name, xyz, radius in D.thin_inputs()}
MASK = np.random.default_rng(8).uniform(size=(7, 5, 3)) < 0.6
ORIGIN, RES = np.array([0.5, -1.0, 10.0]), 0.25


@pytest.fixture(scope="module")
def lib():
    return A.load_library()


@pytest.fixture(scope="module")
def eng(lib):
    e = A.EvalEngine(0, lib)
    yield e
    e.close()


def give(x, where):
    if where == "host" or x is None:
        return x
    import torch
    a = np.ascontiguousarray(x)
    if a.dtype == np.uint32:
        a = a.view(np.int32)  # the same bits
    return torch.from_numpy(a).to(torch.device("cuda", 0))


def take(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else x


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("name", sorted(THIN))
def test_radius_thin_equals_the_host_twin(eng, lib, name, where):
    xyz, radius = THIN[name]
    for mode, rank in D.rank_modes(len(xyz)).items():
        ref = A.radius_thin_host(xyz, radius, rank, lib)
        got = take(eng.radius_thin(give(xyz, where), radius, give(rank, where)))
        assert got.dtype == np.int32 and np.array_equal(got, ref), (name, mode, len(got), len(ref))


def test_a_chain_as_long_as_the_cloud_runs_to_the_fixed_point(eng, lib):
    """3000 collinear points at spacing 0.6 radius in index order, rank = NULL: point k waits for point
    k - 1, so a round limit would show as a difference from the host twin."""
    r = f32(0.2)
    chain = np.zeros((3000, 3), f32)
    chain[:, 0] = np.arange(3000, dtype=f32) * (f32(0.6) * r) + f32(100)
    ref = A.radius_thin_host(chain, r, None, lib)
    got = eng.radius_thin(chain, r, None)
    t = eng.thin_timing()
    print("chain of 3000: rounds", t["rounds"], "rounds_ms", t["rounds_ms"], "kept", len(got))
    assert np.array_equal(got, ref) and len(ref) == 1500
    assert t["rounds"] >= 1 and t["sort_ms"] > 0 and t["rounds_ms"] > 0


def test_two_runs_with_other_work_between_them_give_the_same_bytes(eng, lib):
    xyz, radius = THIN["box6_r05_5000"]
    rank = D.rank_modes(len(xyz))["ranks"]
    first = eng.radius_thin(xyz, radius, rank).copy()
    eng.set_target(THIN["uniform_5000"][0])
    eng.distances(xyz, 1.0)
    eng.voxel_downsample(xyz, 0.3)
    eng.masked_stats(np.arange(3000, dtype=f32), None, 10.0)
    eng.radius_thin(THIN["lattice_tie"][0], 0.25, None)
    again = eng.radius_thin(xyz, radius, rank)
    assert first.tobytes() == again.tobytes() and first.tobytes() == A.radius_thin_host(xyz, radius, rank, lib).tobytes()


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("n", D.SIZES)
def test_mask_half_space_and_stats_equal_their_twins(eng, lib, n, where):
    rng = np.random.default_rng(n + 11)
    x = rng.uniform(-1, 3, (n, 3)).astype(f32) + f32([0, -1, 10])
    if n > 3:
        x[1] = [np.nan, 0, 10]
        x[2, 1] = np.inf
        x[3] = ORIGIN + 1.5 * RES  # on a half-integer index
    got = take(eng.obs_mask(give(x, where), MASK, ORIGIN, RES))
    assert got.dtype == np.uint8 and np.array_equal(got, A.obs_mask_host(x, MASK, ORIGIN, RES, lib))
    P = [0.25, -0.5, 1.0, -10.0]
    got = take(eng.half_space(give(x, where), P))
    assert got.dtype == np.uint8 and np.array_equal(got, A.half_space_host(x, P, lib))
    d = rng.uniform(0, 30, n).astype(f32)
    d[::17] = np.inf
    d[5::19] = np.nan
    flag = (rng.uniform(size=n) < 0.6).astype(np.uint8)
    for f in (flag, None):
        for limit in (20.0, float(np.nextafter(f32(20), f32(0))), np.inf, 0.0):
            assert eng.masked_stats(give(d, where), give(f, where), limit) == A.masked_stats_host(d, f, limit, lib)


def test_mask_is_uploaded_again_when_it_changes(eng, lib):
    x = np.random.default_rng(5).uniform(-1, 3, (2000, 3)).astype(f32) + f32([0, -1, 10])
    a = eng.obs_mask(x, MASK, ORIGIN, RES)
    other = ~MASK
    b = eng.obs_mask(x, other, ORIGIN, RES)
    assert np.array_equal(a, A.obs_mask_host(x, MASK, ORIGIN, RES, lib))
    assert np.array_equal(b, A.obs_mask_host(x, other, ORIGIN, RES, lib)) and not np.array_equal(a, b)
    assert np.array_equal(eng.obs_mask(x, MASK, ORIGIN, RES), a)
    t = eng.dtu_timing()
    assert t["mask_ms"] > 0


def test_status_codes(eng, lib):
    x = np.zeros((4, 3), f32)
    for radius in (0.0, -1.0, np.inf, np.nan, 1e-30, 1e30):
        with pytest.raises(A.ApdError, match="APD_EINVAL"):
            eng.radius_thin(x, radius)
    wide = np.array([[0, 0, 0], [0.4 * 2 ** 21 + 1.0, 0, 0]], f32)
    with pytest.raises(A.ApdError, match="2\\^21 cells"):
        eng.radius_thin(wide, 0.2)
    assert len(eng.radius_thin(x[:0], 0.2)) == 0 and eng.radius_thin(x, 0.2).tolist() == [0]
    assert len(eng.radius_thin(np.full((5, 3), np.nan, f32), 0.2)) == 0
    keep, nk = np.zeros(4, np.int32), A.C.c_int64(0)
    st = lib.apd_eval_radius_thin(eng.ctx, 4, None, 0.2, None, keep.ctypes.data, A.C.addressof(nk))
    assert A.STATUS[st] == "APD_EINVAL"
    st = lib.apd_eval_radius_thin(eng.ctx, 4, x.ctypes.data, 0.2, None, keep.ctypes.data, None)
    assert A.STATUS[st] == "APD_EINVAL"
    st = lib.apd_eval_radius_thin(eng.ctx, -1, x.ctypes.data, 0.2, None, keep.ctypes.data, A.C.addressof(nk))
    assert A.STATUS[st] == "APD_EINVAL"
    for bad in [dict(mask=np.ones((0, 2, 2), bool)), dict(res=0.0), dict(res=np.inf), dict(origin=[0, np.nan, 0])]:
        kw = dict(mask=MASK, origin=ORIGIN, res=RES)
        kw.update(bad)
        with pytest.raises(A.ApdError, match="APD_EINVAL"):
            A.EvalEngine.obs_mask(eng, x, kw["mask"], kw["origin"], kw["res"])
    dims, org, one = np.array([2 ** 11, 2 ** 11, 2 ** 10], np.int32), np.zeros(3), np.ones(1, np.uint8)
    st = lib.apd_eval_obs_mask(eng.ctx, 0, None, dims.ctypes.data, org.ctypes.data, 1.0, one.ctypes.data, None)
    assert A.STATUS[st] == "APD_EINVAL"
    with pytest.raises(A.ApdError, match="APD_EINVAL"):
        eng.masked_stats(np.zeros(3, f32), None, np.nan)
    st = lib.apd_eval_half_space(eng.ctx, 4, x.ctypes.data, None, keep.ctypes.data)
    assert A.STATUS[st] == "APD_EINVAL"


def test_cloud_metrics_dtu_equals_the_protocol_with_the_twins(eng, lib):
    s = D.dtu_scene(seed=2, n_gt_side=40, n_rec=4000)
    for thin in (True, False):
        ref, keep = D.protocol_ref(s["rec"], s["gt"], s["mask"], s["bb"], s["res"], s["plane"], seed=3, thin=thin,
                                   ranks=A.dtu_ranks(len(s["rec"]), 3, lib),
                                   thinner=lambda x, r, rank: A.radius_thin_host(x, r, rank, lib),
                                   nearest=lambda t, q, md: A.nearest_host(t, q, md, lib)[0],
                                   inside=lambda x, m, o, res: A.obs_mask_host(x, m, o, res, lib),
                                   above=lambda x, P: A.half_space_host(x, P, lib),
                                   stats=lambda d, f, lim: A.masked_stats_host(d, f, lim, lib))
        got = A.cloud_metrics_dtu(s["rec"], s["gt"], s["mask"], s["bb"], s["res"], s["plane"], seed=3, thin=thin,
                                  engine=eng)
        assert all(got[k] == ref[k] for k in ref), ({k: got[k] for k in ref}, ref)
        assert np.array_equal(got["keep_idx"], keep) and got["seed"] == 3 and got["thinned"] is thin


# ---- the tool end to end -----------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def scan(tmp_path_factory):
    d = tmp_path_factory.mktemp("dtu_scan")
    s = D.dtu_scene()
    synth.write_ply(str(d / "rec.ply"), s["rec"])
    synth.write_ply(str(d / "gt.ply"), s["gt"])
    D.save_mat(d / "ObsMask.mat", {"ObsMask": s["mask"], "BB": s["bb"], "Res": s["res"], "Margin": 10.0}, compress=True)
    D.save_mat(d / "Plane.mat", {"P": s["plane"].reshape(4, 1)}, compress=False)
    s["dir"] = d
    return s


def run_dtu(scan, name, *extra):
    d = scan["dir"]
    out = d / (name + ".json")
    p = subprocess.run([APD_EVAL, "--cloud", str(d / "rec.ply"), "--dtu_gt", str(d / "gt.ply"), "--dtu_mask",
                        str(d / "ObsMask.mat"), "--dtu_plane", str(d / "Plane.mat"), "--json", str(out),
                        *map(str, extra)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout, p.stderr)
    printed = {}
    for line in p.stdout.splitlines():
        if ": " in line and not line.startswith("DTU protocol"):
            k, v = line.split(": ")
            printed[k.replace(" ", "_")] = float(v)
    return json.loads(out.read_text())["dtu"], printed


def reference(scan, lib, thin=True, seed=0):
    return D.protocol_ref(scan["rec"], scan["gt"], scan["mask"], scan["bb"], scan["res"], scan["plane"], seed=seed,
                          thin=thin, ranks=A.dtu_ranks(len(scan["rec"]), seed, lib),
                          thinner=lambda x, r, rank: A.radius_thin_host(x, r, rank, lib), nearest=D.nearest_kd,
                          inside=lambda x, m, o, res: A.obs_mask_host(x, m, o, res, lib),
                          above=lambda x, P: A.half_space_host(x, P, lib),
                          stats=lambda d, f, lim: A.masked_stats_host(d, f, lim, lib))


FIGURES = ["input_points", "thinned_points", "in_mask_points", "gt_points", "gt_above_plane_points",
           "accuracy_selected", "completeness_selected", "accuracy_mean", "accuracy_median", "completeness_mean",
           "completeness_median", "overall"]


def read_ply15(path):
    raw = open(path, "rb").read()
    body = raw[raw.index(b"end_header\n") + 11:]
    rec = np.frombuffer(body, np.dtype([("xyz", "<f4", 3), ("rgb", "u1", 3)]))
    return np.ascontiguousarray(rec["xyz"])


def test_tool_end_to_end(scan, lib):
    # the restated distances agree with the project's brute-force twin where that is affordable
    sub = scan["rec"][:1500]
    assert np.array_equal(D.nearest_kd(scan["gt"], sub, 20.0), A.nearest_host(scan["gt"], sub, 20.0, lib)[0])
    ref, keep = reference(scan, lib)
    got, printed = run_dtu(scan, "thin", "--thinned_cloud_out", scan["dir"] / "thinned.ply")
    for k in FIGURES:  # counts exact, means and medians the same doubles, printed and in the JSON
        assert got[k] == ref[k] and printed[k] == ref[k], (k, got[k], printed.get(k), ref[k])
    assert got["seed"] == 0 and got["thinned"] is True and got["thin_rounds"] >= 1
    assert len(scan["gt"]) / 4 < got["thinned_points"] < got["input_points"] == len(scan["rec"])
    assert np.array_equal(read_ply15(scan["dir"] / "thinned.ply"), scan["rec"][keep])  # the kept points, in order

    # clutter beyond the mask's box lies within max_dist of the ground truth but does not enter accuracy
    data, label = scan["rec"][keep], scan["label"][keep]
    ins = A.obs_mask_host(data, scan["mask"], scan["bb"][0], scan["res"], lib)
    lim = np.nextafter(f32(20), f32(0))
    d_acc = D.nearest_kd(scan["gt"], data, 20.0)
    assert (label == 1).sum() > 1000 and ins[label == 1].sum() == 0 and (d_acc[label == 1] <= lim).all()
    assert 0 < ins[label == 0].sum() < (label == 0).sum()  # the carved-out corner
    unmasked = A.masked_stats_host(d_acc, None, lim, lib)
    assert unmasked["count"] >= got["accuracy_selected"] + (label == 1).sum()
    assert unmasked["sum"] / unmasked["count"] != got["accuracy_mean"]
    # the slab under the plane draws the ground truth there close, but that part does not enter completeness
    d_comp = D.nearest_kd(data, scan["gt"], 20.0)
    low = np.arange(len(scan["gt"])) >= len(scan["gt"]) - scan["gt_low"]
    abv = A.half_space_host(scan["gt"], scan["plane"], lib)
    assert abv[low].sum() == 0 and abv[~low].all() and (d_comp[low] <= lim).all()
    assert got["gt_above_plane_points"] == len(scan["gt"]) - scan["gt_low"] == got["completeness_selected"]
    everything = A.masked_stats_host(d_comp, None, lim, lib)
    assert everything["count"] == len(scan["gt"]) and everything["sum"] / everything["count"] != got["completeness_mean"]

    # not thinned: a different result that matches as well
    ref2, _ = reference(scan, lib, thin=False)
    got2, printed2 = run_dtu(scan, "nothin", "--dtu_no_thin")
    for k in FIGURES:
        assert got2[k] == ref2[k] and printed2[k] == ref2[k], (k, got2[k], ref2[k])
    assert got2["thinned_points"] == got2["input_points"] and got2["thinned"] is False
    assert got2["accuracy_mean"] != got["accuracy_mean"] and got2["completeness_mean"] != got["completeness_mean"]
