"""apd_prep_* (include/apd_prep.h) and the `apd_prepare` binary on the GPU against the literal numpy
restatement of the contract in tests/prep_lib.py: doubles bit for bit, integers equal, no tolerance
anywhere. Reachable status codes are APD_OK, APD_EINVAL and APD_ESTATE (an allocation or device
failure is not provoked)."""
import ctypes as C
import json
import math
import os
import subprocess

import numpy as np
import pytest

import apd_abi as A
import prep_lib as P

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -5
FRACTIONS = [0.0, 0.01, 0.99, 0.999]
APD_PREPARE = os.path.join(A.HERE, "host", "build", "apd_prepare")
APD = os.path.join(A.HERE, "host", "build", "apd")


@pytest.fixture(scope="module")
def lib():
    return A.load_library()


@pytest.fixture(scope="module")
def eng(lib):
    e = A.PrepEngine(0, lib)
    yield e
    e.close()


@pytest.fixture(scope="module")
def gate(lib):
    return A.prep_cos_gate(1.0, lib)


def identity_cams(centres):
    """R = I, t = -c: the centre comes out as c exactly."""
    c = np.asarray(centres, np.float64).reshape(-1, 3)
    return np.tile(np.eye(3), (len(c), 1, 1)), -c, c.copy()


def check_pairs(eng, gate, rot, trans, cen, xyz, obs):
    """Both atomics paths against the restatement; returns (shared, narrow)."""
    off, pts = P.csr(obs)
    eng.set_model(rot, trans, cen, xyz, off, pts)
    want_s, want_n, want_rec = P.pair_counts_ref(np.asarray(cen, np.float64), np.asarray(xyz, np.float64).reshape(-1, 3),
                                                 obs, gate)
    for mode in (A.PREP_ATOMICS_LDS, A.PREP_ATOMICS_GLOBAL, A.PREP_ATOMICS_DEFAULT):
        s, n = eng.pair_counts(gate, mode)
        assert s.dtype == np.uint32 and n.dtype == np.uint32 and s.shape == want_s.shape
        assert eng.n_records == want_rec
        assert np.array_equal(s, want_s), (mode, int((s != want_s).sum()))
        assert np.array_equal(n, want_n), (mode, int((n != want_n).sum()))
        assert np.array_equal(s, s.T) and np.array_equal(n, n.T)
        assert not s.diagonal().any() and not n.diagonal().any()
    return want_s, want_n


def ring_cams(n, rng):
    images, _, _ = P.ring_model(n, 0, rng)
    m = P.model_ref(images, [], np.zeros((0, 3)))
    return m["rot"], m["trans"], m["centres"]


# ---- pair counts ---------------------------------------------------------------------------------------

def test_track_lengths(eng, gate):
    rng = np.random.default_rng(1)
    n = 70
    rot, trans, cen = ring_cams(n, rng)
    lengths = [0, 1, 2, 3, 63, 64, 65, 0, 2, 65, 1, 3]
    xyz = rng.normal(scale=0.5, size=(len(lengths), 3))
    obs = [[] for _ in range(n)]
    for p, L in enumerate(lengths):
        for i in rng.permutation(n)[:L]:
            obs[i].append(p)
    s, _ = check_pairs(eng, gate, rot, trans, cen, xyz, obs)
    assert int(s.sum()) // 2 == sum(L * (L - 1) // 2 for L in lengths)


def test_one_point_in_2049_images(eng, gate):
    """One track spans many workgroups; its triangular index is unranked up to 2 097 151."""
    rng = np.random.default_rng(2)
    n = 2049
    rot, trans, cen = ring_cams(n, rng)
    xyz = rng.normal(scale=0.5, size=(3, 3))
    obs = [[1] for _ in range(n)]
    obs[5] += [0, 2]
    obs[2047] += [2, 0]
    s, _ = check_pairs(eng, gate, rot, trans, cen, xyz, obs)
    assert eng.n_records == 2049 * 2048 // 2 + 2
    assert s[5, 2047] == 3 and s[0, 2048] == 1


def test_hot_pair(eng, gate):
    rng = np.random.default_rng(3)
    cen = np.array([[0, 0, 0], [0.4, 0, 0], [5, 5, 0]], np.float64)
    rot, trans, cen = identity_cams(cen)
    xyz = np.column_stack([rng.uniform(-2, 2, (5000, 2)), rng.uniform(1, 60, 5000)])
    obs = [list(range(5000)), list(range(5000)), list(range(0, 5000, 7))]
    s, nar = check_pairs(eng, gate, rot, trans, cen, xyz, obs)
    assert s[0, 1] == 5000 and 0 < nar[0, 1] < 5000


def test_ids_duplicates_and_order(eng, gate):
    """Through prep_model_arrays: duplicates within an image, ids -1, unsorted non-contiguous image ids,
    sparse 64-bit point ids."""
    rng = np.random.default_rng(4)
    images, pids, xyz = P.ring_model(9, 60, rng, mean_track=4, first_id=1000, id_step=37,
                                     point_id=lambda k: (1 << 40) + k * 1234567891 if k % 2 else k * 3 + 1)
    for im in images:
        p = im["point_ids"]
        im["point_ids"] = np.concatenate([p, p[:3], [-1, -1], p[:1]]).astype(np.int64)
    order = rng.permutation(len(images))
    shuffled = [images[i] for i in order]
    got = A.prep_model_arrays(shuffled, pids, xyz)
    want = P.model_ref(shuffled, pids, xyz)
    assert got["ids"] == sorted(im["id"] for im in images)
    for k in ("rot", "trans", "centres"):
        assert P.same_bits64(got[k], want[k]), k
    off, pts = P.csr(want["obs"])
    assert np.array_equal(got["obs_offset"], off) and np.array_equal(got["obs_point"], pts)
    s, _ = check_pairs(eng, gate, want["rot"], want["trans"], want["centres"], want["xyz"], want["obs"])
    assert s.any()
    with pytest.raises(ValueError, match="lacks"):
        images[0]["point_ids"][0] = 777777
        A.prep_model_arrays(images, pids, xyz)


def test_point_at_a_centre_and_twin_cameras(eng, gate):
    rng = np.random.default_rng(5)
    cen = np.array([[1, 2, 3], [1, 2, 3], [0.25, -1, 0.5], [7, 7, 7]], np.float64)
    rot, trans, cen = identity_cams(cen)
    xyz = np.vstack([[1.0, 2.0, 3.0], rng.normal(size=(400, 3)) * 3])
    obs = [list(range(401)), list(range(401)), [0, 1, 2, 3], [0]]
    s, nar = check_pairs(eng, gate, rot, trans, cen, xyz, obs)
    q = P.cos_ref(cen[[0]], cen[[2]], xyz[[0]])
    assert np.isnan(q[0])                       # the point at centre 0: NaN compares false
    assert s[0, 1] == 401 and nar[0, 1] == 400  # twins: q = 1 or a rounding off, narrow; the NaN one is not
    qq = P.cos_ref(np.repeat(cen[[0]], 400, 0), np.repeat(cen[[1]], 400, 0), xyz[1:])
    assert np.all(np.abs(qq - 1) <= 2 ** -52) and (qq > 1).any() | (qq == 1).all()
    assert nar[0, 3] == 0 and s[0, 3] == 1


def test_angles_within_ulps_of_the_gate(eng, gate, lib):
    k = 180.0 / math.pi
    assert k * math.acos(gate) < 1.0 and not k * math.acos(np.nextafter(gate, 0.0)) < 1.0
    assert lib.apd_prep_cos_gate(1.0) == gate and math.isnan(lib.apd_prep_cos_gate(0.0))
    # centre a = (1, 0, 0), centre b = (x, s, 0), point at the origin: q = x / sqrt(x*x + s*s)
    s_ = math.sin(math.radians(1.0))
    x = math.cos(math.radians(1.0))
    # dq/dx = s*s / (x*x + s*s)^1.5 ~ 3e-4: 1000 ulps of x move q by about 0.3 ulp
    xs = x + np.arange(-60, 61) * 1000.0 * 2.0 ** -53
    cb = np.column_stack([xs, np.full(len(xs), s_), np.zeros(len(xs))])
    q = P.cos_ref(np.tile([1.0, 0, 0], (len(xs), 1)), cb, np.zeros((len(xs), 3)))
    ulps = q.view(np.int64) - np.float64(gate).view(np.int64)
    keep = np.flatnonzero(np.abs(ulps) <= 3)
    assert (ulps[keep] < 0).any() and (ulps[keep] >= 0).any() and len(keep) >= 6
    cen = np.vstack([[1.0, 0, 0], cb[keep]])
    rot, trans, cen = identity_cams(cen)
    obs = [[0]] + [[0] for _ in keep]
    _, nar = check_pairs(eng, gate, rot, trans, cen, np.zeros((1, 3)), obs)
    assert np.array_equal(nar[0, 1:], (ulps[keep] >= 0).astype(np.uint32))


def test_score_rule_counts_1_to_9(eng, gate):
    cens, xyz, obs, cases = [], [], [], []
    for s in range(1, 10):
        for nn in (3 * s // 4, 3 * s // 4 + 1):
            if nn > s:
                continue
            a = len(cens)
            x0 = 100.0 * a
            cens += [[x0 - 0.5, 0, 0], [x0 + 0.5, 0, 0]]
            obs += [[], []]
            for k in range(s):
                xyz.append([x0, 1000.0 if k < nn else 1.0, 0.1 * k])
                obs[a].append(len(xyz) - 1)
                obs[a + 1].append(len(xyz) - 1)
            cases.append((a, s, nn))
    rot, trans, cen = identity_cams(cens)
    shared, nar = check_pairs(eng, gate, rot, trans, cen, np.array(xyz), obs)
    score = A.prep_score(shared, nar)
    assert np.array_equal(score, P.score_ref(shared, nar))
    for a, s, nn in cases:
        assert shared[a, a + 1] == s and nar[a, a + 1] == nn
        assert score[a, a + 1] == (0 if nn >= 3 * s // 4 + 1 else s)
    assert {nn == 3 * s // 4 for _, s, nn in cases} == {True, False}


# ---- depth ranks ---------------------------------------------------------------------------------------

def test_depth_ranks(eng):
    rng = np.random.default_rng(6)
    counts = [0, 1, 2, 99, 100, 101, 199, 200, 5000, 0, 3]
    rot, trans, cen = ring_cams(len(counts), rng)
    xyz = rng.normal(scale=3.0, size=(700, 3))   # wider than the ring: some points lie behind a camera
    xyz[100:140] = xyz[100]                       # ties
    obs = [rng.integers(0, len(xyz), c).tolist() for c in counts]  # with repeats
    obs[4][:30] = list(range(100, 130))
    off, pts = P.csr(obs)
    eng.set_model(rot, trans, cen, xyz, off, pts)
    z, cnt = eng.depth_ranks(FRACTIONS)
    want_z, want_cnt = P.depth_ranks_ref(rot, trans, xyz, obs, FRACTIONS)
    assert np.array_equal(cnt, want_cnt) and cnt.tolist() == counts
    assert P.same_bits64(z, want_z)
    assert (want_z < 0).any() and not z[0].any() and not z[9].any()
    z2, _ = eng.depth_ranks([0.5])
    assert P.same_bits64(z2, P.depth_ranks_ref(rot, trans, xyz, obs, [0.5])[0])


# ---- the whole -----------------------------------------------------------------------------------------

def test_two_runs_and_a_shuffle_give_identical_bytes(lib):
    rng = np.random.default_rng(7)
    images, pids, xyz = P.ring_model(40, 3000, rng, mean_track=8)
    a = A.prepare_views(images, pids, xyz)
    b = A.prepare_views(images, pids, xyz)
    perm = rng.permutation(len(pids))
    sh_images = []
    for i in rng.permutation(len(images)):
        im = dict(images[i])
        im["point_ids"] = rng.permutation(im["point_ids"])
        sh_images.append(im)
    c = A.prepare_views(sh_images, pids[perm], xyz[perm])
    for other in (b, c):
        for k in ("shared", "narrow", "score", "depth_min", "depth_max", "n_obs"):
            assert a[k].tobytes() == other[k].tobytes(), k
        assert a["selection"] == other["selection"]
    m = P.model_ref(images, pids, xyz)
    gate = A.prep_cos_gate(1.0, lib)
    s, n, _ = P.pair_counts_ref(m["centres"], m["xyz"], m["obs"], gate)
    assert np.array_equal(a["shared"], s) and np.array_equal(a["narrow"], n)
    assert a["selection"] == P.select_ref(P.score_ref(s, n), 20)
    z, cnt = P.depth_ranks_ref(m["rot"], m["trans"], m["xyz"], m["obs"], [0.01, 0.99])
    assert P.same_bits64(a["depth_min"], z[:, 0] * 0.75) and P.same_bits64(a["depth_max"], z[:, 1] * 1.25)
    seq = A.prepare_views(images, pids, xyz, sequential=True, sequential_k=3)
    assert seq["selection"] == P.sequential_ref(40, 3) and "shared" not in seq


def test_status_codes(lib):
    assert not lib.apd_prep_create(99)
    assert b"no such HIP device" in lib.apd_prep_last_error(None)
    ctx = lib.apd_prep_create(0)
    assert ctx
    sh = np.zeros((2, 2), np.uint32)
    z = np.zeros((2, 2))
    fr = np.array([0.5, 0.25])
    assert lib.apd_prep_pair_counts(ctx, 0.5, 0, sh.ctypes.data, None, None) == ESTATE
    assert lib.apd_prep_depth_ranks(ctx, 2, fr.ctypes.data, z.ctypes.data, None) == ESTATE
    rot, trans, cen = identity_cams([[0, 0, 0], [1, 0, 0]])
    xyz = np.array([[0.0, 0, 5], [1, 1, 5]])
    off = np.array([0, 2, 3], np.int64)
    pts = np.array([0, 1, 1], np.int32)

    def set_model(n=2, rot=rot, trans=trans, cen=cen, npts=2, xyz=xyz, nobs=3, off=off, pts=pts):
        p = lambda a: None if a is None else a.ctypes.data
        return lib.apd_prep_set_model(ctx, n, p(rot), p(trans), p(cen), npts, p(xyz), nobs, p(off), p(pts))

    assert set_model(n=0) == EINVAL and set_model(n=A.PREP_MAX_IMAGES + 1) == EINVAL
    assert b"n_images" in lib.apd_prep_last_error(ctx)
    assert set_model(npts=1 << 31) == EINVAL and set_model(nobs=1 << 31) == EINVAL and set_model(nobs=-1) == EINVAL
    assert set_model(rot=None) == EINVAL and set_model(xyz=None) == EINVAL and set_model(pts=None) == EINVAL
    assert set_model(off=np.array([0, 3, 2], np.int64)) == EINVAL
    assert set_model(off=np.array([1, 2, 3], np.int64)) == EINVAL
    assert set_model(off=np.array([0, 2, 4], np.int64)) == EINVAL
    assert set_model(pts=np.array([0, 2, 1], np.int32)) == EINVAL
    assert set_model(pts=np.array([0, -1, 1], np.int32)) == EINVAL
    bad = xyz.copy()
    bad[1, 2] = np.inf
    assert set_model(xyz=bad) == EINVAL
    bad = cen.copy()
    bad[0, 0] = np.nan
    assert set_model(cen=bad) == EINVAL
    assert lib.apd_prep_pair_counts(ctx, 0.5, 0, sh.ctypes.data, None, None) == ESTATE  # still no model
    assert set_model() == 0
    assert lib.apd_prep_pair_counts(ctx, 0.5, 0, None, None, None) == EINVAL
    assert lib.apd_prep_pair_counts(ctx, float("nan"), 0, sh.ctypes.data, None, None) == EINVAL
    assert lib.apd_prep_pair_counts(ctx, 0.5, 3, sh.ctypes.data, None, None) == EINVAL
    assert lib.apd_prep_pair_counts(ctx, 0.5, 0, sh.ctypes.data, None, None) == 0
    assert sh.tolist() == [[0, 1], [1, 0]]
    assert lib.apd_prep_depth_ranks(ctx, 0, fr.ctypes.data, z.ctypes.data, None) == EINVAL
    assert lib.apd_prep_depth_ranks(ctx, 65, fr.ctypes.data, z.ctypes.data, None) == EINVAL
    assert lib.apd_prep_depth_ranks(ctx, 2, None, z.ctypes.data, None) == EINVAL
    assert lib.apd_prep_depth_ranks(ctx, 2, fr.ctypes.data, None, None) == EINVAL
    for f in (1.0, -0.1, float("nan")):
        assert lib.apd_prep_depth_ranks(ctx, 2, np.array([0.5, f]).ctypes.data, z.ctypes.data, None) == EINVAL
    assert lib.apd_prep_depth_ranks(ctx, 2, fr.ctypes.data, z.ctypes.data, None) == 0
    assert z.tolist() == [[5.0, 5.0], [5.0, 5.0]]
    # a model without observations is a model: zero matrices, empty rows
    assert set_model(npts=0, xyz=None, nobs=0, off=np.zeros(3, np.int64), pts=None) == 0
    sh[:] = 9
    assert lib.apd_prep_pair_counts(ctx, 0.5, 0, sh.ctypes.data, None, None) == 0 and not sh.any()
    assert lib.apd_prep_get_timing(ctx, None, None, None, None) == 0 and lib.apd_prep_get_timing(None, None, None, None, None) == EINVAL
    lib.apd_prep_destroy(ctx)
    lib.apd_prep_destroy(None)


def test_interleaved_with_an_eval_engine(lib, gate):
    rng = np.random.default_rng(8)
    images, pids, xyz = P.ring_model(12, 500, rng, mean_track=5)
    m = P.model_ref(images, pids, xyz)
    off, pts = P.csr(m["obs"])
    want = P.pair_counts_ref(m["centres"], m["xyz"], m["obs"], gate)
    cloud = rng.normal(size=(2000, 3)).astype(np.float32)
    prep, ev = A.PrepEngine(0, lib), A.EvalEngine(0, lib)
    try:
        ev.set_target(cloud)
        prep.set_model(m["rot"], m["trans"], m["centres"], m["xyz"], off, pts)
        d0, _ = ev.distances(cloud[:100] + 0.01, 1.0)
        s, n = prep.pair_counts(gate)
        d1, _ = ev.distances(cloud[:100] + 0.01, 1.0)
        z, _ = prep.depth_ranks([0.01, 0.99])
        assert np.array_equal(s, want[0]) and np.array_equal(n, want[1])
        assert d0.tobytes() == d1.tobytes()
        assert P.same_bits64(z, P.depth_ranks_ref(m["rot"], m["trans"], m["xyz"], m["obs"], [0.01, 0.99])[0])
    finally:
        prep.close()
        ev.close()


# ---- the binary ----------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def host():
    A.torch_runtime_first()  # libapdhost.so links libapd_hip.so
    h = C.CDLL(os.path.join(A.HERE, "host", "build", "libapdhost.so"))
    h.apdhost_read_camera.argtypes = [C.c_char_p, C.POINTER(A.ApdCamera)]
    h.apdhost_read_pair_file.restype = C.c_long
    h.apdhost_read_pair_file.argtypes = [C.c_char_p, C.c_void_p, C.c_long, C.c_char_p, C.c_long]
    return h


def read_pairs(host, folder):
    flat, err = np.zeros(1 << 16, np.int32), C.create_string_buffer(512)
    n = host.apdhost_read_pair_file(str(folder).encode(), flat.ctypes.data, flat.size, err, len(err))
    assert n >= 0, err.value
    out, k = [], 0
    for _ in range(n):
        ref, m = int(flat[k]), int(flat[k + 1])
        out.append((ref, flat[k + 2:k + 2 + m].tolist()))
        k += 2 + m
    return out


@pytest.fixture(scope="module")
def model12(tmp_path_factory):
    """A 12-image model in .txt and .bin with its images (one name with a sub-directory) and the
    restatement's results, computed once."""
    rng = np.random.default_rng(12)
    d = tmp_path_factory.mktemp("colmap12")
    images, pids, xyz = P.ring_model(12, 800, rng, mean_track=5, first_id=3, id_step=2)
    cams = [{"id": 7, "model": "PINHOLE", "width": 32, "height": 24, "params": [40.0, 41.0, 15.5, 11.5]}]
    for i, im in enumerate(images):
        im["camera_id"] = 7
        im["name"] = ("sub/im%02d.png" if i == 3 else "im%02d.png") % i
        P.write_png(str(d / "images" / im["name"]), rng.integers(0, 256, (24, 32, 3)))
    P.write_colmap_text(str(d / "sparse"), cams, images, pids, xyz)
    P.write_colmap_bin(str(d / "sparse"), cams, images, pids, xyz)
    m = P.model_ref(images, pids, xyz)
    gate = A.prep_cos_gate(1.0)
    s, n, _ = P.pair_counts_ref(m["centres"], m["xyz"], m["obs"], gate)
    z, cnt = P.depth_ranks_ref(m["rot"], m["trans"], m["xyz"], m["obs"], [0.01, 0.99])
    return d, m, P.select_ref(P.score_ref(s, n), 20), z, cnt


@pytest.mark.parametrize("ext", [".txt", ".bin"])
@pytest.mark.parametrize("mode", ["--no-sequential", "--sequential"])
def test_apd_prepare_on_a_12_image_model(host, model12, tmp_path, ext, mode):
    d, m, want_sel, z, cnt = model12
    out = tmp_path / "scan"
    r = subprocess.run([APD_PREPARE, "--dense_folder", d, "--save_folder", out, "--model_ext", ext, mode,
                        "--sequential_k", "2", "--json", tmp_path / "p.json"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    info = json.loads((tmp_path / "p.json").read_text())
    assert info["images"] == 12 and info["images_copied"] == 12 and info["sequential"] == (mode == "--sequential")
    sel = want_sel if mode == "--no-sequential" else P.sequential_ref(12, 2)
    assert (out / "pair.txt").read_text() == "12\n" + "".join(
        "%d\n%d %s\n" % (i, len(s), "".join("%d %d " % js for js in s)) for i, s in enumerate(sel))
    assert read_pairs(host, out) == [(i, [j for j, sc in s if sc > 0]) for i, s in enumerate(sel)]
    for i in range(12):
        cam = A.ApdCamera()
        assert host.apdhost_read_camera(str(out / "cams" / ("%08d_cam.txt" % i)).encode(), C.byref(cam)) == 0
        assert np.array_equal(np.array(cam.R[:], np.float32), m["rot"][i].astype(np.float32).ravel())
        assert np.array_equal(np.array(cam.t[:], np.float32), m["trans"][i].astype(np.float32))
        assert cam.K[:] == [40.0, 0, 15.5, 0, 41.0, 11.5, 0, 0, 1]
        dmin, interval, num, dmax = P.depth_range_ref(z[i, 0], z[i, 1], cnt[i], 192, 1.0, 40.0)
        want = [np.float32(float("%f" % v)) for v in (dmin, interval, num, dmax)]
        assert [cam.depth_min, cam.interval, cam.depth_num, cam.depth_max] == [float(v) for v in want]
        # the numbers in the file parse back to the same doubles
        rows = (out / "cams" / ("%08d_cam.txt" % i)).read_text().split("\n")
        back = np.array([[float(v) for v in rows[1 + r].split()] for r in range(3)])
        assert P.same_bits64(back[:, :3], m["rot"][i]) and P.same_bits64(back[:, 3], m["trans"][i])
        src = d / "images" / (("sub/im%02d.png" if i == 3 else "im%02d.png") % i)
        assert (out / "images" / ("%08d.png" % i)).read_bytes() == src.read_bytes()
    assert (out / "sparse" / "0" / ("points3D" + ext)).read_bytes() == (d / "sparse" / ("points3D" + ext)).read_bytes()
    assert "7 PINHOLE 32 24 40 41 15.5 11.5" in (out / "sparse" / "0" / "cameras.txt").read_text()
    assert "00000003.png" in (out / "sparse" / "0" / "images.txt").read_text()


def test_prepared_scan_runs_through_apd(tmp_path):
    """The whole chain: a synth scene as a COLMAP model -> apd_prepare -> apd."""
    import synth
    rng = np.random.default_rng(13)
    sc = synth.make_scene(128, 96, 3, seed=11)
    cams, images, pids, xyz = P.scene_to_colmap(sc, rng)
    src = tmp_path / "colmap"
    for im, img in zip(images, sc.images):
        P.write_png(str(src / "images" / im["name"]), np.repeat(np.asarray(img).astype(np.uint8)[:, :, None], 3, 2))
    P.write_colmap_bin(str(src / "sparse"), cams, images, pids, xyz)
    out = tmp_path / "scan"
    r = subprocess.run([APD_PREPARE, "--dense_folder", src, "--save_folder", out, "--model_ext", ".bin", "--no-sequential"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    r = subprocess.run([APD, "--dense_folder", out, "--no_fuse", "true", "--memory_cache", "false"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    depth = synth.read_bin_mat(str(out / "APD" / "00000000" / "depths.bin"))
    assert depth.shape == (96, 128) and (depth > 0).any()
