"""The host twins of include/apd_eval.h's DTU calls (radius thinning, observability mask, half-space,
masked statistics, ranks) against the numpy restatement of tests/dtu_lib.py, the Level-5 MAT-file reader
of `apd_eval --dtu_gt`, that reader under AddressSanitizer + UndefinedBehaviorSanitizer (a stand-alone
program, run directly), and the tool's option checks. No GPU."""
import ctypes as C
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import apd_abi as A
import dtu_lib as D
from eval_lib import APD_EVAL, HOST, f32

SAN_BIN = os.path.join(HOST, "build-san", "mat_corpus_main")
NO_GPU = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
SAN_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
EINVAL = -1

THIN = {name: (xyz, radius) for name, xyz, radius in D.thin_inputs()}


@pytest.fixture(scope="module")
def lib():
    return A.load_library()


# ---- radius thinning -------------------------------------------------------------------------------------

def modes_of(name):
    """every case with ranks and with rank = NULL; the dense, tie and hazard ones with equal and repeated
    ranks as well"""
    full = name.startswith("box6_r05") or name in ("lattice_tie", "hazard", "copies_64")
    return ["ranks", "none", "equal", "repeated"] if full else ["ranks", "none"]


@pytest.mark.parametrize("name", sorted(THIN))
def test_thin_host_equals_the_numpy_loop(lib, name):
    xyz, radius = THIN[name]
    for mode in modes_of(name):
        rank = D.rank_modes(len(xyz))[mode]
        got = A.radius_thin_host(xyz, radius, rank, lib)
        ref = D.thin_ref(xyz, radius, rank)
        assert got.dtype == np.int32 and np.array_equal(got, ref), (name, mode, len(got), len(ref))


def test_thin_host_named_properties(lib):
    xyz, r = THIN["lattice_tie"]  # every neighbour pair ties at d2 == r2: close, so half survive at best
    keep = A.radius_thin_host(xyz, r, None, lib)
    assert 0 < len(keep) <= (len(xyz) + 1) // 2
    for name in ("lattice_above", "lattice_next", "far_apart"):  # none close: all kept
        xyz, r = THIN[name]
        assert np.array_equal(A.radius_thin_host(xyz, r, None, lib), np.arange(len(xyz)))
    xyz, r = THIN["copies_64"]  # exactly the lowest key survives
    rank = D.rank_modes(64)["ranks"]
    assert A.radius_thin_host(xyz, r, None, lib).tolist() == [0]
    assert A.radius_thin_host(xyz, r, rank, lib).tolist() == [int(np.argmin(rank))]
    rep = D.rank_modes(64)["repeated"]
    assert A.radius_thin_host(xyz, r, rep, lib).tolist() == [int(np.flatnonzero(rep == rep.min())[0])]
    xyz, r = THIN["non_finite"]  # dropped, and they suppress nothing: the finite points alone give the same
    fin = np.isfinite(xyz).all(axis=1)
    keep = A.radius_thin_host(xyz, r, None, lib)
    assert fin[keep].all()
    assert np.array_equal(keep, np.flatnonzero(fin)[A.radius_thin_host(xyz[fin], r, None, lib)])


@pytest.mark.parametrize("name", ["uniform_5000", "box6_5000", "box6_r05_5000", "lattice_tie", "hazard", "non_finite"])
@pytest.mark.parametrize("mode", ["ranks", "none"])
def test_thin_host_is_a_maximal_independent_set_by_brute_force(lib, name, mode):
    xyz, radius = THIN[name]
    rank = D.rank_modes(len(xyz))[mode]
    keep = A.radius_thin_host(xyz, radius, rank, lib)
    independent, maximal = D.thin_check(xyz, radius, rank, keep)
    assert independent, "two kept points are close"
    assert maximal, "a removed point has no kept close point with a lower key"


def test_ranks_are_the_projects_philox(lib):
    for seed in (0, 1, 0xFFFFFFFF):
        assert np.array_equal(A.dtu_ranks(300, seed, lib), D.ranks_ref(300, seed))
    # Random123's known answer for counter 0, key 0 ties the pure-Python generator to the published one
    assert D.philox4x32_10((0, 0, 0, 0), (0, 0)) == (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)
    assert len(A.dtu_ranks(0, 0, lib)) == 0


# ---- mask, half-space, statistics ---------------------------------------------------------------------------

MASK = np.random.default_rng(8).uniform(size=(7, 5, 3)) < 0.6
ORIGIN, RES = np.array([0.5, -1.0, 10.0]), 0.25


def mask_points():
    """Points on every half-integer boundary of the cell index, outside each face, on both signs of a .5,
    and non-finite ones."""
    pts = []
    for k in range(3):
        for v in np.arange(-1.0, MASK.shape[k] + 2.0, 0.5):  # v = the unrounded index: x = origin + (v - 1) res
            for dv in (0.0, 2.0 ** -30, -2.0 ** -30):
                p = ORIGIN + 1.0 * RES  # index 2 on the other axes
                p[k] = ORIGIN[k] + (v + dv - 1.0) * RES
                pts.append(p)
    pts = np.array(pts).astype(f32)
    # both signs of a .5: an origin that makes (x - origin) / res + 1 negative halves
    extra = np.array([[np.nan, 0, 10], [0.6, np.inf, 10.2], [0.6, -0.9, -np.inf]], f32)
    rnd = np.random.default_rng(9).uniform(-1, 3, (300, 3)).astype(f32) + f32([0, -1, 10])
    return np.concatenate([pts, extra, rnd])


def test_mask_host_equals_the_numpy_rule(lib):
    x = mask_points()
    got = A.obs_mask_host(x, MASK, ORIGIN, RES, lib)
    ref = D.mask_ref(x, MASK, ORIGIN, RES)
    assert got.dtype == np.uint8 and np.array_equal(got, ref) and 0 < got.sum() < len(x)
    # an origin and res exact in binary, points exactly on .5 of either sign: half away from zero
    m = np.ones((4, 1, 1), bool)
    xs = np.array([[-0.75, 0, 0], [-0.25, 0, 0], [0.25, 0, 0], [1.75, 0, 0], [2.25, 0, 0]], f32)  # v = -0.5 .. 5.5
    # v = x / 0.5 + 1: -0.5 -> -1 (out), 0.5 -> 1, 1.5 -> 2, 4.5 -> 5 (out), 5.5 -> 6 (out)
    assert A.obs_mask_host(xs, m, [0, 0, 0], 0.5, lib).tolist() == [0, 1, 1, 0, 0]
    assert D.mask_ref(xs, m, [0, 0, 0], 0.5).tolist() == [0, 1, 1, 0, 0]
    for n in D.SIZES:
        x = np.random.default_rng(n).uniform(-1, 3, (n, 3)).astype(f32) + f32([0, -1, 10])
        assert np.array_equal(A.obs_mask_host(x, MASK, ORIGIN, RES, lib), D.mask_ref(x, MASK, ORIGIN, RES))


def test_half_space_host_equals_the_numpy_rule(lib):
    P = [0.25, -0.5, 1.0, -2.0]
    rng = np.random.default_rng(3)
    x = rng.uniform(-8, 8, (5000, 3)).astype(f32)
    x[:500, 2] = (2.0 - 0.25 * x[:500, 0].astype(np.float64) + 0.5 * x[:500, 1].astype(np.float64)).astype(f32)
    x[:8] = [[0, 0, 2], [4, 0, 1], [0, 2, 3], [8, 4, 2], [np.nan, 0, 9], [0, np.inf, 0], [0, 0, -np.inf], [0, 0, np.inf]]
    got = A.half_space_host(x, P, lib)
    assert np.array_equal(got, D.half_space_ref(x, P)) and got[:4].tolist() == [0, 0, 0, 0]  # on the plane: not above
    assert got[4] == 0 and got[7] == 1 and 0 < got.sum() < len(x)


@pytest.mark.parametrize("n", D.SIZES)
def test_stats_host_is_bit_equal_to_the_tree_sum(lib, n):
    rng = np.random.default_rng(n + 1)
    d = rng.uniform(0, 30, n).astype(f32)
    d[::17] = np.inf
    d[5::19] = np.nan
    flag = (rng.uniform(size=n) < 0.6).astype(np.uint8)
    for f in (flag, None):
        got, ref = A.masked_stats_host(d, f, 20.0, lib), D.stats_ref(d, f, 20.0)
        assert got == ref, (got, ref)  # count exact, sum and median the same doubles


def test_stats_host_edges(lib):
    lim = np.nextafter(f32(20), f32(0))
    d = np.array([1.0, 3.0, 2.0, 20.0, lim, 50.0], f32)
    assert A.masked_stats_host(d, None, lim, lib) == {"count": 4, "sum": 6.0 + float(lim), "median": 2.5}  # even
    assert A.masked_stats_host(d[:3], None, lim, lib) == {"count": 3, "sum": 6.0, "median": 2.0}  # odd
    assert A.masked_stats_host(d, np.zeros(6, np.uint8), lim, lib) == {"count": 0, "sum": 0.0, "median": 0.0}
    assert A.masked_stats_host(d[:0], None, lim, lib) == {"count": 0, "sum": 0.0, "median": 0.0}
    # exactly at the limit is selected, one ulp above is not; +inf and NaN never, even under limit = +inf
    assert A.masked_stats_host(np.array([lim, 20.0], f32), None, lim, lib)["count"] == 1
    assert A.masked_stats_host(np.array([1.0, np.inf, np.nan], f32), None, np.inf, lib) == \
        {"count": 1, "sum": 1.0, "median": 1.0}
    assert D.stats_ref(np.array([1.0, np.inf, np.nan], f32), None, np.inf) == {"count": 1, "sum": 1.0, "median": 1.0}


def test_host_twins_reject_bad_arguments(lib):
    x = np.zeros((4, 3), f32)
    keep, nk = np.zeros(4, np.int32), C.c_int64(0)

    def thin(n, xyz, radius, keep_ptr, nk_ptr):
        return lib.apd_eval_radius_thin_host(n, xyz, radius, None, keep_ptr, nk_ptr)
    xa, ka, na = x.ctypes.data, keep.ctypes.data, C.addressof(nk)
    assert thin(4, xa, 0.2, ka, na) == 0 and nk.value == 1
    assert thin(0, None, 0.2, None, na) == 0 and nk.value == 0
    for args in [(-1, xa, 0.2, ka, na), (2 ** 31, xa, 0.2, ka, na), (4, None, 0.2, ka, na), (4, xa, 0.2, None, na),
                 (4, xa, 0.2, ka, None), (4, xa, 0.0, ka, na), (4, xa, -1.0, ka, na), (4, xa, np.inf, ka, na),
                 (4, xa, np.nan, ka, na), (4, xa, 1e-30, ka, na), (4, xa, 1e30, ka, na)]:
        assert thin(*args) == EINVAL, args
    wide = np.array([[0, 0, 0], [0.4 * 2 ** 21 + 1.0, 0, 0]], f32)  # more than 2^21 cells of 0.4 apart
    assert thin(2, wide.ctypes.data, 0.2, ka, na) == EINVAL
    with pytest.raises(A.ApdError):
        A.radius_thin_host(wide, 0.2, None, lib)
    for bad in [dict(mask=np.ones((0, 2, 2), bool)), dict(res=0.0), dict(res=np.inf), dict(origin=[0, np.nan, 0])]:
        kw = dict(mask=MASK, origin=ORIGIN, res=RES)
        kw.update(bad)
        with pytest.raises(A.ApdError):
            A.obs_mask_host(x, kw["mask"], kw["origin"], kw["res"], lib)
    dims = np.array([2 ** 11, 2 ** 11, 2 ** 10], np.int32)  # 2^32 cells: rejected before the mask is read
    org = np.zeros(3)
    one = np.ones(1, np.uint8)
    assert lib.apd_eval_obs_mask_host(0, None, dims.ctypes.data, org.ctypes.data, 1.0, one.ctypes.data, None) == EINVAL
    with pytest.raises(A.ApdError):
        A.masked_stats_host(np.zeros(3, f32), None, np.nan, lib)
    assert lib.apd_eval_half_space_host(4, xa, None, keep.ctypes.data) == EINVAL


def test_protocol_with_the_twins_equals_the_numpy_protocol(lib):
    """`apd_eval --dtu_gt`'s sequence of steps on a small scene: pure numpy against the host twins."""
    s = D.dtu_scene(seed=2, n_gt_side=40, n_rec=4000)
    args = (s["rec"], s["gt"], s["mask"], s["bb"], s["res"], s["plane"])
    for thin in (True, False):
        a, ka = D.protocol_ref(*args, thin=thin, seed=3)
        b, kb = D.protocol_ref(*args, thin=thin, ranks=A.dtu_ranks(len(s["rec"]), 3, lib),
                               thinner=lambda x, r, rank: A.radius_thin_host(x, r, rank, lib),
                               nearest=lambda t, q, md: A.nearest_host(t, q, md, lib)[0],
                               inside=lambda x, m, o, res: A.obs_mask_host(x, m, o, res, lib),
                               above=lambda x, P: A.half_space_host(x, P, lib),
                               stats=lambda d, f, lim: A.masked_stats_host(d, f, lim, lib))
        assert a == b and np.array_equal(ka, kb), (a, b)
        assert a["gt_above_plane_points"] == 1600 and 0 < a["in_mask_points"] < a["thinned_points"]
        assert np.array_equal(D.nearest_kd(s["gt"], s["rec"], 20.0), A.nearest_host(s["gt"], s["rec"], 20.0, lib)[0])
    assert a["thinned_points"] == a["input_points"] == 4000


def test_new_symbols_are_declared_and_exported(lib):
    new = ["apd_eval_radius_thin", "apd_eval_radius_thin_host", "apd_eval_get_thin_timing", "apd_eval_dtu_ranks",
           "apd_eval_obs_mask", "apd_eval_obs_mask_host", "apd_eval_half_space", "apd_eval_half_space_host",
           "apd_eval_masked_stats", "apd_eval_masked_stats_host", "apd_eval_get_dtu_timing"]
    assert all(s in A.EVAL_EXPORTS and hasattr(lib, s) for s in new)
    header = open(os.path.join(os.path.dirname(HOST), "..", "include", "apd_eval.h")).read()
    assert all(s + "(" in header for s in new)


# ---- read_mat5 ----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def san_bin():
    r = subprocess.run(["make", "-C", HOST, "sanitize-mat"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return SAN_BIN


def dump(san_bin, path, *names, mask=()):
    args = [san_bin, "--dump"]
    for n in names:
        args += ["--mask" if n in mask else "--want", n]
    r = subprocess.run(args + [str(path)], capture_output=True, text=True, env=SAN_ENV, timeout=120)
    assert r.returncode == 0 and "1 read, 0 rejected" in r.stdout, (r.stdout[-500:], r.stderr[-2000:])
    return {a["name"]: a for a in json.loads(r.stdout.splitlines()[0])["arrays"]}


@pytest.mark.parametrize("compress", [False, True])
def test_mat_round_trips(san_bin, tmp_path, compress):
    rng = np.random.default_rng(2)
    v = {"d3": rng.normal(size=(4, 3, 2)), "d2": rng.normal(size=(2, 3)), "d1": rng.normal(size=5),
         "s2": rng.normal(size=(3, 2)).astype(np.float32), "u8": rng.integers(0, 256, (3, 4, 2)).astype(np.uint8),
         "lg": rng.uniform(size=(5, 4, 3)) < 0.5, "ints": np.array([[1.0, -2.0, 300.0], [70000.0, 0.0, 5.0]]),
         "i64": np.array([2 ** 40, -3], np.int64), "Res": 0.2,
         "st": {"a": 1, "b": "text"}, "ce": np.array([1, "two", np.arange(3.0)], dtype=object), "ch": "a char array"}
    D.save_mat(tmp_path / "m.mat", v, compress)
    names = ["d3", "d2", "d1", "s2", "u8", "lg", "ints", "i64", "Res"]
    got = dump(san_bin, tmp_path / "m.mat", *names, mask=("lg",))
    for n in names:
        a = np.atleast_2d(np.asarray(v[n]))
        if n in ("d1", "i64"):
            a = a.reshape(-1, 1)  # oned_as="column"
        assert got[n]["dims"] == list(a.shape), n
        assert got[n]["logical"] == (n == "lg")
        assert np.array_equal(np.array(got[n]["values"], np.float64), a.astype(np.float64).ravel(order="F")), n
    # a uint8 array asked for as a mask comes as 0 / 1
    assert dump(san_bin, tmp_path / "m.mat", "u8", mask=("u8",))["u8"]["values"] == \
        (v["u8"] != 0).astype(int).ravel(order="F").tolist()


def test_mat_hand_packed_forms(san_bin, tmp_path):
    """What savemat never emits: small-element names and data, a 1-D dimensions array, narrow storage of a
    double class, a logical stored as doubles, an empty matrix element, a compressed element after a plain."""
    vals = np.array([3, 1, 2], np.int16)
    parts = [D.mat_matrix("a", D.MX_DOUBLE, [3], D.MI_INT16, vals.tobytes(), small_name=True),
             D.mat_element(D.MI_MATRIX, b""),
             D.mat_matrix("tiny", D.MX_UINT8, [1, 2], D.MI_UINT8, b"\x07\x00", small_name=True, small_data=True),
             D.mat_compressed(D.mat_matrix("lg", D.MX_DOUBLE, [2, 1, 2], D.MI_DOUBLE,
                                           np.array([0.0, 2.5, -1.0, 0.0]).tobytes(), flags=D.FLAG_LOGICAL)),
             D.mat_matrix("empty", D.MX_DOUBLE, [0, 3], D.MI_DOUBLE, b"")]
    D.write_bytes(tmp_path / "h.mat", D.mat_header() + b"".join(parts))
    got = dump(san_bin, tmp_path / "h.mat", "a", "tiny", "lg", "empty", mask=("lg",))
    assert got["a"]["dims"] == [3] and got["a"]["values"] == [3, 1, 2]
    assert got["tiny"]["dims"] == [1, 2] and got["tiny"]["values"] == [7, 0]
    assert got["lg"]["dims"] == [2, 1, 2] and got["lg"]["logical"] and got["lg"]["values"] == [0, 1, 1, 0]
    assert got["empty"]["dims"] == [0, 3] and got["empty"]["values"] == []


def good_mask_file(compress=False):
    import io
    from scipy.io import savemat
    b = io.BytesIO()
    savemat(b, {"ObsMask": MASK, "BB": np.array([[0.5, -1.0, 10.0], [2.0, 0.0, 10.5]]), "Res": RES,
                "Margin": 10.0, "note": "skipped"}, do_compression=compress)
    return b.getvalue()


def good_plane_file():
    import io
    from scipy.io import savemat
    b = io.BytesIO()
    savemat(b, {"P": np.array([[0.0], [0.0], [1.0], [-9.5]])})
    return b.getvalue()


def bad_mat_files():
    """name -> (bytes of the mask file, what the message must say)"""
    g, gz = good_mask_file(False), good_mask_file(True)
    mask_bytes = (MASK != 0).astype(np.uint8).ravel(order="F").tobytes()
    bb = D.mat_matrix("BB", D.MX_DOUBLE, [2, 3], D.MI_DOUBLE, np.arange(6.0).tobytes())
    res = D.mat_matrix("Res", D.MX_DOUBLE, [1, 1], D.MI_DOUBLE, np.array([0.25]).tobytes())
    hdr = D.mat_header()

    def with_mask(m):
        return hdr + m + bb + res
    first = 128 + 8  # the first element's body in an uncompressed file
    obs = D.mat_matrix("ObsMask", D.MX_UINT8, list(MASK.shape), D.MI_UINT8, mask_bytes, flags=D.FLAG_LOGICAL)
    bomb = obs + b"\0" * (1 << 20)  # a whole ObsMask element, and the stream goes on for a megabyte
    out = {
        "empty": (b"", "shorter than the 128-byte header"),
        "header_cut": (g[:100], "shorter than the 128-byte header"),
        "tag_cut": (g[:128 + 4], "truncated inside an element tag"),
        "element_cut": (g[:first + 40], "overruns the file"),
        "last_element_cut": (g[:-3], "overruns the file"),
        "compressed_cut": (gz[:len(gz) - 20], "overruns the file"),
        "compressed_corrupt": (gz[:200] + bytes(x ^ 0x5A for x in gz[200:260]) + gz[260:], ""),
        "big_endian": (D.mat_header(endian=b"MI") + g[128:], "big-endian"),
        "no_endian_mark": (D.mat_header(endian=b"XX") + g[128:], "endian indicator"),
        "wrong_version": (D.mat_header(version=0x0200) + g[128:], "version"),
        "v73": (b"MATLAB 7.3 MAT-file, Platform: GLNXA64".ljust(128, b" ") + b"\x89HDF\r\n\x1a\n" + b"\0" * 64, "-v7"),
        "inflates_past_declared": (hdr + D.mat_compressed(bomb) + bb + res, "inflates past its declared size"),
        "declares_over_the_cap": (with_mask(D.mat_compressed(struct.pack("<II", D.MI_MATRIX, 0xFFFFFFF0) + b"\0" * 64)),
                                  "inflation cap"),
        "dims_overflow": (with_mask(D.mat_matrix("ObsMask", D.MX_UINT8, [2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1],
                                                 D.MI_UINT8, mask_bytes)), "more than 2^31 elements"),
        "dims_mismatch": (with_mask(D.mat_matrix("ObsMask", D.MX_UINT8, [7, 5, 4], D.MI_UINT8, mask_bytes)),
                          "does not match its dimensions"),
        "negative_dim": (with_mask(D.mat_matrix("ObsMask", D.MX_UINT8, [-7, 5, 3], D.MI_UINT8, mask_bytes)),
                         "negative dimension"),
        "sub_overruns_parent": (with_mask(D.mat_matrix("ObsMask", D.MX_UINT8, list(MASK.shape), D.MI_UINT8, mask_bytes,
                                                       nbytes=80)) , "overruns its matrix"),
        "element_overruns_file": (hdr + struct.pack("<II", D.MI_MATRIX, 1 << 30) + obs[8:], "overruns the file"),
        "mask_is_struct": (with_mask(D.mat_matrix("ObsMask", D.MX_STRUCT, [1, 1], D.MI_INT8, b"")), "is a struct"),
        "mask_is_complex": (with_mask(D.mat_matrix("ObsMask", D.MX_DOUBLE, [1, 2], D.MI_DOUBLE, b"\0" * 16,
                                                   flags=D.FLAG_COMPLEX, imag=b"\0" * 16)), "is complex"),
        "mask_is_4d": (with_mask(D.mat_matrix("ObsMask", D.MX_UINT8, [7, 5, 3, 1], D.MI_UINT8, mask_bytes)),
                       "more than 3 dimensions"),
        "mask_is_double": (with_mask(D.mat_matrix("ObsMask", D.MX_DOUBLE, [1, 2], D.MI_DOUBLE, b"\0" * 16)),
                           "neither logical nor uint8"),
        "mask_is_char": (with_mask(D.mat_matrix("ObsMask", D.MX_CHAR, [1, 2], D.MI_UINT16, b"a\0b\0")), "char"),
        "mask_is_sparse": (with_mask(D.mat_matrix("ObsMask", D.MX_SPARSE, [2, 2], D.MI_INT32, b"\0" * 8)), "sparse"),
        "mask_twice": (with_mask(obs + obs), "occurs twice"),
        "missing_res": (hdr + obs + bb, "variable 'Res' is missing"),
        "bb_wrong_shape": (hdr + obs + res + D.mat_matrix("BB", D.MX_DOUBLE, [3, 2], D.MI_DOUBLE,
                                                          np.arange(6.0).tobytes()), "BB is not 2x3"),
        "res_zero": (hdr + obs + bb + D.mat_matrix("Res", D.MX_DOUBLE, [1, 1], D.MI_DOUBLE, np.zeros(1).tobytes()),
                     "Res is not positive"),
    }
    # cut at the structural boundaries of the first element: behind the header, its tag, the array flags,
    # the dimensions, the name, the real part's tag, and in the middle of the file
    for cut in (128, 136, 152, 176, 192, 200, len(g) // 2):
        out[f"cut_at_{cut}"] = (g[:cut], "")
    return out


BAD_MAT = bad_mat_files()


@pytest.fixture(scope="module")
def dtu_files(tmp_path_factory):
    import synth
    d = tmp_path_factory.mktemp("dtu")
    rng = np.random.default_rng(4)
    synth.write_ply(str(d / "rec.ply"), rng.uniform(-1, 1, (50, 3)).astype(f32))
    (d / "mask.mat").write_bytes(good_mask_file(True))
    (d / "plane.mat").write_bytes(good_plane_file())
    return d


def run_eval(*args):
    return subprocess.run([APD_EVAL, *map(str, args)], capture_output=True, text=True, timeout=120, env=NO_GPU)


def test_valid_mat_files_get_past_the_readers(dtu_files):
    """Everything parses, so the tool goes on to the device and fails there (status 1, not 2)."""
    d = dtu_files
    p = run_eval("--cloud", d / "rec.ply", "--dtu_gt", d / "rec.ply", "--dtu_mask", d / "mask.mat", "--dtu_plane",
                 d / "plane.mat")
    assert p.returncode == 1 and "device" in p.stderr, (p.stdout, p.stderr)


@pytest.mark.parametrize("name", sorted(BAD_MAT))
def test_malformed_mat_file_is_rejected_on_the_host(dtu_files, tmp_path, name):
    blob, message = BAD_MAT[name]
    (tmp_path / "bad.mat").write_bytes(blob)
    d = dtu_files
    for as_mask in (True, False):  # the same bytes as the plane file: P is missing from every one that parses
        args = ["--cloud", d / "rec.ply", "--dtu_gt", d / "rec.ply", "--json", tmp_path / "o.json",
                "--dtu_mask", tmp_path / "bad.mat" if as_mask else d / "mask.mat",
                "--dtu_plane", d / "plane.mat" if as_mask else tmp_path / "bad.mat"]
        p = run_eval(*args)
        assert p.returncode == 2, (p.stdout, p.stderr)
        bad = str(tmp_path / "bad.mat")
        assert bad in p.stderr and len(p.stderr.strip()) > len(bad) + 10 and "device" not in p.stderr, p.stderr
        if as_mask:
            assert message in p.stderr, p.stderr
        assert not (tmp_path / "o.json").exists()


def test_dtu_bad_arguments(dtu_files):
    d = dtu_files
    base = ["--cloud", d / "rec.ply", "--dtu_gt", d / "rec.ply", "--dtu_mask", d / "mask.mat", "--dtu_plane",
            d / "plane.mat"]
    for extra, message in [(["--dtu_density", "0"], "bad --dtu_density 0"), (["--dtu_density", "x"], "bad --dtu_density x"),
                           (["--dtu_density", "1e-30"], "bad --dtu_density 1e-30"),
                           (["--dtu_max_dist", "-1"], "bad --dtu_max_dist -1"), (["--dtu_seed", "-1"], "bad --dtu_seed -1"),
                           (["--dtu_seed", "4294967296"], "bad --dtu_seed"), (["--dtu_seed", "1.5"], "bad --dtu_seed 1.5"),
                           (["--gt", d / "rec.ply"], "--dtu_gt excludes the other modes"),
                           (["--voxel", "0.01"], "--dtu_gt excludes the other modes"),
                           (["--max_dist", "1"], "--dtu_gt excludes the other modes"),
                           (["--gt_mlp", d / "x.mlp"], "--dtu_gt excludes the other modes"),
                           (["--tat_gt", d / "rec.ply", "--tat_crop", d / "c.json", "--tau", "0.01"],
                            "--dtu_gt excludes the other modes")]:
        p = run_eval(*base, *extra)
        assert p.returncode == 2 and message in p.stderr, (extra, p.stdout, p.stderr)
    for k in (2, 4, 6):  # a required file is missing
        p = run_eval(*(base[:k] + base[k + 2:]))
        assert p.returncode == 2 and ("needs --cloud, --dtu_gt, --dtu_mask and --dtu_plane" in p.stderr or
                                      "without --dtu_gt" in p.stderr), p.stderr
    for flag in (["--dtu_no_thin"], ["--dtu_mask", d / "mask.mat"], ["--dtu_plane", d / "plane.mat"],
                 ["--dtu_density", "0.2"], ["--dtu_max_dist", "20"], ["--dtu_seed", "1"],
                 ["--thinned_cloud_out", d / "t.ply"]):  # a DTU flag without --dtu_gt
        p = run_eval("--cloud", d / "rec.ply", "--gt", d / "rec.ply", *flag)
        assert p.returncode == 2 and "without --dtu_gt" in p.stderr, (flag, p.stderr)
    p = run_eval("--help")
    assert p.returncode == 0 and "--dtu_gt" in p.stdout and "--dtu_seed" in p.stdout and "-v7.3" in p.stdout
    for missing in ("mask", "plane"):
        args = list(base)
        args[5 if missing == "mask" else 7] = d / "none.mat"
        p = run_eval(*args)
        assert p.returncode == 2 and str(d / "none.mat") in p.stderr, p.stderr


def test_mat_reader_under_sanitizers(san_bin, tmp_path):
    rng = np.random.default_rng(1)
    good = {"good.mat": good_mask_file(False), "good_z.mat": good_mask_file(True)}
    blobs = dict(good)
    for name, (blob, _) in BAD_MAT.items():
        blobs[name + ".mat"] = blob
    files = []
    for name, data in blobs.items():
        p = tmp_path / name
        p.write_bytes(data)
        files.append(str(p))
    g = good["good.mat"]
    for cut in range(len(g)):  # every prefix of one good file
        p = tmp_path / f"prefix{cut}.mat"
        p.write_bytes(g[:cut])
        files.append(str(p))
    for k in range(200):  # single-byte corruptions, half of them of the compressed file
        src = good["good.mat" if k % 2 else "good_z.mat"]
        b = bytearray(src)
        b[int(rng.integers(0, len(b)))] = int(rng.integers(0, 256))
        p = tmp_path / f"flip{k}.mat"
        p.write_bytes(bytes(b))
        files.append(str(p))
    files += [str(tmp_path), str(tmp_path / "none.mat")]
    r = subprocess.run([san_bin, "--mask", "ObsMask", "--want", "BB", "--want", "Res", *files], capture_output=True,
                       text=True, env=SAN_ENV, timeout=600)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    read, rejected = (int(x) for x in r.stdout.split("mat corpus:")[1].replace("read,", "").replace("rejected", "").split())
    assert read + rejected == len(files) and read >= 2 and rejected >= len(g) - 3
    # the whole files: exactly the good ones are read (bb_wrong_shape and res_zero are the tool's checks)
    whole = [str(tmp_path / n) for n in blobs]
    r = subprocess.run([san_bin, "--mask", "ObsMask", "--want", "BB", "--want", "Res", *whole], capture_output=True,
                       text=True, env=SAN_ENV, timeout=600)
    assert r.returncode == 0 and "mat corpus: 4 read, %d rejected" % (len(whole) - 4) in r.stdout, \
        (r.stdout[-500:], r.stderr[-2000:])
