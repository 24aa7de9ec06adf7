"""Numpy restatements of the DTU contract of include/apd_eval.h (radius thinning, observability mask,
half-space, masked statistics, the rank generator, the protocol of `apd_eval --dtu_gt`) and a writer
of Level-5 MAT-files for fixtures: scipy.io.savemat, plus hand-packed elements for what savemat never
emits. No GPU and no project library is needed by anything here except where a callable is passed in."""
import struct
import zlib

import numpy as np

from eval_lib import f32
from register_lib import tree_sum


# ---- radius thinning --------------------------------------------------------------------------------

def close32(P, i, cand, r2):
    """Which of the points `cand` are close to point i: d2 = (dx*dx + dy*dy) + dz*dz <= r2, every
    operation an np.float32 one in the contract's order."""
    d = P[cand] - P[i]  # float32 - float32; the sign does not matter to the squares
    with np.errstate(all="ignore"):
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    return d2 <= r2


def thin_order(n, finite, rank):
    """The finite points in ascending key (rank << 32 | index)."""
    idx = np.flatnonzero(finite)
    if rank is None:
        return idx
    r = np.asarray(rank, np.uint32)[idx]
    return idx[np.argsort(r, kind="stable")]


def thin_ref(xyz, radius, rank=None, brute=None):
    """Ascending indices kept by the greedy loop. Candidates come from a cKDTree with a generous radius
    (or from all points when brute, default for n <= 2048); every decision is the fp32 test."""
    P = np.ascontiguousarray(xyz, f32).reshape(-1, 3)
    n = len(P)
    radius = f32(radius)
    r2 = f32(radius * radius)
    finite = np.isfinite(P).all(axis=1)
    order = thin_order(n, finite, rank)
    kept = np.zeros(n, bool)
    if brute is None:
        brute = n <= 2048
    if brute:
        fin_idx = np.flatnonzero(finite)
        for i in order:
            cand = fin_idx[kept[fin_idx]]
            if len(cand) == 0 or not close32(P, i, cand, r2).any():
                kept[i] = True
        return np.flatnonzero(kept).astype(np.int32)
    from scipy.spatial import cKDTree
    fin_idx = np.flatnonzero(finite)
    P64 = P[fin_idx].astype(np.float64)
    tree = cKDTree(P64)
    # generous: half a radius and eight fp32 ulps of the largest coordinate beyond the radius
    lists = tree.query_ball_point(P64, 1.5 * float(radius) + float(np.abs(P64).max(initial=0.0)) * 2.0 ** -20)
    where = np.full(n, -1, np.int64)
    where[fin_idx] = np.arange(len(fin_idx))
    for i in order:
        cand = fin_idx[np.asarray(lists[where[i]], np.int64)]
        cand = cand[kept[cand]]
        if len(cand) == 0 or not close32(P, i, cand, r2).any():
            kept[i] = True
    return np.flatnonzero(kept).astype(np.int32)


def thin_check(xyz, radius, rank, keep):
    """Independent of the loop, by brute force: (no two kept points are close, every finite removed point
    has a kept close point with a lower key)."""
    P = np.ascontiguousarray(xyz, f32).reshape(-1, 3)
    n = len(P)
    radius = f32(radius)
    r2 = f32(radius * radius)
    finite = np.isfinite(P).all(axis=1)
    key = (np.zeros(n, np.uint64) if rank is None else np.asarray(rank, np.uint64) << np.uint64(32)) | np.arange(
        n, dtype=np.uint64)
    keep = np.asarray(keep, np.int64)
    kept = np.zeros(n, bool)
    kept[keep] = True
    independent = True
    for a, i in enumerate(keep):
        rest = keep[a + 1:]
        if len(rest) and close32(P, i, rest, r2).any():
            independent = False
            break
    maximal = True
    for i in np.flatnonzero(finite & ~kept):
        c = keep[close32(P, i, keep, r2)]
        if not (key[c] < key[i]).any():
            maximal = False
            break
    return independent, maximal and bool(finite[keep].all())


SIZES = (0, 1, 2, 1023, 1024, 1025, 5000)


def hazard_points(radius=0.2):
    """Coordinates at integer multiples of the radius and one ulp either side, on each axis and sign, at
    offsets 0, 100 and 599: neighbours along the axis are close or not by one rounding, and they sit on
    the borders of any grid whose cell is a multiple of the radius."""
    pts = []
    for off in (0.0, 100.0, 599.0):
        for axis in range(3):
            for sg in (1.0, -1.0):
                for k in range(7):
                    c = f32(sg * (off + k * radius))
                    for v in (np.nextafter(c, f32(-np.inf)), c, np.nextafter(c, f32(np.inf))):
                        p = np.full(3, f32(sg * off), f32)
                        p[axis] = v
                        pts.append(p)
    return np.array(pts, f32)


def lattice(base, spacing, dims):
    """base + k * spacing per axis, computed in float64 and required to be exact in float32."""
    ax = [np.float64(base) + np.arange(d) * np.float64(spacing) for d in dims]
    g = np.stack(np.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3)
    assert (g.astype(f32).astype(np.float64) == g).all(), "the lattice is not exact in float32"
    return g.astype(f32)


def thin_inputs():
    """(name, xyz float32 (n, 3), radius) for every thinning case of the issue."""
    rng = np.random.default_rng(20)
    out = []
    for n in SIZES:
        out.append((f"uniform_{n}", rng.uniform(-300, 600, (n, 3)).astype(f32), 0.2))
        out.append((f"box6_{n}", (rng.uniform(0, 6, (n, 3)) + [40, -70, 500]).astype(f32), 0.2))
        out.append((f"box6_r05_{n}", (rng.uniform(0, 6, (n, 3)) + [40, -70, 500]).astype(f32), 0.5))
    # spacing == radius, far from the origin: every neighbour pair ties at d2 == r2 (close)
    out.append(("lattice_tie", lattice(512.0, 0.25, (17, 17, 17)), 0.25))
    # the smallest spacing above the radius that the coordinates' ulp (2^-14 at 512) allows: none close
    out.append(("lattice_above", lattice(512.0, 0.25 + 2.0 ** -14, (17, 17, 17)), 0.25))
    # spacing nextafterf(radius, inf) exactly, which float32 holds for three steps at the origin
    out.append(("lattice_next", lattice(0.0, float(np.nextafter(f32(0.25), f32(1))), (3, 3, 3)), 0.25))
    out.append(("hazard", hazard_points(0.2), 0.2))
    out.append(("copies_64", np.tile(np.array([[12.5, -3.25, 599.0]], f32), (64, 1)), 0.2))
    out.append(("far_apart", lattice(-2.0, 1.0, (5, 5, 5)), 0.2))
    bad = (rng.uniform(0, 3, (1500, 3)) + [10, 20, 30]).astype(f32)
    bad[::7, 0] = np.nan
    bad[3::11, 1] = np.inf
    bad[5::13, 2] = -np.inf
    out.append(("non_finite", bad, 0.2))
    return out


def rank_modes(n, seed=3):
    """with ranks, with rank = None, with all ranks equal, and with heavily repeated ranks"""
    rng = np.random.default_rng(seed + n)
    return {"ranks": rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32), "none": None,
            "equal": np.full(n, 7, np.uint32), "repeated": rng.integers(0, 4, n).astype(np.uint32)}


# ---- mask, half-space, statistics ----------------------------------------------------------------------

def round_half_away(x):
    return np.floor(np.abs(x) + 0.5) * np.sign(x)


def mask_ref(xyz, mask, origin, res):
    P = np.ascontiguousarray(xyz, f32).reshape(-1, 3)
    m = np.asarray(mask) != 0
    origin = np.asarray(origin, np.float64).reshape(3)
    finite = np.isfinite(P).all(axis=1)
    with np.errstate(all="ignore"):
        v = round_half_away((P.astype(np.float64) - origin) / np.float64(res) + 1.0)
    ok = finite.copy()
    for k in range(3):
        ok &= (v[:, k] >= 1) & (v[:, k] <= m.shape[k])
    out = np.zeros(len(P), np.uint8)
    vi = v[ok].astype(np.int64) - 1
    out[ok] = m[vi[:, 0], vi[:, 1], vi[:, 2]]
    return out


def half_space_ref(xyz, plane):
    P = np.ascontiguousarray(xyz, f32).reshape(-1, 3).astype(np.float64)
    p = np.asarray(plane, np.float64).reshape(4)
    with np.errstate(all="ignore"):
        s = ((p[0] * P[:, 0] + p[1] * P[:, 1]) + p[2] * P[:, 2]) + p[3]
        return (s > 0).astype(np.uint8)


def stats_ref(dist, flag, limit):
    d = np.ascontiguousarray(dist, f32).reshape(-1)
    with np.errstate(all="ignore"):
        sel = (d <= f32(limit)) & np.isfinite(d)
    if flag is not None:
        sel &= np.asarray(flag).reshape(-1) != 0
    rows = np.where(sel, d.astype(np.float64), 0.0).reshape(-1, 1)
    total = float(tree_sum(rows)[0]) if len(d) else 0.0
    s = d[sel]
    # ascending in the sign-magnitude order of the bits (-0 before +0)
    u = s.view(np.uint32)
    o = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))
    s = s[np.argsort(o, kind="stable")]
    m = len(s)
    if m == 0:
        med = 0.0
    elif m & 1:
        med = float(s[(m - 1) // 2])
    else:
        med = (float(s[m // 2 - 1]) + float(s[m // 2])) / 2.0
    return {"count": m, "sum": total, "median": med}


# ---- ranks: a pure-Python Philox4x32-10 ------------------------------------------------------------------

def philox4x32_10(ctr, key):
    x0, x1, x2, x3 = ctr
    k0, k1 = key
    M = 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = 0xD2511F53 * x0, 0xCD9E8D57 * x2
        x0, x1, x2, x3 = (p1 >> 32) ^ x1 ^ k0, p1 & M, (p0 >> 32) ^ x3 ^ k1, p0 & M
        k0, k1 = (k0 + 0x9E3779B9) & M, (k1 + 0xBB67AE85) & M
    return x0, x1, x2, x3


def ranks_ref(n, seed=0):
    return np.array([philox4x32_10((i, 0, 0, 0), (seed & 0xFFFFFFFF, 0))[0] for i in range(n)], np.uint32)


# ---- the protocol ------------------------------------------------------------------------------------------

def nearest_kd(target, q, max_dist, k=8):
    """The distance contract for finite clouds without brute force: the k nearest targets in float64 from a
    cKDTree are the candidates (far more than can tie within fp32 rounding), the minimum is taken over
    their fp32 d2 = (dx*dx + dy*dy) + dz*dz, then sqrt in fp32 and the cut at max_dist."""
    from scipy.spatial import cKDTree
    t = np.ascontiguousarray(target, f32).reshape(-1, 3)
    q = np.ascontiguousarray(q, f32).reshape(-1, 3)
    if len(t) == 0 or len(q) == 0:
        return np.full(len(q), np.inf, f32)
    k = min(k, len(t))
    _, idx = cKDTree(t.astype(np.float64)).query(q.astype(np.float64), k=k)
    idx = idx.reshape(len(q), k)
    d = q[:, None, :] - t[idx]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    m = np.sqrt(d2.min(axis=1))
    return np.where(m <= f32(max_dist), m, f32(np.inf)).astype(f32)


def protocol_ref(rec, gt, mask, bb, res, plane, density=0.2, max_dist=20.0, seed=0, thin=True, ranks=None,
                 thinner=None, nearest=None, inside=None, above=None, stats=None):
    """The steps of `apd_eval --dtu_gt`. The callables default to the restatements above (nearest: brute
    force through register_lib.nearest_ref); tests pass the project's host twins."""
    from register_lib import nearest_ref
    rec = np.ascontiguousarray(rec, f32).reshape(-1, 3)
    gt = np.ascontiguousarray(gt, f32).reshape(-1, 3)
    thinner = thinner or thin_ref
    nearest = nearest or (lambda t, q, md: nearest_ref(t, q, md)[0])
    inside = inside or mask_ref
    above = above or half_space_ref
    stats = stats or stats_ref
    bb = np.asarray(bb, np.float64).reshape(2, 3)
    if thin:
        rank = ranks_ref(len(rec), seed) if ranks is None else ranks
        keep = np.asarray(thinner(rec, f32(density), rank))
    else:
        keep = np.arange(len(rec), dtype=np.int32)
    data = np.ascontiguousarray(rec[keep])
    md = f32(max_dist)
    limit = np.nextafter(md, f32(0))
    d_acc = nearest(gt, data, md)
    d_comp = nearest(data, gt, md)
    ins = np.asarray(inside(data, mask, bb[0], res))
    abv = np.asarray(above(gt, plane))
    sa, sc = stats(d_acc, ins, limit), stats(d_comp, abv, limit)
    out = {"input_points": len(rec), "thinned_points": len(data), "in_mask_points": int(ins.sum()),
           "gt_points": len(gt), "gt_above_plane_points": int(abv.sum()),
           "accuracy_selected": sa["count"], "completeness_selected": sc["count"],
           "accuracy_mean": sa["sum"] / sa["count"] if sa["count"] else 0.0, "accuracy_median": sa["median"],
           "completeness_mean": sc["sum"] / sc["count"] if sc["count"] else 0.0,
           "completeness_median": sc["median"]}
    out["overall"] = (out["accuracy_mean"] + out["completeness_mean"]) / 2.0
    return out, keep


def dtu_scene(seed=5, n_gt_side=200, n_rec=120000):
    """A synthetic scan in millimetres: a smooth height field sampled at spacing 0.2 as ground truth; a
    reconstruction of noisy resamplings of it, 5 % clutter outside the mask's box and a slab of points
    below the plane; a box mask with a carved-out corner; a plane under the surface."""
    rng = np.random.default_rng(seed)

    def height(x, y):
        return 3.0 * np.sin(x / 9.0) * np.cos(y / 7.0) + 0.05 * x

    g = np.arange(n_gt_side) * 0.2
    gx, gy = np.meshgrid(g, g, indexing="ij")
    gt = np.stack([gx.ravel(), gy.ravel(), height(gx, gy).ravel()], 1).astype(f32)
    side = float(g[-1])
    n_surf = int(n_rec * 0.85)
    sx, sy = rng.uniform(0, side, n_surf), rng.uniform(0, side, n_surf)
    surf = np.stack([sx, sy, height(sx, sy)], 1) + rng.normal(0, 0.08, (n_surf, 3))
    n_clut = int(n_rec * 0.05)
    # beyond the mask's box (which ends 5 past the surface) but within max_dist of the ground truth
    clutter = np.stack([rng.uniform(side + 8, side + 15, n_clut), rng.uniform(0, side, n_clut),
                        rng.uniform(-5, 5, n_clut)], 1)
    n_slab = n_rec - n_surf - n_clut
    slab = np.stack([rng.uniform(0, side, n_slab), rng.uniform(0, side, n_slab), rng.uniform(-14, -12, n_slab)], 1)
    rec = np.concatenate([surf, clutter, slab]).astype(f32)
    label = np.concatenate([np.zeros(n_surf, np.uint8), np.ones(n_clut, np.uint8), np.full(n_slab, 2, np.uint8)])
    perm = rng.permutation(len(rec))
    rec, label = np.ascontiguousarray(rec[perm]), label[perm]  # label: 0 surface, 1 clutter, 2 slab
    res = 0.5
    bb = np.array([[-5.0, -5.0, -20.0], [side + 5.0, side + 5.0, 10.0]])
    dims = np.floor((bb[1] - bb[0]) / res).astype(int) + 1
    mask = np.ones(tuple(dims), bool)
    mask[: dims[0] // 4, : dims[1] // 4, :] = False  # the carved-out corner
    plane = np.array([0.0, 0.0, 1.0, 8.0])  # z > -8: the slab at -13 is below
    # the part of the ground truth below the plane: a strip pushed down
    gt_low = gt[: n_gt_side * 4].copy()
    gt_low[:, 2] = f32(-11.0)
    gt = np.ascontiguousarray(np.concatenate([gt, gt_low]))
    return {"rec": rec, "label": label, "gt": gt, "gt_low": len(gt_low), "mask": mask, "bb": bb, "res": res,
            "plane": plane}


# ---- MAT-file fixtures ----------------------------------------------------------------------------------------

MI_INT8, MI_UINT8, MI_INT16, MI_UINT16, MI_INT32, MI_UINT32, MI_SINGLE, MI_DOUBLE = 1, 2, 3, 4, 5, 6, 7, 9
MI_INT64, MI_UINT64, MI_MATRIX, MI_COMPRESSED = 12, 13, 14, 15
MX_CELL, MX_STRUCT, MX_CHAR, MX_SPARSE, MX_DOUBLE, MX_SINGLE, MX_INT8, MX_UINT8 = 1, 2, 4, 5, 6, 7, 8, 9
MX_INT32 = 12
FLAG_COMPLEX, FLAG_LOGICAL = 0x0800, 0x0200


def save_mat(path, variables, compress=False):
    """scipy.io.savemat, Level 5."""
    from scipy.io import savemat
    savemat(path, variables, format="5", do_compression=compress, oned_as="column")


def mat_header(endian=b"IM", text=b"MATLAB 5.0 MAT-file, written by tests/dtu_lib.py", version=0x0100):
    return text.ljust(116, b" ") + b"\0" * 8 + struct.pack("<H", version) + endian


def mat_element(mi, payload, small=False, nbytes=None):
    """A tagged data element padded to 8 bytes; small: the 4-byte-payload tag form."""
    n = len(payload) if nbytes is None else nbytes
    if small:
        assert len(payload) <= 4
        return struct.pack("<HH", mi, n) + payload.ljust(4, b"\0")
    return struct.pack("<II", mi, n) + payload + b"\0" * (-len(payload) % 8)


def mat_matrix(name, mx_class, dims, mi, data, flags=0, small_name=False, small_data=False, imag=None,
               nbytes=None):
    """An miMATRIX element: array flags, dimensions, name, real part (and an imaginary part)."""
    body = mat_element(MI_UINT32, struct.pack("<II", mx_class | flags, 0))
    body += mat_element(MI_INT32, struct.pack("<%di" % len(dims), *dims))
    nm = name.encode()
    body += mat_element(MI_INT8, nm, small=small_name and len(nm) <= 4)
    body += mat_element(mi, data, small=small_data and len(data) <= 4)
    if imag is not None:
        body += mat_element(mi, imag)
    return mat_element(MI_MATRIX, body, nbytes=nbytes)


def mat_compressed(element, declared=None):
    z = zlib.compress(element)
    return struct.pack("<II", MI_COMPRESSED, len(z) if declared is None else declared) + z


def write_bytes(path, data):
    with open(path, "wb") as f:
        f.write(data)
    return path
