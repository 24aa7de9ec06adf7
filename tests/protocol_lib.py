"""Shared by tests/test_eval_protocol.py (GPU), tests/test_eval_protocol_host.py (CPU) and
tools/time_eval_protocol.py: the free-gap / voxel-score contract of include/apd_eval.h restated
literally in numpy (float32 for the floats, Python integers for the ratios), the cube-map table, the
whole scanner protocol built from those, and the room scene the tests draw."""
import numpy as np

from render_lib import cam_arrays, make_cam, project_ref, render_ref

f32 = np.float32
NEG_INF = f32(-np.inf)

# rows (right, down, forward) of the faces +X, -X, +Y, -Y, +Z, -Z
CUBE_R = [[(0, 0, -1), (0, 1, 0), (1, 0, 0)], [(0, 0, 1), (0, 1, 0), (-1, 0, 0)],
          [(1, 0, 0), (0, 0, -1), (0, 1, 0)], [(1, 0, 0), (0, 0, 1), (0, -1, 0)],
          [(1, 0, 0), (0, 1, 0), (0, 0, 1)], [(-1, 0, 0), (0, 1, 0), (0, 0, -1)]]


def cube_cameras_ref(origin, size):
    o = np.asarray(origin, f32).reshape(3)
    K = [[size / 2, 0, size / 2 - 0.5], [0, size / 2, size / 2 - 0.5], [0, 0, 1]]
    cams = []
    for rows in CUBE_R:
        R = np.array(rows, f32)
        t = np.array([-(r[0] * o[0] + r[1] * o[1] + r[2] * o[2]) for r in R], f32)  # exact: entries 0 and +-1
        cams.append(make_cam(K, R, t, size, size))
    return cams


def in_view_ref(xyz, cam):
    """(bool[n] centre pixel inside the image of a kept point, d, u, v)"""
    _, _, _, W, H = cam_arrays(cam)
    kept, d, u, v = project_ref(xyz, cam)
    return kept & (u >= 0) & (u < W) & (v >= 0) & (v < H), d, u, v


def free_gap_ref(xyz, cams, depths):
    n = len(np.asarray(xyz).reshape(-1, 3))
    gap = np.full(n, NEG_INF, f32)
    for cam, dep in zip(cams, depths):
        _, _, _, W, H = cam_arrays(cam)
        inb, d, u, v = in_view_ref(xyz, cam)
        dep = np.ascontiguousarray(dep, f32).reshape(H, W)
        j = np.flatnonzero(inb)
        with np.errstate(all="ignore"):
            zb = dep[v[j], u[j]]
            ok = zb > 0
            e = zb[ok] - d[j[ok]]
        assert e.dtype == f32 and not np.isnan(e).any()
        gap[j[ok]] = np.maximum(gap[j[ok]], e)
    return gap


def classes_ref(dist, gap, tol):
    """(good, bad) bool arrays for one tolerance"""
    t = f32(tol)
    with np.errstate(all="ignore"):
        good = np.asarray(dist, f32) <= t
        bad = ~good if gap is None else ~good & (np.asarray(gap, f32) > t)
    return good, bad


def voxel_scores_ref(xyz, voxel, dist, gap, tolerances):
    """dict of lists of Python integers: good, bad, ratio_sum, voxels"""
    x = np.asarray(xyz, f32).reshape(-1, 3)
    fin = np.flatnonzero(np.isfinite(x).all(axis=1))
    out = {k: [] for k in ("good", "bad", "ratio_sum", "voxels")}
    if len(fin):
        with np.errstate(all="ignore"):
            cells = np.floor(x[fin] / f32(voxel))
        assert cells.dtype == f32
        inv = np.unique(cells.astype(np.float64) + 0.0, axis=0, return_inverse=True)[1].reshape(-1)  # -0.0 -> 0.0
        nv = int(inv.max()) + 1
    for t in np.asarray(tolerances, f32).reshape(-1):
        if not len(fin):
            for k in out:
                out[k].append(0)
            continue
        good, bad = classes_ref(np.asarray(dist, f32)[fin], None if gap is None else np.asarray(gap, f32)[fin], t)
        a = np.bincount(inv, good, nv).astype(np.int64)
        b = np.bincount(inv, bad, nv).astype(np.int64)
        rs = cnt = 0
        for ai, bi in zip(a.tolist(), b.tolist()):
            if ai + bi > 0:
                rs += (ai << 32) // (ai + bi)
                cnt += 1
        out["good"].append(int(a.sum()))
        out["bad"].append(int(b.sum()))
        out["ratio_sum"].append(rs)
        out["voxels"].append(cnt)
    return out


def score_of(ratio_sum, voxels):
    return [float(r) / (float(v) * 4294967296.0) if v else 0.0 for r, v in zip(ratio_sum, voxels)]


def scores_equal(got, want):
    """the four integer outputs of EvalEngine.voxel_scores against voxel_scores_ref"""
    return all([int(v) for v in got[k]] == want[k] for k in ("good", "bad", "ratio_sum", "voxels"))


def finite_rows(x):
    x = np.ascontiguousarray(x, f32).reshape(-1, 3)
    return np.ascontiguousarray(x[np.isfinite(x).all(axis=1)])


def protocol_ref(rec, scans, tolerances, voxel, cube_size, splat, max_dist, brute):
    """The whole scanner protocol from the references: brute = eval_lib.brute."""
    R = finite_rows(rec)
    parts = [finite_rows(p) for p, _ in scans]
    G = np.ascontiguousarray(np.concatenate(parts))
    gap = np.full(len(R), NEG_INF, f32)
    for p, (_, o) in zip(parts, scans):
        cams = cube_cameras_ref(o, cube_size)
        gap = np.maximum(gap, free_gap_ref(R, cams, [render_ref(p, c, splat)[0] for c in cams]))
    da = brute(R, G, max_dist)
    dc = brute(G, R, max_dist)
    return {"R": R, "G": G, "gap": gap, "accuracy_dist": da, "completeness_dist": dc,
            "accuracy": voxel_scores_ref(R, voxel, da, gap, tolerances),
            "completeness": voxel_scores_ref(G, voxel, dc, None, tolerances)}


# ---- MeshLab projects and coloured clouds ------------------------------------------------------------

def mlp_text(meshes, numbers_per_line=4):
    """A MeshLab project: meshes = [(filename, 4x4 matrix or a ready string for the matrix body)]."""
    out = ["<!DOCTYPE MeshLabDocument>", "<MeshLabProject>", " <MeshGroup>"]
    for name, M in meshes:
        out.append('  <MLMesh label="%s" filename="%s">' % (name.split("/")[-1], name))
        if M is not None:
            if not isinstance(M, str):
                v = ["%.17g" % float(x) for x in np.asarray(M, np.float64).reshape(-1)]
                M = "\n".join(" ".join(v[i:i + numbers_per_line]) + " " for i in range(0, len(v), numbers_per_line))
            out.append("   <MLMatrix44>\n%s\n</MLMatrix44>" % M)
        out.append("  </MLMesh>")
    out += [" </MeshGroup>", " <RasterGroup/>", "</MeshLabProject>", ""]
    return "\n".join(out)


def to_world_ref(xyz, M):
    """M (x, y, z, 1) in float64, every sum left to right, rounded once to float32; the origin"""
    M = np.asarray(M, np.float64).reshape(4, 4)
    p = np.asarray(xyz, f32).reshape(-1, 3).astype(np.float64)
    w = np.stack([M[r, 0] * p[:, 0] + M[r, 1] * p[:, 1] + M[r, 2] * p[:, 2] + M[r, 3] for r in range(3)], axis=1)
    return w.astype(f32), M[:3, 3].astype(f32)


def read_ply_xyz_rgb(path):
    """(xyz float32 (n, 3), rgb uint8 (n, 3)) of the 15-byte layout write_ply_xyz_rgb makes"""
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    lines = head.decode().split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    n = int([ln for ln in lines if ln.startswith("element vertex")][0].split()[2])
    props = [ln.split()[1:] for ln in lines if ln.startswith("property")]
    assert props == [["float", "x"], ["float", "y"], ["float", "z"], ["uchar", "red"], ["uchar", "green"],
                     ["uchar", "blue"]]
    rec = np.frombuffer(body, np.dtype([("p", "<f4", 3), ("c", "u1", 3)]))
    assert len(rec) == n and len(body) == 15 * n
    return rec["p"].copy(), rec["c"].copy()


def colours_ref(dist, gap, tol):
    good, bad = classes_ref(dist, gap, tol)
    rgb = np.zeros((len(good), 3), np.uint8)
    rgb[good] = (0, 255, 0)
    rgb[bad] = (255, 0, 0)
    rgb[~good & ~bad] = (0, 0, 255)
    return rgb


# ---- the room scene ---------------------------------------------------------------------------------

ROOM_ORIGINS = [(0.5, 0.3, -0.4), (-0.8, -0.5, 0.6)]


def _on_cube(rng, n, half):
    """n points on the surface of the axis-aligned cube of half-width `half`"""
    p = rng.uniform(-half, half, (n, 3))
    ax = rng.integers(0, 3, n)
    p[np.arange(n), ax] = half * rng.choice([-1.0, 1.0], n)
    return p


def room_scene(seed=11):
    """Two scanners inside a cube of half-width 2, each scanning 6000 random wall points; scanner 1
    also scans a box of half-width 0.3 at (1, 0, 0) (the faces it can see from its side, roughly:
    the points of that box nearer to it than the box centre plane). The reconstruction: 3000 wall
    points with sigma 0.02, 1200 floaters inside (free space), 1200 points on a shell of half-width
    2.6 (behind the walls), 400 points inside the small box. Returns (rec, scans, parts)."""
    rng = np.random.default_rng(seed)
    walls = [_on_cube(rng, 6000, 2.0) for _ in ROOM_ORIGINS]
    box = _on_cube(rng, 1500, 0.3) + [1.0, 0.0, 0.0]
    scans = [(np.concatenate([walls[0], box]).astype(f32), np.array(ROOM_ORIGINS[0], f32)),
             (walls[1].astype(f32), np.array(ROOM_ORIGINS[1], f32))]
    rec = np.concatenate([_on_cube(rng, 3000, 2.0) + rng.normal(0, 0.02, (3000, 3)),
                          rng.uniform(-1.9, 1.9, (1200, 3)),
                          _on_cube(rng, 1200, 2.6),
                          rng.uniform(-0.25, 0.25, (400, 3)) + [1.0, 0.0, 0.0]]).astype(f32)
    parts = {"wall": slice(0, 3000), "floater": slice(3000, 4200), "shell": slice(4200, 5400),
             "box": slice(5400, 5800)}
    return rec, scans, parts
