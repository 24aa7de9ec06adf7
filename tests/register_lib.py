"""Numpy restatement (float64 unless the contract says fp32) of include/apd_eval.h's crop / nearest /
registration contract and of the `apd_eval --tat_gt` protocol, shared by tests/test_eval_register_host.py
(CPU) and tests/test_eval_register.py (GPU). Numpy does not contract a*b+c, so the statements below
round like the C ones."""
import json

import numpy as np

from eval_lib import INF, f32, voxel_ref

REG_BLOCK = 1024
REG_SUMS = 19
UVW = {0: (1, 2, 0), 1: (0, 2, 1), 2: (0, 1, 2)}
IDENTITY = np.eye(4)


def xform64(xyz, T=None):
    """p' of every point, float64 (n, 3): ((T0*x + T1*y) + T2*z) + T3 per row."""
    p = np.asarray(xyz, f32).reshape(-1, 3).astype(np.float64)
    if T is None:
        return p
    T = np.asarray(T, np.float64).reshape(4, 4)
    with np.errstate(all="ignore"):
        return np.stack([((T[r, 0] * p[:, 0] + T[r, 1] * p[:, 1]) + T[r, 2] * p[:, 2]) + T[r, 3] for r in range(3)],
                        axis=1)


def transform_ref(xyz, T=None):
    with np.errstate(all="ignore"):
        return xform64(xyz, IDENTITY if T is None else T).astype(f32)


def crop_ref(xyz, axis, axis_min, axis_max, polygon, T=None):
    """Ascending indices of the kept points."""
    x = np.asarray(xyz, f32).reshape(-1, 3)
    p = xform64(x, T)
    ui, vi, wi = UVW[axis]
    poly = np.asarray(polygon, np.float64).reshape(-1, 2)
    m = len(poly)
    with np.errstate(all="ignore"):
        ok = np.isfinite(x).all(axis=1) & np.isfinite(p).all(axis=1)
        pu, pv, pw = p[:, ui], p[:, vi], p[:, wi]
        ok &= (axis_min <= pw) & (pw <= axis_max)
        odd = np.zeros(len(x), bool)
        for i in range(m):
            j = (i + 1) % m
            Ui, Vi, Uj, Vj = poly[i, 0], poly[i, 1], poly[j, 0], poly[j, 1]
            straddle = (Vi > pv) != (Vj > pv)
            xs = ((Uj - Ui) * (pv - Vi)) / (Vj - Vi) + Ui
            odd ^= straddle & (pu < xs)
    return np.flatnonzero(ok & odd).astype(np.int32)


def nearest_ref(target, q, max_dist):
    """(dist fp32, idx int32, d2 fp32): the fp32 distance contract by brute force, the lowest target index
    among equal d2 (numpy's argmin returns the first minimum), -1 / +inf beyond max_dist."""
    q = np.asarray(q, f32).reshape(-1, 3)
    t = np.asarray(target, f32).reshape(-1, 3)
    fin = np.flatnonzero(np.isfinite(t).all(axis=1))
    tf = t[fin]
    dist = np.full(len(q), INF, f32)
    idx = np.full(len(q), -1, np.int32)
    d2o = np.zeros(len(q), f32)
    if len(tf) == 0 or len(q) == 0:
        return dist, idx, d2o
    md = f32(max_dist)
    with np.errstate(all="ignore"):
        for s in range(0, len(q), 256):
            c = q[s:s + 256]
            dx = c[:, None, 0] - tf[None, :, 0]
            dy = c[:, None, 1] - tf[None, :, 1]
            dz = c[:, None, 2] - tf[None, :, 2]
            d2 = (dx * dx + dy * dy) + dz * dz
            d2 = np.where(np.isnan(d2), INF, d2)
            a = d2.argmin(axis=1)
            mn = d2[np.arange(len(c)), a]
            r = np.sqrt(mn)
            ok = (r <= md) & np.isfinite(c).all(axis=1)
            dist[s:s + 256] = np.where(ok, r, INF)
            idx[s:s + 256] = np.where(ok, fin[a], -1)
            d2o[s:s + 256] = np.where(ok, mn, 0)
    return dist, idx, d2o


def tree_sum(rows):
    """rows (n, k) float64 -> (k,): blocks of 1024 rows padded with +0.0, each summed as a recursive
    pairwise (balanced binary) tree, the block sums added left to right from block 0's sum."""
    rows = np.asarray(rows, np.float64)
    n, k = rows.shape
    total = np.zeros(k)
    for b, s in enumerate(range(0, n, REG_BLOCK)):
        a = np.zeros((REG_BLOCK, k))
        a[:min(REG_BLOCK, n - s)] = rows[s:s + REG_BLOCK]
        while len(a) > 1:
            a = a[0::2] + a[1::2]
        total = a[0].copy() if b == 0 else total + a[0]
    return total


def terms_ref(target, xyz, max_corr, T=None):
    """The (n, 19) terms of one evaluation."""
    t = np.asarray(target, f32).reshape(-1, 3)
    q = transform_ref(xyz, T)
    fin = np.isfinite(q).all(axis=1)
    _, idx, d2 = nearest_ref(t, q, max_corr)
    has = idx >= 0
    v = np.zeros((len(q), REG_SUMS))
    qd = q[has].astype(np.float64)
    td = t[idx[has]].astype(np.float64)
    v[has, 0] = 1.0
    v[has, 1:4] = qd
    v[has, 4:7] = td
    for a in range(3):
        for b in range(3):
            v[has, 7 + 3 * a + b] = qd[:, a] * td[:, b]
    v[has, 16] = (qd[:, 0] * qd[:, 0] + qd[:, 1] * qd[:, 1]) + qd[:, 2] * qd[:, 2]
    v[has, 17] = d2[has].astype(np.float64)
    v[:, 18] = fin
    return v


def sums_ref(target, xyz, max_corr, T=None):
    return tree_sum(terms_ref(target, xyz, max_corr, T))


def info_of(m, iterations):
    return {"iterations": iterations, "n_corr": int(m[0]), "n_finite": int(m[18]),
            "fitness": m[0] / m[18] if m[18] > 0 else 0.0, "rmse": float(np.sqrt(m[17] / m[0])) if m[0] > 0 else 0.0}


def umeyama(m, with_scale):
    """The 4x4 update from the 19 sums, numpy.linalg.svd in place of the project's Jacobi SVD; None if
    it does not exist."""
    N = m[0]
    if N < 3:
        return None
    mq, mt = m[1:4] / N, m[4:7] / N
    C = m[7:16].reshape(3, 3).T / N - np.outer(mt, mq)  # rows: target, columns: source
    var_q = m[16] / N - mq @ mq
    U, D, Vt = np.linalg.svd(C)
    if D[1] <= D[0] * 1e-14:
        return None
    g = -1.0 if np.linalg.det(U @ Vt) < 0 else 1.0
    R = U @ np.diag([1.0, 1.0, g]) @ Vt
    s = 1.0
    if with_scale:
        if not var_q > 0:
            return None
        s = (D[0] + D[1] + g * D[2]) / var_q
    S = np.eye(4)
    S[:3, :3] = s * R
    S[:3, 3] = mt - s * (R @ mq)
    return S


def register_ref(target, xyz, max_corr, T0=None, with_scale=True, max_iter=30, eps_fitness=1e-6, eps_rmse=1e-6):
    """(T, info, ok): the loop of the header."""
    cur = np.eye(4) if T0 is None else np.asarray(T0, np.float64).reshape(4, 4).copy()
    valid, prev, it = cur.copy(), None, 0
    while True:
        m = sums_ref(target, xyz, max_corr, cur)
        info = info_of(m, it)
        if info["n_corr"] < 3:
            return valid, info, False
        valid = cur.copy()
        if prev is not None and abs(info["fitness"] - prev["fitness"]) < eps_fitness and \
                abs(info["rmse"] - prev["rmse"]) < eps_rmse:
            return cur, info, True
        if it == max_iter:
            return cur, info, True
        S = umeyama(m, with_scale)
        if S is None:
            return valid, info, False
        cur = S @ cur
        prev = info
        it += 1


# ---- the apd_eval --tat_gt protocol -------------------------------------------------------------------

def default_stages(tau):
    tau = f32(tau)
    return [(tau, f32(80) * tau), (tau / f32(2), f32(20) * tau), (tau / f32(2), f32(2) * tau)]


def crop_polygon(crop):
    """(axis, axis_min, axis_max, (m, 2) polygon) of a crop dict in the crop-file layout."""
    axis = "XYZ".index(crop["orthogonal_axis"])
    ui, vi, _ = UVW[axis]
    pts = np.asarray(crop["bounding_polygon"], np.float64)
    return axis, float(crop["axis_min"]), float(crop["axis_max"]), np.ascontiguousarray(pts[:, [ui, vi]])


def protocol_ref(rec, gt, crop, tau, T=None, refine=True, with_scale=True, stages=None, iterations=20,
                 register=None, nearest=None):
    """The protocol of `apd_eval --tat_gt`. register(target, source, max_corr, T0, with_scale, max_iter,
    eps_fitness, eps_rmse) -> (T, info, ok) and nearest(target, q, max_dist) -> (dist, ...) default to the
    numpy statements above (brute force: small clouds only); the host twins of apd_abi fit too."""
    register = register or register_ref
    nearest = nearest or nearest_ref
    rec = np.asarray(rec, f32).reshape(-1, 3)
    gt = np.asarray(gt, f32).reshape(-1, 3)
    axis, lo, hi, poly = crop_polygon(crop)
    T = np.eye(4) if T is None else np.asarray(T, np.float64).reshape(4, 4).copy()
    tau = f32(tau)
    gt_c = gt[crop_ref(gt, axis, lo, hi, poly)]

    def source(Tc, voxel):
        s1 = rec[crop_ref(rec, axis, lo, hi, poly, Tc)]
        return s1[voxel_ref(transform_ref(s1, Tc), voxel)]

    infos = []
    if refine:
        for voxel, max_corr in (default_stages(tau) if stages is None else stages):
            tgt = gt_c[voxel_ref(gt_c, voxel)]
            T, info, ok = register(tgt, source(T, voxel), max_corr, T, with_scale, iterations, 1e-6, 1e-6)
            infos.append(dict(info, ok=bool(ok is True or ok == 0)))
    half = tau / f32(2)
    s = transform_ref(source(T, half), T)
    g = gt_c[voxel_ref(gt_c, half)]
    strict = np.nextafter(tau, f32(0))
    dp = nearest(g, s, tau)[0]
    dr = nearest(s, g, tau)[0]
    P = float((dp <= strict).sum()) / len(s) if len(s) else 0.0
    R = float((dr <= strict).sum()) / len(g) if len(g) else 0.0
    F = 2 * P * R / (P + R) if P + R > 0 else 0.0
    return {"T": T, "stages": infos, "source_points": len(s), "target_points": len(g), "precision": P, "recall": R,
            "fscore": F}


def tat_case(gt, tau, seed=11):
    """The end-to-end case of tests/test_eval_register.py from a ground-truth cloud: a crop volume over
    most of it, a reconstruction that is the ground truth under the inverse of residual * trans (a 2
    degree, 0.5 % scale, 0.3 tau residual the refinement must find; trans is what --tat_trans supplies)
    plus 5 % far outliers that land outside the crop polygon. Returns (rec, crop, trans, residual)."""
    gt = np.asarray(gt, f32).reshape(-1, 3)
    rng = np.random.default_rng(seed)
    lo, hi = gt.min(axis=0).astype(np.float64), gt.max(axis=0).astype(np.float64)
    c, h = (lo + hi) / 2, (hi - lo) / 2
    ring = np.array([[-0.9, -0.5], [-0.5, -0.9], [0.5, -0.9], [0.9, -0.5], [0.9, 0.5], [0.5, 0.9], [-0.5, 0.9],
                     [-0.9, 0.5]])
    crop = {"axis_max": float(hi[2] + 1.0), "axis_min": float(lo[2] - 1.0), "orthogonal_axis": "Z",
            "bounding_polygon": [[float(c[0] + u * h[0]), float(c[1] + v * h[1]), 0.0] for u, v in ring]}
    trans = similarity(30.0, [0.2, 1.0, -0.3], 2.0, [1.0, -2.0, 0.5])
    d = 0.3 * float(tau) / np.sqrt(3.0)
    residual = similarity(2.0, [1.0, 0.5, -0.25], 1.005, [d, -d, d])
    n_out = len(gt) // 20
    outliers = np.column_stack([rng.uniform(hi[0] + 4 * h[0], hi[0] + 6 * h[0], n_out), rng.uniform(lo[1], hi[1], n_out),
                                rng.uniform(lo[2], hi[2], n_out)])
    scan_frame = np.concatenate([gt.astype(np.float64), outliers])
    scan_frame = scan_frame[rng.permutation(len(scan_frame))]
    inv = np.linalg.inv(residual @ trans)
    rec = (scan_frame @ inv[:3, :3].T + inv[:3, 3]).astype(f32)
    return rec, crop, trans, residual


def write_crop_json(path, crop):
    with open(path, "w") as f:
        json.dump(dict(crop, class_name="SelectionPolygonVolume", version_major=1, version_minor=0), f, indent=1)


def write_matrix(path, T):
    with open(path, "w") as f:
        for row in np.asarray(T, np.float64).reshape(4, 4):
            f.write(" ".join(repr(float(v)) for v in row) + "\n")


def similarity(angle_deg, axis, scale, translation):
    """4x4 similarity: rotation by angle about axis (Rodrigues), uniform scale, translation."""
    k = np.asarray(axis, np.float64)
    k = k / np.linalg.norm(k)
    a = np.deg2rad(angle_deg)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)
    S = np.eye(4)
    S[:3, :3] = scale * R
    S[:3, 3] = translation
    return S
