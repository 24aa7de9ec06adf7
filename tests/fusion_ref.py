"""Float64 restatement of the reference's depth-map fusion, written from APD.cpp (not from
oracle/fusion_oracle.c): Get3DPointonWorld / ProjectCamera / GetAngle (APD.cpp:866-910), WeakVisFilter
(:972-1026), the RunFusion loop (:1140-1222), RunFusion_TAT_I / _A (:1340-1428, :1534-1603) and
ExportPointCloud's uchar truncation (:344-348). Plain Python loops over Python floats (binary64).

Every value comes with a running error bound for a float32 evaluation of the same expression: the
expression evaluated on absolute values, times gamma(n) = n*u / (1 - n*u), u = 2**-24, n = the number
of rounded operations on the longest path (counted below, next to each constant). A quotient x / y
uses A(x) / |y| * (A(y) / |y|): the second factor is the denominator's own condition number, so a
cancelling denominator widens the bound. That bound is the only tolerance anywhere in the fusion
tests; a decision is "guarded" when its float64 value is farther than the bound from its cut.

Undefined reference behaviours, fixed as in DESIGN section 9:
  - confidences[i].at<float>(r, c) on the 8-bit map is the float whose 4 little-endian bytes start
    at byte r*W + 4c; bytes past the W*H buffer are 0;
  - int() of NaN or of a value outside int's range is out of bounds;
  - the TAT cost cache is declared once per image and persists across pixels and rows
    (reset_tat_cache=True resets it per pixel instead: what the code would do had `diff` been
    declared inside the pixel loop; used to show that a scan depends on the carry).
"""
import math
import struct

import numpy as np

U = 2.0 ** -24


def gamma(n):
    return n * U / (1.0 - n * U)


# rounded operations on the longest path of each expression
N_X = 7        # world point: (x - K2) 1, depth * 2, / K0 3, R row: mul 4, add 5, add 6, + C 7
#                (C = -(R^T t): mul, add, add = 3, the shorter branch)
N_PD = 14      # projected depth: world point 7, R row mul 8, add 9, add 10, + t 11, K row mul 12, add 13, add 14
N_RND = 16     # px + 0.5f: the projected pixel (the same 14 as the depth for the numerator, / depth 15), + 0.5f 16
N_DIST = 20    # source pixel's world point 7 + projection 8 = 15, (c - x) 16, square 17, add 18, sqrt 19, cast 20
N_REL = 16     # projected depth 14, - ref_depth 15, / ref_depth 16 (fabs is exact)
N_Q = 5        # GetAngle's acosf argument: dot mul 1, add 2, add 3, the double quotient 4, its cast to float 5
N_ACOS = 1     # acosf itself (glibc: below one ulp)
N_VQ = 13      # the view-angle q: world point 7, (c - X) 8, dot mul 9, add 10, add 11, quotient 12, cast 13
N_DEG = 3      # acosf 1, * 180.0f 2, / M_PI and the cast back to float 3
N_OCC = 2      # src_depth - 0.01f * src_depth: mul 1, subtract 2
N_TMP = 3      # reproj + 200 * rel + angle * 10: mul 1, add 2, add 3 (angle * 10 is the shorter branch)
N_EXP = 1      # expf (the negation is exact)
N_FACT = 1     # factor * num_consistent
N_KCUT = 1     # k * depth_base (k * 0.25f is exact)
N_ACUT = 2     # k * angle_grad + angle_base
N_COL = 1      # colour: integer sums below 2**24 are exact, one division
G = {n: gamma(n) for n in range(1, 64)}

F32 = lambda x: float(np.float32(x))  # noqa: E731
CUT_DIST, CUT_REL, CUT_ANGLE = 2.0, F32(0.01), F32(0.174533)
FACT_WEAK, FACT_STRONG = F32(0.45), F32(0.3)
OCC = F32(0.01)
DIST_BASE = 0.25
DEPTH_BASE = {1: float(np.float32(1.0) / np.float32(3500.0)), 2: float(np.float32(1.0) / np.float32(3000.0))}
ANGLE_BASE, ANGLE_GRAD = F32(0.06981317007977318), F32(0.05235987755982988)
FLT_MAX = float(np.finfo(np.float32).max)
WEAK, STRONG = 0, 1
NAN, INF = float("nan"), float("inf")


def _div(a, b):
    if b != 0.0:
        return a / b
    if a != a or a == 0.0 or b != b:
        return NAN
    return math.copysign(INF, a) * math.copysign(1.0, b)


def _finite(x):
    return x == x and x not in (INF, -INF)


class Guards:
    """Every decision taken, which side it fell on, and the ones closer to their cut than the bound."""

    def __init__(self):
        self.total = 0
        self.bad = []
        self.cov = {}

    def _note(self, name, res, val, cut, bound, where):
        self.total += 1
        c = self.cov.setdefault(name, [0, 0])
        c[1 if res else 0] += 1
        if _finite(val) and not abs(val - cut) > bound:  # a non-finite value compares false in any precision
            self.bad.append((name, where, val, cut, bound))
        return res

    def lt(self, name, val, cut, bound, where=None):
        return self._note(name, val < cut, val, cut, bound, where)

    def gt(self, name, val, cut, bound, where=None):
        return self._note(name, val > cut, val, cut, bound, where)

    def le(self, name, val, cut, bound, where=None):
        return self._note(name, val <= cut, val, cut, bound, where)

    def trunc(self, name, val, bound, where=None, size=None):
        """int(val) as the reference's cast: toward zero; None for NaN / out of int's range. A value
        whose whole error interval lies outside (-1, size) is out of bounds whatever it rounds to."""
        if not (val >= -2147483648.0 and val < 2147483648.0):
            return None
        self.total += 1
        if size is not None and (val + bound < -1.0 or val - bound > size):
            return int(val)
        near = float(round(val))
        if not abs(val - near) > bound:
            self.bad.append((name, where, val, near, bound))
        c = self.cov.setdefault(name + " in (-1,0)", [0, 0])  # truncation gives 0 there, floor would give -1
        c[1 if -1.0 < val < 0.0 else 0] += 1
        return int(val)


def world_point(cam, x, y, d):
    """Get3DPointonWorld: (X, A) with A the same expression on absolute values."""
    K, R, t = cam["K"], cam["R"], cam["t"]
    px = _div(d * (x - K[2]), K[0])
    py = _div(d * (y - K[5]), K[4])
    ad = abs(d)
    apx = ad * (abs(x) + abs(K[2])) / abs(K[0])
    apy = ad * (abs(y) + abs(K[5])) / abs(K[4])
    X, A = [], []
    for i in range(3):  # the rotation uses R's columns: R^T p - R^T t
        X.append((R[i] * px + R[3 + i] * py + R[6 + i] * d) - (R[i] * t[0] + R[3 + i] * t[1] + R[6 + i] * t[2]))
        A.append(abs(R[i]) * apx + abs(R[3 + i]) * apy + abs(R[6 + i]) * ad
                 + abs(R[i] * t[0]) + abs(R[3 + i] * t[1]) + abs(R[6 + i] * t[2]))
    return X, A


def project(cam, X, A):
    """ProjectCamera: (px, py, depth) and their absolute-value evaluations."""
    K, R, t = cam["K"], cam["R"], cam["t"]
    T, B = [], []
    for i in range(3):  # R's rows: R X + t
        T.append(R[3 * i] * X[0] + R[3 * i + 1] * X[1] + R[3 * i + 2] * X[2] + t[i])
        B.append(abs(R[3 * i]) * A[0] + abs(R[3 * i + 1]) * A[1] + abs(R[3 * i + 2]) * A[2] + abs(t[i]))
    dep = K[6] * T[0] + K[7] * T[1] + K[8] * T[2]
    adep = abs(K[6]) * B[0] + abs(K[7]) * B[1] + abs(K[8]) * B[2]
    nx = K[0] * T[0] + K[1] * T[1] + K[2] * T[2]
    ny = K[3] * T[0] + K[4] * T[1] + K[5] * T[2]
    anx = abs(K[0]) * B[0] + abs(K[1]) * B[1] + abs(K[2]) * B[2]
    any_ = abs(K[3]) * B[0] + abs(K[4]) * B[1] + abs(K[5]) * B[2]
    cond = _div(adep, abs(dep))
    return (_div(nx, dep), _div(ny, dep), dep), (_div(anx, abs(dep)) * cond, _div(any_, abs(dep)) * cond, adep)


def angle_q(a, b):
    """GetAngle's acosf argument: (q, A(q)), A(q) the same expression on absolute values."""
    dot = a[0] * b[0] + a[1] * b[1] + a[2] * b[2]
    adot = abs(a[0] * b[0]) + abs(a[1] * b[1]) + abs(a[2] * b[2])
    nn = math.sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]) * math.sqrt(b[0] * b[0] + b[1] * b[1] + b[2] * b[2])
    q = _div(dot, nn)
    aq = _div(adot, nn)
    return q, aq


def acos0(q):
    return math.acos(q) if -1.0 <= q <= 1.0 else 0.0


def angle_with_bound(q, eq):
    """acosf(q), NaN -> 0, with the bound that an error eq of q and acosf's own rounding allow."""
    if q != q:
        return 0.0, 0.0
    ang = acos0(q)
    lo, hi = acos0(q + eq), acos0(q - eq)  # q beyond +-1 by less than eq: float32 may still see NaN -> 0
    cand = [abs(lo - ang), abs(hi - ang)]
    if abs(q) + eq > 1.0:
        cand.append(ang)
    return ang, max(cand) + G[N_ACOS] * ang


def conf_float(conf_bytes, W, r, c):
    o = r * W + 4 * c
    b = conf_bytes[o:o + 4]
    b = b + b"\0" * (4 - len(b))
    return struct.unpack("<f", b)[0]


class Scene:
    """The loaded views of RunFusion (dicts as tests/fusion_lib.py builds them) in Python lists."""

    def __init__(self, views):
        self.views = views
        self.n = len(views)
        self.ids = [int(v["ref"]) for v in views]
        self.srcs = [[int(s) for s in v["srcs"]] for v in views]
        self.cam = []
        for v in views:
            c = v["cam"]
            self.cam.append(dict(K=[float(x) for x in c.K], R=[float(x) for x in c.R], t=[float(x) for x in c.t],
                                 c=[float(x) for x in c.c]))
        self.W = [int(v["depth"].shape[1]) for v in views]
        self.H = [int(v["depth"].shape[0]) for v in views]
        self.depth = [np.asarray(v["depth"], np.float64).reshape(-1).tolist() for v in views]
        self.normal = [np.asarray(v["normal"], np.float64).reshape(-1, 3).tolist() for v in views]
        self.weak = [np.asarray(v["weak"]).reshape(-1).tolist() for v in views]
        self.conf = [np.ascontiguousarray(v["conf"], np.uint8).tobytes() for v in views]
        self.bgr = [np.asarray(v["bgr"]).reshape(-1, 3).tolist() for v in views]
        self._memo = {}

    def index_of(self, image_id):
        """imageIdToindexMap: emplace keeps the first index of an id; operator[] of a missing id gives 0."""
        for i, x in enumerate(self.ids):
            if x == image_id:
                return i
        return 0

    def src_pixel(self, ref, src, p, g):
        """The rounded projection of pixel p of view ref into view src: (sp or -1, proj_depth, bound)."""
        W = self.W[ref]
        r, c = divmod(p, W)
        X, A = world_point(self.cam[ref], c, r, self.depth[ref][p])
        (px, py, pd), (apx, apy, apd) = project(self.cam[src], X, A)
        where = (ref, r, c, src)
        sr = g.trunc("round", py + 0.5, (apy + 0.5) * G[N_RND], where, self.H[src])
        sc = g.trunc("round", px + 0.5, (apx + 0.5) * G[N_RND], where, self.W[src])
        if sr is None or sc is None or not (0 <= sc < self.W[src] and 0 <= sr < self.H[src]):
            return -1, pd, apd * G[N_PD], X, A
        return sr * self.W[src] + sc, pd, apd * G[N_PD], X, A

    def candidate(self, ref, src, p, g):
        """Per-(pixel, source) quantities of :1166-1187 without the masks, memoised.
        dict(sp, dist, rel, angle, q and e_*) ; sp = -1 when out of bounds, None values then."""
        key = (ref, src, p)
        m = self._memo.get(key)
        if m is not None:
            return m
        sp, _pd, _epd, _X, _A = self.src_pixel(ref, src, p, g)
        out = dict(sp=sp, live=False)
        if sp >= 0:
            sd = self.depth[src][sp]
            out["src_depth"] = sd
            if not sd <= 0.0:
                W = self.W[ref]
                r, c = divmod(p, W)
                sr, sc = divmod(sp, self.W[src])
                d = self.depth[ref][p]
                Y, B = world_point(self.cam[src], sc, sr, sd)
                (tx, ty, td), (atx, aty, atd) = project(self.cam[ref], Y, B)
                dist = math.sqrt((c - tx) ** 2 + (r - ty) ** 2) if _finite(tx) and _finite(ty) else abs(tx - ty)
                e_dist = math.sqrt((c + atx) ** 2 + (r + aty) ** 2) * G[N_DIST] if _finite(atx + aty) else INF
                rel = _div(abs(td - d), d)
                e_rel = _div(atd + abs(d), abs(d)) * G[N_REL]
                q, aq = angle_q(self.normal[ref][p], self.normal[src][sp])
                e_q = aq * G[N_Q]
                ang, e_ang = angle_with_bound(q, e_q)
                out.update(live=True, at=(ref, r, c, src, sp), dist=dist, e_dist=e_dist, rel=rel, e_rel=e_rel, q=q, e_q=e_q, angle=ang,
                           e_angle=e_ang)
        self._memo[key] = out
        return out


def weak_vis_filter(sc, ref, g):
    """WeakVisFilter for one view: (skip flags, strong counters, weak counters), row-major lists."""
    W, H, n = sc.W[ref], sc.H[ref], sc.n
    skip, ns, nw = [0] * (W * H), [0] * (W * H), [0] * (W * H)
    rc, cref = sc.cam[ref], sc.cam[ref]["c"]
    for p in range(W * H):
        if sc.weak[ref][p] != WEAK:
            continue
        r, c = divmod(p, W)
        X, A = world_point(rc, c, r, sc.depth[ref][p])
        strong = weak = 0
        for s in range(n):
            if s == ref:
                continue
            cs = sc.cam[s]["c"]
            a = [cref[i] - X[i] for i in range(3)]
            b = [cs[i] - X[i] for i in range(3)]
            q, _ = angle_q(a, b)
            # absolute-value evaluation of the dot of differences
            aa = [abs(cref[i]) + A[i] for i in range(3)]
            ab = [abs(cs[i]) + A[i] for i in range(3)]
            nn = math.sqrt(sum(x * x for x in a)) * math.sqrt(sum(x * x for x in b))
            e_q = _div(sum(aa[i] * ab[i] for i in range(3)), nn) * G[N_VQ]
            ang, e_ang = angle_with_bound(q, e_q)
            deg = ang * 180.0 / math.pi
            e_deg = e_ang * 180.0 / math.pi + G[N_DEG] * deg
            where = (ref, r, c, s)
            if g.gt("view>80", deg, 80.0, e_deg, where):
                continue
            sp, pd, e_pd, _X, _A = sc.src_pixel(ref, s, p, g)
            if g.le("proj<=0", pd, 0.0, e_pd, where):
                continue
            if sp < 0:
                continue
            sd = sc.depth[s][sp]
            st = sc.weak[s][sp]
            if st == STRONG:
                if g.lt("occl", pd, sd - OCC * sd, e_pd + (abs(sd) + OCC * abs(sd)) * G[N_OCC], where):
                    strong += 1
            elif st == WEAK:
                sr, scol = divmod(sp, sc.W[s])
                if conf_float(sc.conf[s], sc.W[s], sr, scol) < conf_float(sc.conf[ref], W, r, c):  # exact bits
                    if g.lt("occl", pd, sd - OCC * sd, e_pd + (abs(sd) + OCC * abs(sd)) * G[N_OCC], where):
                        weak += 1
        ns[p], nw[p] = strong, weak
        if strong >= 2 or weak >= 4:
            skip[p] = 1
    return skip, ns, nw


def fuse(views, variant, weak_filter, reset_tat_cache=False, scene=None, guards=None):
    """The whole fusion. variant 0: RunFusion, 1: RunFusion_TAT_I, 2: RunFusion_TAT_A.
    Returns dict(order=[(problem i, view index, r, c)], xyz, e_xyz, col, e_col (float64 arrays), skips,
    strong, weak (per view lists), skip_weak (TAT_A's printed counts), guards, scene)."""
    sc = scene or Scene(views)
    g = guards or Guards()
    n = sc.n
    masks = [bytearray(sc.W[i] * sc.H[i]) for i in range(n)]
    skips = [[0] * (sc.W[i] * sc.H[i]) for i in range(n)]
    strong = [None] * n
    weakc = [None] * n
    if weak_filter:
        for i in range(n):
            skips[i], strong[i], weakc[i] = weak_vis_filter(sc, i, g)
    order, xyz, exyz, col, ecol = [], [], [], [], []
    skip_weak = []

    def emit(i, ref, p, colour):
        W = sc.W[ref]
        r, c = divmod(p, W)
        X, A = world_point(sc.cam[ref], c, r, sc.depth[ref][p])
        order.append((i, ref, r, c))
        xyz.append(X)
        exyz.append([a * G[N_X] for a in A])
        col.append(colour)
        ecol.append([abs(x) * G[N_COL] for x in colour])

    for i in range(n):
        ref = sc.index_of(sc.ids[i])
        src = [sc.index_of(s) for s in sc.srcs[i]]
        N = len(src)
        W, H = sc.W[ref], sc.H[ref]
        if variant == 0:
            for p in range(W * H):
                if masks[ref][p] == 1 or skips[ref][p] == 1:
                    continue
                d = sc.depth[ref][p]
                if d <= 0.0:
                    continue
                used = []
                dyn = e_dyn = 0.0
                for j in range(N):
                    cd = sc.candidate(ref, src[j], p, g)
                    if cd["sp"] < 0 or masks[src[j]][cd["sp"]] == 1 or not cd["live"]:
                        continue
                    wj = cd["at"]
                    if (g.lt("dist<2", cd["dist"], CUT_DIST, cd["e_dist"], wj)
                            and g.lt("rel<0.01", cd["rel"], CUT_REL, cd["e_rel"], wj)
                            and g.lt("angle<0.1745", cd["angle"], CUT_ANGLE, cd["e_angle"], wj)):
                        used.append((src[j], cd["sp"]))
                        t = cd["dist"] + 200.0 * cd["rel"] + cd["angle"] * 10.0
                        e_t = cd["e_dist"] + 200.0 * cd["e_rel"] + 10.0 * cd["e_angle"] + G[N_TMP] * t
                        term = math.exp(-t)
                        dyn += term
                        e_dyn += term * e_t + G[N_EXP] * term
                nc = len(used)
                if nc < 1:
                    continue
                factor = FACT_WEAK if sc.weak[ref][p] == WEAK else FACT_STRONG
                e_sum = e_dyn + G[nc] * dyn + G[N_FACT] * factor * nc  # nc - 1 additions, rounded up to nc
                if g.gt("sum>factor*n", dyn, factor * nc, e_sum, (ref,) + divmod(p, W)):
                    colour = [float(x) for x in sc.bgr[ref][p]]
                    for s, sp in used:
                        masks[s][sp] = 1
                        for k in range(3):
                            colour[k] += sc.bgr[s][sp][k]
                    emit(i, ref, p, [x / (nc + 1) for x in colour])
        else:
            db = DEPTH_BASE[variant]
            fresh = lambda: [dict(dist=FLT_MAX, e_dist=0.0, rel=FLT_MAX, e_rel=0.0, angle=FLT_MAX, e_angle=0.0,  # noqa: E731
                                  sp=0, at=None) for _ in range(N)]
            diff = fresh()
            nskip = 0
            for p in range(W * H):
                if skips[ref][p] == 1:
                    nskip += 1
                    continue
                d = sc.depth[ref][p]
                if d <= 0.0:
                    continue
                if reset_tat_cache:
                    diff = fresh()
                for j in range(N):
                    cd = sc.candidate(ref, src[j], p, g)
                    if cd["sp"] < 0 or masks[src[j]][cd["sp"]] == 1 or not cd["live"]:
                        continue
                    diff[j] = cd
                for k in range(2, N + 1):
                    use = []
                    for j in range(N):
                        e = diff[j]
                        wj = e["at"]  # the pixel the cached costs came from
                        ok = (g.lt("dist<k/4", e["dist"], k * DIST_BASE, e["e_dist"], wj)
                              and g.lt("rel<k*base", e["rel"], k * db, e["e_rel"] + G[N_KCUT] * k * db, wj))
                        if ok and variant == 1:
                            cut = k * ANGLE_GRAD + ANGLE_BASE
                            ok = g.lt("angle<k*grad+base", e["angle"], cut, e["e_angle"] + G[N_ACUT] * cut, wj)
                        if ok:
                            use.append(j)
                    if len(use) >= k:
                        colour = [float(x) for x in sc.bgr[ref][p]]
                        if variant == 1:
                            for j in use:
                                for q in range(3):
                                    colour[q] += sc.bgr[src[j]][diff[j]["sp"]][q]
                            colour = [x / (len(use) + 1.0) for x in colour]
                        emit(i, ref, p, colour)
                        masks[ref][p] = 1
                        break
            skip_weak.append(nskip)
    return dict(order=order, xyz=np.array(xyz, np.float64).reshape(-1, 3), e_xyz=np.array(exyz).reshape(-1, 3),
                col=np.array(col, np.float64).reshape(-1, 3), e_col=np.array(ecol).reshape(-1, 3), skips=skips,
                strong=strong, weak=weakc, skip_weak=skip_weak, guards=g, scene=sc,
                masks=[bytes(m) for m in masks])


def candidates(sc, ref, src_idx, g):
    """Arrays (H, W, len(src_idx)) of sp, dist, rel, angle, q and their bounds; the per-(pixel, source)
    values of the three fusion loops without masks. sp = -1: out of bounds or source depth <= 0."""
    H, W, N = sc.H[ref], sc.W[ref], len(src_idx)
    out = {k: np.zeros((H * W, N)) for k in ("dist", "rel", "angle", "q", "e_dist", "e_rel", "e_angle", "e_q")}
    sp = np.full((H * W, N), -1, np.int64)
    for p in range(H * W):
        if sc.depth[ref][p] <= 0.0:
            continue
        for j, s in enumerate(src_idx):
            cd = sc.candidate(ref, s, p, g)
            if cd["live"]:
                sp[p, j] = cd["sp"]
                for k in out:
                    out[k][p, j] = cd[k]
    out = {k: v.reshape(H, W, N) for k, v in out.items()}
    out["sp"] = sp.reshape(H, W, N)
    return out


def decisions(sc, ref, src_idx, g):
    """What the device entry points decide per (pixel, source), without masks: RunFusion's consistent
    / not, and the smallest TAT level k in [2, N] the candidate passes (255: none) for TAT_I and
    TAT_A. Every comparison is recorded in g."""
    H, W, N = sc.H[ref], sc.W[ref], len(src_idx)
    cons = np.zeros((H * W, N), bool)
    lv = {1: np.full((H * W, N), 255, np.uint8), 2: np.full((H * W, N), 255, np.uint8)}
    for p in range(H * W):
        if sc.depth[ref][p] <= 0.0:
            continue
        for j, s in enumerate(src_idx):
            cd = sc.candidate(ref, s, p, g)
            if not cd["live"]:
                continue
            at = cd["at"]
            cons[p, j] = (g.lt("dist<2", cd["dist"], CUT_DIST, cd["e_dist"], at)
                          and g.lt("rel<0.01", cd["rel"], CUT_REL, cd["e_rel"], at)
                          and g.lt("angle<0.1745", cd["angle"], CUT_ANGLE, cd["e_angle"], at))
            for variant in (1, 2):
                db = DEPTH_BASE[variant]
                for k in range(2, N + 1):
                    ok = (g.lt("dist<k/4", cd["dist"], k * DIST_BASE, cd["e_dist"], at)
                          and g.lt("rel<k*base", cd["rel"], k * db, cd["e_rel"] + G[N_KCUT] * k * db, at))
                    if ok and variant == 1:
                        cut = k * ANGLE_GRAD + ANGLE_BASE
                        ok = g.lt("angle<k*grad+base", cd["angle"], cut, cd["e_angle"] + G[N_ACUT] * cut, at)
                    if ok:
                        lv[variant][p, j] = k
                        break
    return cons.reshape(H, W, N), lv[1].reshape(H, W, N), lv[2].reshape(H, W, N)


def ply_colour_bytes(col, e_col):
    """ExportPointCloud's static_cast<uchar>: truncation. Returns (bytes, decided) where decided marks
    colours farther than the bound from an integer (a float32 quotient truncates to the same byte)."""
    t = np.floor(col)
    near = np.rint(col)
    return t.astype(np.uint8), np.abs(col - near) > e_col
