"""The undistortion contract of include/apd_prep.h restated in numpy, operation for operation: atan_c,
the forward functions of COLMAP's camera models, the 1/256 fixed-point bilinear warp with a black
border (int64), and a Newton inverse of the forward function that is the tests' own. Doubles
throughout; numpy evaluates sums and products as written and never contracts them."""
import os
import struct

import numpy as np

f64 = np.float64

# name: (COLMAP id, parameter count)
MODELS = {"SIMPLE_PINHOLE": (0, 3), "PINHOLE": (1, 4), "SIMPLE_RADIAL": (2, 4), "RADIAL": (3, 5), "OPENCV": (4, 8),
          "OPENCV_FISHEYE": (5, 8), "FULL_OPENCV": (6, 12), "SIMPLE_RADIAL_FISHEYE": (8, 4), "RADIAL_FISHEYE": (9, 5),
          "THIN_PRISM_FISHEYE": (10, 12)}
DISTORTED = [m for m in MODELS if "PINHOLE" not in m]
ONE_F = ("SIMPLE_PINHOLE", "SIMPLE_RADIAL", "RADIAL", "SIMPLE_RADIAL_FISHEYE", "RADIAL_FISHEYE")

ATAN_HI = [4.63647609000806093515e-01, 7.85398163397448278999e-01, 9.82793723247329054082e-01, 1.57079632679489655800e+00]
ATAN_LO = [2.26987774529616870924e-17, 3.06161699786838301793e-17, 1.39033110312309984516e-17, 6.12323399573676603587e-17]
AT = [3.33333333333329318027e-01, -1.99999999998764832476e-01, 1.42857142725034663711e-01, -1.11111104054623557880e-01,
      9.09088713343650656196e-02, -7.69187620504482999495e-02, 6.66107313738753120669e-02, -5.83357013379057348645e-02,
      4.97687799461593236017e-02, -3.65315727442169155270e-02, 1.62858201153657823623e-02]
# where atan_c changes its path
ATAN_BREAKS = [2.0 ** -29, 0.4375, 0.6875, 1.1875, 2.4375, 2.0 ** 66]


def atan_c(x):
    """The contract's arctangent of x >= 0, elementwise."""
    x = np.asarray(x, f64)
    with np.errstate(all="ignore"):
        big = x >= 2.0 ** 66
        tiny = x < 2.0 ** -29
        b0 = x < 0.4375
        b1 = ~b0 & (x < 0.6875)
        b2 = ~b0 & ~b1 & (x < 1.1875)
        b3 = ~b0 & ~b1 & ~b2 & (x < 2.4375)
        t = np.where(b0, x, np.where(b1, (2.0 * x - 1.0) / (2.0 + x), np.where(
            b2, (x - 1.0) / (x + 1.0), np.where(b3, (x - 1.5) / (1.0 + 1.5 * x), -1.0 / x))))
        hi = np.where(b1, ATAN_HI[0], np.where(b2, ATAN_HI[1], np.where(b3, ATAN_HI[2], ATAN_HI[3])))
        lo = np.where(b1, ATAN_LO[0], np.where(b2, ATAN_LO[1], np.where(b3, ATAN_LO[2], ATAN_LO[3])))
        z = t * t
        w = z * z
        s1 = z * (AT[0] + w * (AT[2] + w * (AT[4] + w * (AT[6] + w * (AT[8] + w * AT[10])))))
        s2 = w * (AT[1] + w * (AT[3] + w * (AT[5] + w * (AT[7] + w * AT[9]))))
        r = np.where(b0, t - t * (s1 + s2), hi - ((t * (s1 + s2) - lo) - t))
        r = np.where(tiny, x, r)
        return np.where(big, f64(ATAN_HI[3]) + f64(ATAN_LO[3]), r)


def intrinsics(model, params):
    """(fx, fy, cx, cy, the parameters after them)"""
    p = [f64(v) for v in params]
    assert len(p) == MODELS[model][1], (model, len(p))
    return (p[0], p[0], p[1], p[2], p[3:]) if model in ONE_F else (p[0], p[1], p[2], p[3], p[4:])


def forward(model, params, u, v):
    """normalised pinhole (u, v) -> normalised distorted (ud, vd), elementwise"""
    k = intrinsics(model, params)[4]
    u, v = np.asarray(u, f64), np.asarray(v, f64)
    with np.errstate(all="ignore"):
        if model in ("SIMPLE_PINHOLE", "PINHOLE"):
            return u, v
        r2 = u * u + v * v
        if model == "SIMPLE_RADIAL":
            rad = k[0] * r2
            return u + u * rad, v + v * rad
        if model == "RADIAL":
            rad = k[0] * r2 + (k[1] * r2) * r2
            return u + u * rad, v + v * rad
        if model == "OPENCV":
            k1, k2, p1, p2 = k
            rad = k1 * r2 + (k2 * r2) * r2
            return (u + ((u * rad + ((2.0 * p1) * u) * v) + p2 * (r2 + (2.0 * u) * u)),
                    v + ((v * rad + ((2.0 * p2) * u) * v) + p1 * (r2 + (2.0 * v) * v)))
        if model == "FULL_OPENCV":
            k1, k2, p1, p2, k3, k4, k5, k6 = k
            g = (1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))) / (1.0 + r2 * (k4 + r2 * (k5 + r2 * k6)))
            return ((u * g + ((2.0 * p1) * u) * v) + p2 * (r2 + (2.0 * u) * u),
                    (v * g + ((2.0 * p2) * u) * v) + p1 * (r2 + (2.0 * v) * v))
        r = np.sqrt(r2)
        s = np.where(r2 == 0.0, f64(1.0), atan_c(r) / r)
        a, b = u * s, v * s
        t2 = a * a + b * b
        if model == "SIMPLE_RADIAL_FISHEYE":
            rad = k[0] * t2
            return a + a * rad, b + b * rad
        if model == "RADIAL_FISHEYE":
            rad = k[0] * t2 + (k[1] * t2) * t2
            return a + a * rad, b + b * rad
        if model == "OPENCV_FISHEYE":
            k1, k2, k3, k4 = k
            rad = t2 * (k1 + t2 * (k2 + t2 * (k3 + t2 * k4)))
            return a + a * rad, b + b * rad
        assert model == "THIN_PRISM_FISHEYE"
        k1, k2, p1, p2, k3, k4, sx1, sy1 = k
        rad = t2 * (k1 + t2 * (k2 + t2 * (k3 + t2 * k4)))
        return (a + (((a * rad + ((2.0 * p1) * a) * b) + p2 * (t2 + (2.0 * a) * a)) + sx1 * t2),
                b + (((b * rad + ((2.0 * p2) * a) * b) + p1 * (t2 + (2.0 * b) * b)) + sy1 * t2))


def source_coords(model, params, out_K, out_w, out_h):
    """(sx, sy) of every output pixel, (out_h, out_w) doubles each"""
    fx, fy, cx, cy, _ = intrinsics(model, params)
    ofx, ofy, ocx, ocy = [f64(v) for v in out_K]
    x = np.arange(out_w, dtype=f64)[None, :] + np.zeros((out_h, 1), f64)
    y = np.arange(out_h, dtype=f64)[:, None] + np.zeros((1, out_w), f64)
    with np.errstate(all="ignore"):
        u = ((x + 0.5) - ocx) / ofx
        v = ((y + 0.5) - ocy) / ofy
        ud, vd = forward(model, params, u, v)
        return (fx * ud + cx) - 0.5, (fy * vd + cy) - 0.5


def pinhole_K(model, params):
    return [float(v) for v in intrinsics(model, params)[:4]]


def warp(bgr, model, params, out_K=None, out_size=None, details=False):
    """The contract's warp of a (h, w, 3) uint8 image. details: also (inside, all four taps inside)."""
    src = np.asarray(bgr, np.uint8)
    sh, sw = src.shape[:2]
    out_K = pinhole_K(model, params) if out_K is None else out_K
    ow, oh = (sw, sh) if out_size is None else out_size
    sx, sy = source_coords(model, params, out_K, ow, oh)
    with np.errstate(all="ignore"):
        inside = (sx > -1.0) & (sx < f64(sw)) & (sy > -1.0) & (sy < f64(sh))  # a NaN compares false
    sxs, sys_ = np.where(inside, sx, 0.0), np.where(inside, sy, 0.0)
    fxi, fyi = np.floor(sxs), np.floor(sys_)
    ix, iy = fxi.astype(np.int64), fyi.astype(np.int64)
    wx = np.floor((sxs - fxi) * 256.0 + 0.5).astype(np.int64)
    wy = np.floor((sys_ - fyi) * 256.0 + 0.5).astype(np.int64)
    padded = np.zeros((sh + 2, sw + 2, 3), np.int64)  # a tap outside the image is 0
    padded[1:-1, 1:-1] = src
    t00, t10 = padded[iy + 1, ix + 1], padded[iy + 1, ix + 2]
    t01, t11 = padded[iy + 2, ix + 1], padded[iy + 2, ix + 2]
    wx, wy = wx[..., None], wy[..., None]
    val = (t00 * (256 - wx) * (256 - wy) + t10 * wx * (256 - wy) + t01 * (256 - wx) * wy + t11 * wx * wy + 32768) >> 16
    out = np.where(inside[..., None], val, 0).astype(np.uint8)
    if details:
        full = inside & (ix >= 0) & (ix + 1 < sw) & (iy >= 0) & (iy + 1 < sh)
        return out, inside, full
    return out


def invert(model, params, ud, vd, steps=60):
    """The tests' own inverse of forward(): Newton with a central-difference Jacobian from (ud, vd),
    elementwise, a fixed number of steps. Where it has not converged the result is NaN."""
    ud, vd = np.asarray(ud, f64), np.asarray(vd, f64)
    u, v = ud.copy(), vd.copy()
    h = 1e-6
    with np.errstate(all="ignore"):
        for _ in range(steps):
            f0, f1 = forward(model, params, u, v)
            a0, b0 = forward(model, params, u - h, v)
            a1, b1 = forward(model, params, u + h, v)
            c0, d0 = forward(model, params, u, v - h)
            c1, d1 = forward(model, params, u, v + h)
            j00, j10, j01, j11 = (a1 - a0) / (2 * h), (b1 - b0) / (2 * h), (c1 - c0) / (2 * h), (d1 - d0) / (2 * h)
            e0, e1 = f0 - ud, f1 - vd
            det = j00 * j11 - j01 * j10
            u = u - (j11 * e0 - j01 * e1) / det
            v = v - (j00 * e1 - j10 * e0) / det
        f0, f1 = forward(model, params, u, v)
        ok = (np.abs(f0 - ud) < 1e-9) & (np.abs(f1 - vd) < 1e-9)
    return np.where(ok, u, np.nan), np.where(ok, v, np.nan)


def distort_pixels(model, params, x, y):
    """pinhole pixel coordinates -> distorted pixel coordinates of the same camera"""
    fx, fy, cx, cy, _ = intrinsics(model, params)
    ud, vd = forward(model, params, (np.asarray(x, f64) - cx) / fx, (np.asarray(y, f64) - cy) / fy)
    return fx * ud + cx, fy * vd + cy


def undistort_pixels(model, params, x, y):
    """distorted pixel coordinates -> pinhole pixel coordinates (NaN where there is no inverse)"""
    fx, fy, cx, cy, _ = intrinsics(model, params)
    u, v = invert(model, params, (np.asarray(x, f64) - cx) / fx, (np.asarray(y, f64) - cy) / fy)
    return fx * u + cx, fy * v + cy


# ---- shared cases -------------------------------------------------------------------------------------

F, CX, CY = 50.0, 30.5, 22.25  # principal point off the centre of 64 x 48
# moderate coefficients of both signs
COEFFS = {"SIMPLE_RADIAL": [-0.12], "RADIAL": [0.1, -0.03], "OPENCV": [-0.15, 0.05, 0.004, -0.003],
          "OPENCV_FISHEYE": [0.05, -0.02, 0.004, -0.001],
          "FULL_OPENCV": [-0.15, 0.05, 0.004, -0.003, 0.01, 0.02, -0.01, 0.003],
          "SIMPLE_RADIAL_FISHEYE": [0.03], "RADIAL_FISHEYE": [0.03, -0.01],
          "THIN_PRISM_FISHEYE": [0.05, -0.02, 0.004, -0.003, 0.004, -0.001, 0.002, -0.002],
          "SIMPLE_PINHOLE": [], "PINHOLE": []}


def camera(model, coeffs=None, f=F, cx=CX, cy=CY):
    """The parameter list of a model: f (or f, 1.02 f), the principal point, the coefficients."""
    k = COEFFS[model] if coeffs is None else list(coeffs)
    head = [f, cx, cy] if model in ONE_F else [f, 1.02 * f, cx, cy]
    return head + [float(c) for c in k]


def overflow_camera(model):
    """Coefficients that, seen through OVERFLOW_K, drive the source coordinates beyond +-1e300, to
    infinity and to NaN (0 * inf on the column u = 0, inf - inf elsewhere)."""
    n = len(COEFFS[model])
    return camera(model, [(1.7e308 if k % 2 == 0 else -1.7e308) for k in range(n)])


OVERFLOW_K = [10.0, 10.0, CX, CY]  # r2 > 1 in the corners: the products overflow there


def warp_cases(models):
    """(label, model, params, (src_h, src_w), out_K or None, out_size or None) for each model: the plain
    64x48 warp, an output camera whose corners fall outside the source, another output size, 1x1 and
    3x2 sources, and the overflowing coefficients."""
    out = []
    for m in models:
        p = camera(m)
        out += [(m + "/plain", m, p, (48, 64), None, None),
                (m + "/corners-outside", m, p, (48, 64), [20.0, 20.0, CX, CY], None),
                (m + "/other-size", m, p, (48, 64), [40.0, 41.0, 20.0, 15.0], (41, 29)),
                (m + "/1x1", m, camera(m, cx=0.5, cy=0.5), (1, 1), [F, F, 2.5, 2.0], (5, 4)),
                (m + "/3x2", m, camera(m, cx=1.25, cy=1.0), (2, 3), [F, F, 3.5, 1.5], (7, 3))]
        if m in DISTORTED:
            out.append((m + "/overflow", m, overflow_camera(m), (48, 64), OVERFLOW_K, None))
    return out


def write_cameras_bin(path, cameras):
    """cameras.bin with any model id (dicts id, model, width, height, params)"""
    with open(path, "wb") as fh:
        fh.write(struct.pack("<Q", len(cameras)))
        for c in cameras:
            mid = c["model"] if isinstance(c["model"], int) else {**{m: i for m, (i, _) in MODELS.items()}, "FOV": 7}[c["model"]]
            fh.write(struct.pack("<iiQQ", c["id"], mid, c["width"], c["height"]))
            fh.write(struct.pack("<%dd" % len(c["params"]), *[float(p) for p in c["params"]]))


def write_cameras_txt(path, cameras):
    with open(path, "w") as fh:
        fh.write("# Camera list with one line of data per camera:\n")
        for c in cameras:
            fh.write("%d %s %d %d %s\n" % (c["id"], c["model"], c["width"], c["height"],
                                          " ".join(repr(float(p)) for p in c["params"])))
