"""numpy / plain-Python restatement of include/apd_seg.h's five stages, written from the contract's
text, and the generators of the masks and images the segmentation tests share. The labelling is a
sequential union-find over the raster; fast enough for images up to about 200 x 140.
Test infrastructure only."""
from __future__ import annotations

import numpy as np

MAX_LABELS = 255


# ---- the contract ------------------------------------------------------------------------------------------

def working_size(w, h, max_size):
    m = max(w, h)
    s = 1 if max_size == 0 or m <= max_size else -(-m // max_size)
    return s, -(-w // s), -(-h // s)


def downscale(bgr, max_size):
    h, w = bgr.shape[:2]
    s, W, H = working_size(w, h, max_size)
    if s == 1:
        return bgr.copy()
    pad = np.zeros((H * s, W * s, 3), np.int64)
    pad[:h, :w] = bgr
    one = np.zeros((H * s, W * s), np.int64)
    one[:h, :w] = 1
    total = pad.reshape(H, s, W, s, 3).sum((1, 3))
    cnt = one.reshape(H, s, W, s).sum((1, 3))[..., None]
    return ((2 * total + cnt) // (2 * cnt)).astype(np.uint8)


def smooth(work):
    """(H, W, 3) uint8 -> (3, H, W) uint16, 256 x the smoothed level"""
    a = work.astype(np.int64).transpose(2, 0, 1)
    k = (1, 4, 6, 4, 1)
    H, W = a.shape[1:]
    p = np.pad(a, ((0, 0), (0, 0), (2, 2)), mode="edge")
    t = sum(k[i] * p[:, :, i:i + W] for i in range(5))
    p = np.pad(t, ((0, 0), (2, 2), (0, 0)), mode="edge")
    s = sum(k[i] * p[:, i:i + H, :] for i in range(5))
    assert s.max() <= 65280
    return s.astype(np.uint16)


def flatness(S, threshold_q8):
    """g(p) <= threshold_q8, as uint8"""
    s = S.astype(np.int64)
    _, H, W = s.shape
    g = np.zeros((H, W), np.int64)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx == 0 and dy == 0:
                continue
            # the pixels p = (y, x) whose neighbour q = (y + dy, x + dx) is inside
            y0, y1 = max(0, -dy), min(H, H - dy)
            x0, x1 = max(0, -dx), min(W, W - dx)
            if y1 <= y0 or x1 <= x0:
                continue
            d = np.abs(s[:, y0:y1, x0:x1] - s[:, y0 + dy:y1 + dy, x0 + dx:x1 + dx]).max(0)
            g[y0:y1, x0:x1] = np.maximum(g[y0:y1, x0:x1], d)
    return (g <= threshold_q8).astype(np.uint8)


def label_mask(mask):
    """(H, W), non-zero = set -> int32 roots: the smallest linear index of the 4-connected component, -1 off it"""
    m = np.asarray(mask) != 0
    H, W = m.shape
    flat = m.ravel().tolist()
    parent = list(range(H * W))

    def find(a):
        r = a
        while parent[r] != r:
            r = parent[r]
        while parent[a] != r:
            parent[a], a = r, parent[a]
        return r

    for i, on in enumerate(flat):
        if not on:
            continue
        x = i % W
        for j in ((i - 1) if x > 0 else -1, i - W):
            if j >= 0 and flat[j]:
                a, b = find(i), find(j)
                if a != b:
                    parent[max(a, b)] = min(a, b)
    out = np.full(H * W, -1, np.int32)
    for i, on in enumerate(flat):
        if on:
            out[i] = find(i)
    return out.reshape(H, W)


def rank(roots, min_area):
    """-> (labels uint8, n_survivors, n_labels, areas int32 by root)"""
    r = roots.ravel()
    areas = np.bincount(r[r >= 0], minlength=r.size).astype(np.int32)
    surv = [(-int(areas[i]), int(i)) for i in np.nonzero(areas >= min_area)[0]]
    surv.sort()  # area descending, then root ascending
    lut = np.zeros(r.size + 1, np.uint8)  # the last entry serves the root -1
    for k, (_, root) in enumerate(surv[:MAX_LABELS]):
        lut[root] = k + 1
    labels = lut[r].reshape(roots.shape)
    return labels, len(surv), min(len(surv), MAX_LABELS), areas.reshape(roots.shape)


def flat_zones(bgr, max_size=2560, threshold_q8=256, min_area=256):
    """-> (labels, n_survivors, n_labels, stages) with stages as apd_abi.seg_flat_zones_host(stages=True) has them"""
    work = downscale(np.asarray(bgr, np.uint8), max_size)
    S = smooth(work)
    flat = flatness(S, threshold_q8)
    roots = label_mask(flat)
    labels, ns, nl, areas = rank(roots, min_area)
    return labels, ns, nl, {"work": work, "smooth": S, "flat": flat, "roots": roots, "areas": areas}


def colour(k):
    """(B, G, R) of label k in the picture"""
    return (255, 255, 255) if k == 0 else ((37 * k + 11) % 224, (91 * k + 53) % 224, (151 * k + 101) % 224)


# ---- masks -------------------------------------------------------------------------------------------------

def spiral(H, W, gap=1, start=(0, 0), avoid=None):
    """A one-pixel-wide spiral walked from `start` to the right and inwards, clockwise: straight on while the
    next cell is inside, the gap + 1 cells ahead are free of the path and the 2 cells ahead are free of
    `avoid`; else one turn to the right; else the end."""
    m = np.zeros((H, W), np.uint8)
    y, x = start
    dy, dx = 0, 1
    m[y, x] = 1

    def can_go(dy, dx):
        if not (0 <= y + dy < H and 0 <= x + dx < W):
            return False
        for k in range(1, gap + 2):
            yy, xx = y + k * dy, x + k * dx
            if 0 <= yy < H and 0 <= xx < W and (m[yy, xx] or (avoid is not None and k <= 2 and avoid[yy, xx])):
                return False
        return True

    while True:
        if not can_go(dy, dx):
            dy, dx = dx, -dy  # right -> down -> left -> up
            if not can_go(dy, dx):
                return m
        y, x = y + dy, x + dx
        m[y, x] = 1


def two_spirals(H, W):
    """Two spirals with three free pixels between a spiral's own turns, the second in the first's middle lane"""
    first = spiral(H, W, 3)
    if H < 3 or W < 3:
        return first
    m = np.maximum(first, spiral(H, W, 3, (2, 2), first))
    m[H // 2 - 5:H // 2 + 6, W // 2 - 8:W // 2 + 9] = 0  # where the walks end they may touch: cut the centre out
    return m


def serpentine(H, W):
    """A path that covers every other row and turns at alternate ends: one component through the whole image."""
    m = np.zeros((H, W), np.uint8)
    m[0::2] = 1
    for k, y in enumerate(range(1, H, 2)):
        m[y, W - 1 if k % 2 == 0 else 0] = 1
    return m


def comb(H, W):
    m = np.zeros((H, W), np.uint8)
    m[H - 1] = 1
    m[:, 0::2] = 1
    return m


def checkerboard(H, W):
    y, x = np.mgrid[0:H, 0:W]
    return ((x + y) % 2 == 0).astype(np.uint8)


def mask_cases(H, W, seed=0):
    """name -> mask, every shape of the issue at one size"""
    rng = np.random.default_rng(seed)
    cases = {
        "zeros": np.zeros((H, W), np.uint8),
        "ones": np.ones((H, W), np.uint8),
        "checkerboard": checkerboard(H, W),
        "spiral": spiral(H, W),
        "serpentine": serpentine(H, W),
        "two_spirals": two_spirals(H, W),
        "comb": comb(H, W),
    }
    for d in (0.3, 0.59, 0.8):
        cases["random_%g" % d] = (rng.random((H, W)) < d).astype(np.uint8)
    # non-zero means set, whatever the value
    cases["random_0.59"] = cases["random_0.59"] * rng.integers(1, 256, (H, W)).astype(np.uint8)
    return cases


# ---- images ------------------------------------------------------------------------------------------------

def patches_image(h, w, seed, patch=24, noise=2):
    """Constant patches of random colour plus uniform noise of +-noise levels"""
    rng = np.random.default_rng(seed)
    ny, nx = -(-h // patch), -(-w // patch)
    base = rng.integers(20, 236, (ny, nx, 3))
    img = np.repeat(np.repeat(base, patch, 0), patch, 1)[:h, :w]
    return np.clip(img + rng.integers(-noise, noise + 1, (h, w, 3)), 0, 255).astype(np.uint8)


def gradient_image(h, w, seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    chans = [127.5 + 100 * np.sin(x / rng.uniform(30, 90) + y / rng.uniform(30, 90) + rng.uniform(0, 6)) for _ in range(3)]
    return np.clip(np.stack(chans, -1), 0, 255).astype(np.uint8)


def random_image(h, w, seed):
    """Smooth noise: patches of several sizes added up, so that every stage has something to say"""
    rng = np.random.default_rng(seed)
    img = np.zeros((h, w, 3))
    for patch, amp in ((32, 90), (9, 30), (1, 3)):
        ny, nx = -(-h // patch), -(-w // patch)
        img += np.repeat(np.repeat(rng.uniform(0, amp, (ny, nx, 3)), patch, 0), patch, 1)[:h, :w]
    return np.clip(img, 0, 255).astype(np.uint8)


def step_image(h, w, c, lo=100, delta=16):
    """Columns < c at lo, columns >= c at lo + delta, all channels"""
    img = np.full((h, w, 3), lo, np.uint8)
    img[:, c:] = lo + delta
    return img


def ramp_image(h, w, slope):
    return np.repeat((np.arange(w) * slope)[None, :, None], h, 0).repeat(3, 2).astype(np.uint8)


def squares_image(n=17):
    """n x n constant rectangles on a grid: row i is 10 + i pixels high, column j is 10 + j pixels wide, the
    levels alternate between 30 and 230 like a chessboard's. 306 x 306 for n = 17. (n * n distinct areas with
    every side at least 10 do not fit in about 200 x 200; here rectangle (i, j) and rectangle (j, i) have
    the same area, so that the order of equal areas by root is needed inside the first 255 as well.)"""
    sides = np.arange(10, 10 + n)
    edges = np.concatenate([[0], np.cumsum(sides)])
    img = np.zeros((edges[-1], edges[-1], 3), np.uint8)
    for i in range(n):
        for j in range(n):
            img[edges[i]:edges[i + 1], edges[j]:edges[j + 1]] = 30 if (i + j) % 2 == 0 else 230
    return img


# (name, maker, max_size, threshold_q8, min_area): what the host twin and the device are compared on
IMAGE_CASES = [("patches", lambda: patches_image(61, 97, 1), 0, 256, 16),
               ("patches/s=3", lambda: patches_image(140, 200, 2, patch=48), 70, 256, 16),
               ("patches/s=2/threshold-0.5", lambda: patches_image(75, 131, 3, patch=30, noise=1), 66, 128, 4),
               ("gradient", lambda: gradient_image(90, 120, 4), 0, 256, 8),
               ("gradient/s=2", lambda: gradient_image(121, 95, 5), 64, 1024, 1),
               ("random", lambda: random_image(83, 117, 6), 0, 256, 2),
               ("random/s=3", lambda: random_image(200, 139, 7), 70, 300, 1),
               ("noise", lambda: np.random.default_rng(8).integers(0, 256, (40, 50, 3)).astype(np.uint8), 0, 5000, 1)]
# the images of the known answers, at s = 1
KNOWN_CASES = [("constant", lambda: np.full((30, 40, 3), 77, np.uint8), 0, 256, 1),
               ("step/256", lambda: step_image(12, 50, 20), 0, 256, 1),
               ("step/255", lambda: step_image(12, 50, 20), 0, 255, 1),
               ("step/equal-areas", lambda: step_image(12, 40, 20), 0, 256, 1),
               ("ramp-1", lambda: ramp_image(9, 100, 1), 0, 256, 1),
               ("ramp-2/352", lambda: ramp_image(9, 100, 2), 0, 352, 1),
               ("constant/min_area+1", lambda: np.full((30, 40, 3), 77, np.uint8), 0, 256, 1201),
               ("squares", squares_image, 0, 256, 1),
               ("squares/s=3", squares_image, 102, 256, 1)]
