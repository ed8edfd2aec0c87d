"""Pixel-value patterns for the shrink kernels (tests/test_value_domain_host.py, tests/test_gpu_value_domain.py).

The parity suites feed the shrink side smooth ramps plus noise, with alpha at 255 or in 128..255.  The tiles below sit at the
ends of the value domain instead: 0/255 edges, stripes at the ringing period of the wide filters, impulses (the horizontal
pass overshoots and is clamped, then the vertical pass overshoots again), and alpha in 0..3 and around 127/128 and 254/255,
where the reciprocal table's multiplier is large and a resampled colour byte can exceed its resampled alpha.  What the
patterns make the oracle do is asserted in test_value_domain_host.py, without the code under test.

Everything here is pure numpy and deterministic: the noise is a hash of the pixel index, no generator state is involved."""
import numpy as np

OPAQUE = ("checker 2", "v stripes 2", "h stripes 2", "v stripes 6", "h stripes 6", "blocks 3", "v step", "h step", "corner step",
          "white pixel", "black pixel", "noise", "v stripes 6 dither", "h stripes 6 dither")
ALPHA = ("alpha 1..3", "alpha extremes", "alpha checker 0/255", "alpha checker 254/255", "alpha ramp across", "alpha ramp down",
         "opaque pixel", "transparent pixel", "stripes alpha 3/255", "white alpha 1")
FLAT = ("white alpha 1",)                                 # both detectors give 0: stored at 1x1 whatever the factor
PERIOD_2 = ("checker 2", "v stripes 2", "h stripes 2")   # every 3x3 Sobel window sums to 0: flat to the directional detector
# one axis constant: the directional detector gives 0 on that axis, the other one walks the levels (alpha is not looked at).
# v: columns differ (rows are equal), h: rows differ
VARIES_ACROSS = ("v stripes 6", "v step", "alpha ramp across", "stripes alpha 3/255")
VARIES_DOWN = ("h stripes 6", "h step", "alpha ramp down")
DITHERED = ("v stripes 6 dither", "h stripes 6 dither")
# edges along both axes, the same strength on either: the directional detector keeps their tiles square
# (the corner step's two edges are as long as half a side each: the same strength in square tiles only)
SQUARE_IN_MODE_1 = ("blocks 3", "corner step", "white pixel", "black pixel")

# Amplitude of the dither on the stripe-6 tiles (see dither()): the strong axis is capped at level 0 from a factor of ~1.5 on,
# while the weak axis, ~ DITHER / 4096 of it, walks the levels one by one as the factor goes on growing.
DITHER = 2


def hash32(i, seed):
    """murmur3's finaliser over index i (any integer array) xor a seed: uint32, the same on every numpy"""
    h = (np.asarray(i, np.uint64) ^ np.uint64(seed & 0xFFFFFFFF)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85EBCA6B)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xC2B2AE35)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(16)
    return h.astype(np.uint32)


def noise(bw, bh, seed, planes=3):
    """0/255 drawn independently per pixel and channel: [bh, bw, planes] uint8"""
    i = np.arange(bh * bw * planes, dtype=np.uint64).reshape(bh, bw, planes)
    return ((hash32(i, seed) >> 7) & 1).astype(np.uint8) * 255


def pick(bw, bh, seed, values):
    """one of `values` per pixel: [bh, bw] uint8"""
    i = np.arange(bh * bw, dtype=np.uint64).reshape(bh, bw)
    return np.asarray(values, np.uint8)[(hash32(i, seed) >> 5) % len(values)]


def dither(n):
    """n small offsets in 0..DITHER along one axis, no period of two (a period-2 ripple is flat to a 3x3 Sobel window)"""
    return ((hash32(np.arange(n, dtype=np.uint64), 0xD17) >> 9) % (DITHER + 1)).astype(np.int32)


def mono(mask):
    """bool [bh, bw] -> 0/255 in three equal channels"""
    return np.repeat((mask.astype(np.uint8) * 255)[:, :, None], 3, axis=2)


def patterns(bw, bh, channels):
    """[(name, tile [bh, bw, channels] uint8)]: the opaque tiles (alpha 255 when channels == 4), then, RGBA only, the alpha tiles"""
    assert channels in (3, 4) and bw >= 2 and bh >= 2
    y, x = np.mgrid[0:bh, 0:bw]
    seed = bw * 4099 + bh * 17
    vs6, hs6 = ((x // 3) & 1) == 1, ((y // 3) & 1) == 1
    rgb = {
        "checker 2": mono(((x + y) & 1) == 1),
        "v stripes 2": mono((x & 1) == 1),
        "h stripes 2": mono((y & 1) == 1),
        "v stripes 6": mono(vs6),
        "h stripes 6": mono(hs6),
        "blocks 3": mono((((x // 3) + (y // 3)) & 1) == 1),
        "v step": mono(x >= bw // 2),
        "h step": mono(y >= bh // 2),
        "corner step": mono((x >= bw // 2) & (y >= bh // 2)),
        "white pixel": mono((x == bw // 2) & (y == bh // 2)),
        "black pixel": mono(~((x == bw // 2) & (y == bh // 2))),
        "noise": noise(bw, bh, seed + 1),
    }
    # the dither moves black up and white down, so that nothing clips: rows (columns) differ by at most DITHER
    dy, dx = dither(bh)[:, None, None], dither(bw)[None, :, None]
    v, h = rgb["v stripes 6"].astype(np.int32), rgb["h stripes 6"].astype(np.int32)
    rgb["v stripes 6 dither"] = np.where(v == 0, v + dy, v - dy).astype(np.uint8)
    rgb["h stripes 6 dither"] = np.where(h == 0, h + dx, h - dx).astype(np.uint8)
    out = []
    for name in OPAQUE:
        t = np.empty((bh, bw, channels), np.uint8)
        t[..., :3] = rgb[name]
        if channels == 4:
            t[..., 3] = 255
        out.append((name, t))
    if channels == 3:
        return out
    one = (x == bw // 2) & (y == bh // 2)
    alpha = {
        "alpha 1..3": (noise(bw, bh, seed + 2), pick(bw, bh, seed + 3, (1, 2, 3))),
        "alpha extremes": (noise(bw, bh, seed + 4), pick(bw, bh, seed + 5, (0, 1, 2, 127, 128, 254, 255))),
        "alpha checker 0/255": (noise(bw, bh, seed + 6), np.where(((x + y) & 1) == 1, 255, 0)),
        "alpha checker 254/255": (noise(bw, bh, seed + 7), np.where(((x + y) & 1) == 1, 255, 254)),
        "alpha ramp across": (mono(vs6), (x * 255 + (bw - 1) // 2) // (bw - 1)),
        "alpha ramp down": (mono(hs6), 1 + (y * 254 + (bh - 1) // 2) // (bh - 1)),
        "opaque pixel": (noise(bw, bh, seed + 8), np.where(one, 255, 0)),
        "transparent pixel": (noise(bw, bh, seed + 9), np.where(one, 0, 255)),
        "stripes alpha 3/255": (mono(vs6), np.where(vs6, 3, 255)),
        "white alpha 1": (np.full((bh, bw, 3), 255, np.uint8), np.full((bh, bw), 1)),
    }
    for name in ALPHA:
        t = np.empty((bh, bw, 4), np.uint8)
        t[..., :3] = alpha[name][0]
        t[..., 3] = alpha[name][1].astype(np.uint8)
        out.append((name, t))
    return out


def layout(n):
    """(full columns, full rows) of a frame of n patterns: as square as it gets, every pattern in a full tile"""
    cols = int(np.ceil(np.sqrt(n)))
    return cols, -(-n // cols)


def frame(bw, bh, channels, names=None):
    """The patterns (all of them, or `names` in that order) as the tiles of one frame, row-major, over and over until the grid
    is full.  The last column is 7 px wide and the last row 5 px high, cut from the top left of the patterns that come next:
    the ragged tiles carry the same content.  Returns (image [H, W, channels], the pattern name of every tile)."""
    every = dict(patterns(bw, bh, channels))
    names = list(every) if names is None else list(names)
    cols, rows = layout(len(names))
    img = np.zeros((rows * bh + 5, cols * bw + 7, channels), np.uint8)
    tile_names = [None] * ((cols + 1) * (rows + 1))
    k = 0
    full = [(r, c) for r in range(rows) for c in range(cols)]
    ragged = [(r, c) for r in range(rows + 1) for c in range(cols + 1) if r == rows or c == cols]
    for r, c in full + ragged:
        name = names[k % len(names)]
        k += 1
        part = img[r * bh:(r + 1) * bh, c * bw:(c + 1) * bw]
        part[...] = every[name][: part.shape[0], : part.shape[1]]
        tile_names[r * (cols + 1) + c] = name
    return img, tile_names


def interleave(a, b):
    """a0, b0, a1, b1, ... (the shorter one starts over)"""
    n = max(len(a), len(b))
    return [(a, b)[k & 1][(k >> 1) % len((a, b)[k & 1])] for k in range(2 * n)]


WALK = tuple(2.0 ** (12 - k / 2) for k in range(56))


def factors(oracle, img, bw, bh, mode):
    """The factors of WALK (4096 down to 2^-15.5, half a level apart) at which the oracle stores img's tiles at a vector of
    sizes it has not stored them at before: one factor per distinct decision, in the order of the walk."""
    seen, out = set(), []
    for k in WALK:
        _, ow, oh, _ = oracle.shrink_image(img, bw, bh, mode, 4, k, want_pixels=False)
        key = ow.tobytes() + oh.tobytes()
        if key not in seen:
            seen.add(key)
            out.append(k)
    return out


def sides(n):
    """the stored sizes of a side of n pixels, level by level: n, ceil(n / 2), ceil(n / 4), ... 1"""
    out, level = [], 0
    while not out or out[-1] > 1:
        out.append(max(1, -(-n // (1 << level))))
        level += 1
    return out


def square_classes(bw, bh):
    """both sides at the same level, from the full tile down to 1x1"""
    ws, hs = sides(bw), sides(bh)
    n = max(len(ws), len(hs))
    return {(ws[min(l, len(ws) - 1)], hs[min(l, len(hs) - 1)]) for l in range(n)}


def required_classes(name, bw, bh, mode):
    """(the stored sizes a full bw x bh tile of pattern `name` must reach over WALK, whether it may reach no others).
    Mode 0 (Oklab detector, alpha included): one value for both sides.  Mode 1 (directional detector, alpha ignored): the
    width follows the variation down the tile and the height the variation across it."""
    if name in FLAT or (mode == 1 and name in PERIOD_2):
        return {(1, 1)}, True
    if mode == 0:
        return square_classes(bw, bh), True
    if name in VARIES_ACROSS:
        return {(1, s) for s in sides(bh)}, True
    if name in VARIES_DOWN:
        return {(s, 1) for s in sides(bw)}, True
    if name == "v stripes 6 dither":   # the stripes hold the height, the dither down the tile walks the width
        return {(1, s) for s in sides(bh)} | {(s, bh) for s in sides(bw)}, True
    if name == "h stripes 6 dither":
        return {(s, 1) for s in sides(bw)} | {(bw, s) for s in sides(bh)}, True
    if name in SQUARE_IN_MODE_1 and (bw == bh or name != "corner step"):
        return square_classes(bw, bh), False
    return {(bw, bh), (1, 1)}, False


def classes_by_pattern(tile_names, ow, oh, full):
    """{pattern: {(w, h)}} over the tiles flagged in `full` (the ragged ones have classes of their own)"""
    out = {}
    for name, w, h, f in zip(tile_names, ow.tolist(), oh.tolist(), full):
        if f:
            out.setdefault(name, set()).add((w, h))
    return out


def full_tiles(img, bw, bh):
    """bool per tile of img's grid: the tile is bw x bh"""
    H, W = img.shape[:2]
    cols, rows = -(-W // bw), -(-H // bh)
    return [(c + 1) * bw <= W and (r + 1) * bh <= H for r in range(rows) for c in range(cols)]
