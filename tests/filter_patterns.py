"""Frames and a model for the two image-to-image filters, process() and tree::process (tests/test_filter_domain_host.py,
tests/test_gpu_filter_domain.py).

Under the identity closure a tile's level is round(log2(mean absolute deviation)), and the 0/255 tiles of tests/value_patterns.py
all have a deviation near 0.5: every opaque one is pixelised at exactly half size.  The SPARSE tiles below walk the levels
instead: a foreground pixel wherever hash32(i, seed) % per == 0 over a background, so that the deviation is about 2 / per of
the step between the two -- per = 4 .. 64 gives half size down to 1 / 32.  Five kinds of step: white on black, black on white,
alpha 1 on opaque white, opaque on alpha-2 white, and opaque white on clear black (whose reduced tiles hold alpha of a few
units under colours up to 255: where the reciprocal of un-premultiply is large).  In all five a premultiplied colour equals its
alpha or is 0 where the alpha is, so colour and alpha resample alike and un-premultiply is never handed a colour above its
alpha; a sixth kind, opaque pixels of 0 / 255 drawn per channel on clear black, is there for that: a pixel whose channel is 0
under alpha 255, met by a negative weight, leaves the colour above the alpha.

frame() lays the sparse tiles and the value_patterns tiles out as one image; process() and tree_process() restate the two
filters from the oracle's primitives (tile_rect, lod_oklab_identity, reduce_dims, resize) and return, beside the image, what
became of every rectangle -- the census the host module asserts coverage from.

Pure numpy and deterministic: no generator state, the same frames on every machine."""
import functools

import numpy as np

import value_patterns as vp

PERS = (4, 8, 16, 32, 64)
# kind: (foreground RGBA, background RGBA)
KINDS = {
    "white on black": ((255, 255, 255, 255), (0, 0, 0, 255)),
    "black on white": ((0, 0, 0, 255), (255, 255, 255, 255)),
    "alpha 1 on white": ((255, 255, 255, 1), (255, 255, 255, 255)),
    "opaque on alpha 2": ((255, 255, 255, 255), (255, 255, 255, 2)),
    "white on clear": ((255, 255, 255, 255), (0, 0, 0, 0)),
    "colours on clear": (None, (0, 0, 0, 0)),   # (foreground: value_patterns.noise, opaque)
}
OPAQUE_KINDS = ("white on black", "black on white")
ALPHA_KINDS = ("alpha 1 on white", "opaque on alpha 2", "white on clear", "colours on clear")
EDGES = ((7, 5), (1, 1))

# (filter down, filter up): every filter runs on each side (0 Nearest, 1 Triangle, 2 CatmullRom, 3 Gaussian, 4 Lanczos3)
FILTER_PAIRS = ((4, 0), (2, 4), (3, 1), (1, 2), (0, 3))
# tree::process thresholds, between the clusters the tiles' values form (about 0.5, 0.37, 0.21, 0.11, 0.05, 0.02 and 0): 0.0
# splits everything (the source comes back), 50.0 pixelises everything (process() comes back), the negative one inverts level 0
THRESHOLDS = (0.0, 0.03, 0.08, 0.16, 0.3, 0.45, 50.0, -0.16)
# the cases both modules run: (bw, bh, ragged edge, all tiles or the subset)
PROCESS_CASES = (
    (16, 16, (7, 5), False), (32, 32, (7, 5), False), (32, 32, (1, 1), False), (64, 64, (7, 5), False),
    (20, 12, (7, 5), False), (20, 12, (1, 1), False), (128, 128, (7, 5), True),
)
# (bw, bh, minimum bw, minimum bh, ragged edge, subset).  GRIDS: every block is exactly two of the next, up to 64 px: the
# per-level grids.  RECTS: halvings that go odd, or blocks above 64 px: the rectangle lists.
TREE_GRID_CASES = (
    (64, 64, 4, 4, (7, 5), False), (32, 32, 4, 4, (1, 1), False), (64, 32, 4, 4, (7, 5), False), (16, 16, 4, 4, (7, 5), False),
    (64, 64, 20, 9, (1, 1), False),
)
TREE_RECT_CASES = (
    (50, 50, 4, 4, (7, 5), False), (37, 61, 4, 4, (1, 1), False), (100, 36, 4, 4, (7, 5), False), (128, 128, 4, 4, (7, 5), True),
    (50, 50, 20, 9, (1, 1), False),
)


def sparse_name(per, kind):
    return f"sparse {per} {kind}"


def sparse_mask(bw, bh, per, kind):
    """bool [bh, bw]: the foreground pixels"""
    i = np.arange(bh * bw, dtype=np.uint64).reshape(bh, bw)
    seed = 0x5A17 + bw * 4099 + bh * 17 + per * 257 + list(KINDS).index(kind) * 65537
    return (vp.hash32(i, seed) % np.uint32(per)) == 0


def sparse(bw, bh, per, kind, channels):
    """[bh, bw, channels] uint8: the kind's foreground on its background (RGB: the colours alone, opaque kinds only)"""
    assert channels == 4 or kind in OPAQUE_KINDS
    fg, bg = KINDS[kind]
    if fg is None:
        fg = np.concatenate([vp.noise(bw, bh, 0xC0 + per + bw * 4099 + bh * 17), np.full((bh, bw, 1), 255, np.uint8)], axis=2)
    else:
        fg = np.array(fg[:channels], np.uint8)
    return np.where(sparse_mask(bw, bh, per, kind)[:, :, None], fg, np.array(bg[:channels], np.uint8)).astype(np.uint8)


def sparse_names(channels):
    kinds = OPAQUE_KINDS + (ALPHA_KINDS if channels == 4 else ())
    return [sparse_name(per, kind) for kind in kinds for per in PERS]


def tiles(bw, bh, channels):
    """{name: tile}: the sparse family, then the value_patterns tiles"""
    kinds = OPAQUE_KINDS + (ALPHA_KINDS if channels == 4 else ())
    out = {sparse_name(per, kind): sparse(bw, bh, per, kind, channels) for kind in kinds for per in PERS}
    out.update(vp.patterns(bw, bh, channels))
    return out


def frame(bw, bh, channels, edge=(7, 5), names=None, rotate=0):
    """value_patterns.frame with the sparse tiles in front and the ragged edge as a parameter: the last column is edge[0] px
    wide and the last row edge[1] px high.  rotate: the list of names starts that many places later (the second frame of a
    batch: the same tiles, every one a place further on).  -> (image [H, W, channels], the pattern name of every tile)"""
    every = tiles(bw, bh, channels)
    names = list(every) if names is None else list(names)
    names = names[rotate % len(names):] + names[: rotate % len(names)]
    cols, rows = vp.layout(len(names))
    img = np.zeros((rows * bh + edge[1], cols * bw + edge[0], channels), np.uint8)
    tile_names = [None] * ((cols + 1) * (rows + 1))
    full = [(r, c) for r in range(rows) for c in range(cols)]
    ragged = [(r, c) for r in range(rows + 1) for c in range(cols + 1) if r == rows or c == cols]
    for k, (r, c) in enumerate(full + ragged):
        name = names[k % len(names)]
        part = img[r * bh:(r + 1) * bh, c * bw:(c + 1) * bw]
        part[...] = every[name][: part.shape[0], : part.shape[1]]
        tile_names[r * (cols + 1) + c] = name
    return img, tile_names


def batch(bw, bh, channels, edge=(7, 5), names=None):
    """two frames [2, H, W, channels]: the second holds the same tiles rotated by one place; and their tile names"""
    a, na = frame(bw, bh, channels, edge, names, 0)
    b, nb = frame(bw, bh, channels, edge, names, 1)
    return np.stack([a, b]), (na, nb)


@functools.lru_cache(maxsize=None)
def case_batch(bw, bh, channels, edge=(7, 5), sub=False):
    """batch() of a case, made once and read-only: (frames [2, H, W, channels], (tile names of frame 0, of frame 1))"""
    frames, names = batch(bw, bh, channels, edge, subset(channels) if sub else None)
    frames.setflags(write=False)
    return frames, names


def subset(channels):
    """about a dozen tiles for the largest blocks: every `per` of one opaque kind, some of the low-alpha kinds, and the
    value_patterns tiles that overshoot most"""
    names = [sparse_name(per, "white on black") for per in PERS]
    names += ["checker 2", "corner step", "white pixel", "noise"]
    if channels == 4:
        names += [sparse_name(8, "colours on clear"), sparse_name(32, "colours on clear"), sparse_name(64, "white on clear"),
                  sparse_name(16, "alpha 1 on white"), "alpha extremes"]
    else:
        names += [sparse_name(8, "black on white"), "black pixel", "blocks 3"]
    return names


# ---- the model: process() and tree::process from the oracle's primitives -------------------------------------------------------

def rgba(tile):
    if tile.shape[2] == 4:
        return tile
    return np.concatenate([tile, np.full(tile.shape[:2] + (1,), 255, np.uint8)], axis=2)


def pixelise(oracle, img, x, y, w, h, down, up, memo=None):
    """process/mod.rs:84-95 on the tile (x, y, w, h) of img -> (the tile back at its size, its reduced size, its value).
    memo: a dict of the caller's, one per image: a tile's value and result are computed once, whatever asks for them again"""
    memo = {} if memo is None else memo
    tile = img[y:y + h, x:x + w]
    if ("v", x, y, w, h) not in memo:
        memo["v", x, y, w, h] = oracle.lod_oklab_identity(tile)
    v = memo["v", x, y, w, h]
    if down is None:
        return None, None, v
    if ("p", x, y, w, h, down, up) not in memo:
        nw, nh, _ = oracle.reduce_dims(v, v, w, h)
        small = oracle.resize(tile, nw, nh, down)
        memo["p", x, y, w, h, down, up] = (oracle.resize(small, w, h, up), (nw, nh))
    return memo["p", x, y, w, h, down, up] + (v,)


def process(oracle, img, bw, bh, down=4, up=0, memo=None):
    """-> (RGBA image, census): census is a list of (level 0, "pixelised", x, y, w, h, nw, nh), one per tile"""
    H, W, _ = img.shape
    out = np.zeros((H, W, 4), np.uint8)
    census = []
    cols, rows = oracle.grid(W, H, bw, bh)
    for t in range(cols * rows):
        x0, y0, w, h = oracle.tile_rect(W, H, bw, bh, t)
        full, (nw, nh), _ = pixelise(oracle, img, x0, y0, w, h, down, up, memo)
        out[y0:y0 + h, x0:x0 + w] = rgba(full)
        census.append((0, "pixelised", x0, y0, w, h, nw, nh))
    return out, census


def tree_process(oracle, img, bw, bh, threshold, min_bw=4, min_bh=4, down=4, up=0, memo=None):
    """tree::process_custom (process/tree.rs:23-83) -> (RGBA image, census).  census: (level, what, x, y, w, h, nw, nh) per
    rectangle, `what` one of "pixelised" (nw x nh its reduced size), "split" and "kept" (at or below the minimum block: the
    pixels as they are); nw = nh = 0 for the latter two.  Level l has blocks of (bw >> l, bh >> l)."""
    H, W, _ = img.shape
    out = np.zeros((H, W, 4), np.uint8)
    census = []
    mbw, mbh = max(min_bw, 4), max(min_bh, 4)
    memo = {} if memo is None else memo

    def rec(x, y, w, h, bw, bh, level, thr, positive):
        if bw <= mbw or bh <= mbh:
            out[y:y + h, x:x + w] = rgba(img[y:y + h, x:x + w])
            census.append((level, "kept", x, y, w, h, 0, 0))
            return
        if ("g", w, h, bw, bh) not in memo:
            cols, rows = oracle.grid(w, h, bw, bh)
            memo["g", w, h, bw, bh] = [oracle.tile_rect(w, h, bw, bh, t) for t in range(cols * rows)]
        for tx, ty, tw, th in memo["g", w, h, bw, bh]:
            v = pixelise(oracle, img, x + tx, y + ty, tw, th, None, None, memo)[2]
            if bool(v >= thr) != positive:
                full, (nw, nh), _ = pixelise(oracle, img, x + tx, y + ty, tw, th, down, up, memo)
                out[y + ty:y + ty + th, x + tx:x + tx + tw] = rgba(full)
                census.append((level, "pixelised", x + tx, y + ty, tw, th, nw, nh))
            else:
                census.append((level, "split", x + tx, y + ty, tw, th, 0, 0))
                rec(x + tx, y + ty, tw, th, bw >> 1, bh >> 1, level + 1, thr, True)

    rec(0, 0, W, H, bw, bh, 0, np.float32(abs(threshold)), threshold >= 0.0)
    return out, census


def tree_references(oracle, frames, bw, bh, min_bw, min_bh, down, up, thresholds=THRESHOLDS):
    """{(frame, threshold): oracle.tree_process_image}.  The oracle's calls are independent C calls (ctypes lets go of the
    interpreter lock for them): a few at a time."""
    from concurrent.futures import ThreadPoolExecutor
    keys = [(n, thr) for n in range(len(frames)) for thr in thresholds]
    with ThreadPoolExecutor(max_workers=8) as pool:
        images = pool.map(lambda k: oracle.tree_process_image(frames[k[0]], bw, bh, k[1], min_bw, min_bh, down, up), keys)
        return dict(zip(keys, images))


def rects_of(census, bad):
    """the census entries (but the split ones) that hold a pixel flagged in bad [H, W]"""
    return [e for e in census if e[1] != "split" and bad[e[3]:e[3] + e[5], e[2]:e[2] + e[4]].any()]


def describe(entries, tile_names, W, bw, bh, limit=10):
    """the rectangles by the pattern of the frame tile they lie in"""
    cols = -(-W // bw)
    out = []
    for level, what, x, y, w, h, nw, nh in entries[:limit]:
        name = tile_names[(y // bh) * cols + x // bw]
        out.append(f"{name}: level {level} {what} {w}x{h} at ({x}, {y})" + (f" via {nw}x{nh}" if what == "pixelised" else ""))
    more = len(entries) - limit
    return "; ".join(out) + (f"; and {more} more" if more > 0 else "")
