"""Decode at reduced scale: the expected images, the stored sizes the tests deal and the classes they have to meet
(tests/test_scaled_host.py, tests/test_gpu_scaled_decode.py).

The model is the reference's own: Pixlzr::expand (pixlzr.rs:77-122) of a file whose public width, height and block sizes were
divided by s = 2^k resizes every block to ceil(fw/s) x ceil(fh/s) through PixlzrBlock::resize, and to_image places it at
(x0/s, y0/s).  oracle.resize is that per-tile resize for every size pair, so the expected image is built tile by tile from
oracle.decode_container and oracle.resize; nothing of the code under test is involved.

The classes of a resize are relative to the TARGET.  Not every class can occur at every (geometry, scale): at k = 0 the target is the
full place, so nothing shrinks, no edge tile is narrower than s = 1 and, with no 1x1 edge tile in these geometries, no target is
1x1; at the largest scale every target is 1x1 and nothing can grow.  What CAN occur is found by trying every stored size of every tile (feasible_classes); the dealer has to meet all
of it, at every (geometry, scale), and test_scaled_host.py asserts that it does and that every class occurs somewhere in each
geometry's scales."""
import numpy as np

# block_w, block_h, image width, image height, scales k: the geometries of tests/test_gpu_windows.py
GEOMS = [(32, 32, 100, 70, (0, 1, 2, 3, 4, 5)), (64, 64, 130, 65, (0, 1, 2, 3, 4, 5, 6)), (16, 16, 50, 33, (0, 1, 2, 3, 4)),
         (48, 20, 100, 37, (0, 1, 2))]
# a second geometry of each block for the batches: a block and a bit, so that its edge tiles are narrower than most scales
EXTRA = {(32, 32): (37, 63), (64, 64): (67, 33), (16, 16): (19, 5), (48, 20): (51, 23)}
CLASSES = ("clone", "one axis up", "one axis down", "both up", "both down", "mixed wider/lower", "mixed narrower/higher", "stored 1x1",
           "target 1x1", "ratio not a power of two", "edge narrower than s")
POISON = 0xA5


def ceil_div(a, b):
    return -(-a // b)


def tile_rects(w, h, bw, bh):
    cols, rows = ceil_div(w, bw), ceil_div(h, bh)
    return [(tx * bw, ty * bh, min(bw, w - tx * bw), min(bh, h - ty * bh)) for ty in range(rows) for tx in range(cols)]


def target_of(fw, fh, k):
    return ceil_div(fw, 1 << k), ceil_div(fh, 1 << k)


def pow2_ratio(a, b):
    hi, lo = max(a, b), min(a, b)
    return hi % lo == 0 and (hi // lo) & (hi // lo - 1) == 0


def classes_of(fw, fh, tw, th, k):
    """the classes of the resize of a tile of full place fw x fh, stored tw x th, decoded at 1/2^k"""
    nw, nh = target_of(fw, fh, k)
    out = set()
    dx, dy = (tw > nw) - (tw < nw), (th > nh) - (th < nh)  # +1: the axis shrinks, -1: it grows
    if dx == 0 and dy == 0:
        out.add("clone")
    elif dx == 0 or dy == 0:
        out.add("one axis up" if dx + dy < 0 else "one axis down")
    elif dx < 0 and dy < 0:
        out.add("both up")
    elif dx > 0 and dy > 0:
        out.add("both down")
    else:
        out.add("mixed wider/lower" if dx > 0 else "mixed narrower/higher")
    if (tw, th) == (1, 1):
        out.add("stored 1x1")
    if (nw, nh) == (1, 1):
        out.add("target 1x1")
    if not pow2_ratio(tw, nw) or not pow2_ratio(th, nh):
        out.add("ratio not a power of two")
    if fw < (1 << k) or fh < (1 << k):
        out.add("edge narrower than s")
    return out


def feasible_classes(w, h, bw, bh, k):
    """every class some stored size of some tile of the geometry has at scale k"""
    out = set()
    for (_, _, fw, fh) in set(tile_rects(w, h, bw, bh)):
        for tw in range(1, fw + 1):
            for th in range(1, fh + 1):
                out |= classes_of(fw, fh, tw, th, k)
    return out


def candidates(full, target):
    c = {1, max(target // 2, 1), max(target - 1, 1), target, min(full, target + 1), min(full, 3 * target // 2 + 1), min(full, 2 * target), full,
         max(3 * full // 4, 1), max(target // 3, 1)}
    return sorted(c)


def deal_sizes(w, h, bw, bh, k):
    """Stored sizes for the tiles of the files of one geometry that are decoded at scale k: tile by tile, largest first, the candidate
    pair (a handful of sizes around the target and the full place on each axis) that meets the most classes not met yet; ties go to
    the first.  A geometry of six tiles cannot meet seven directions in one file, so further files are dealt until everything that
    can occur is met.  Deterministic.  -> [(tile_w, tile_h)] per file"""
    rects = tile_rects(w, h, bw, bh)
    order = sorted(range(len(rects)), key=lambda t: (-rects[t][2] * rects[t][3], t))
    can, met, files = feasible_classes(w, h, bw, bh, k), set(), []
    while not files or (met != can and len(files) < 4):
        tw, th = np.zeros(len(rects), np.uint32), np.zeros(len(rects), np.uint32)
        for t in order:
            _, _, fw, fh = rects[t]
            nw, nh = target_of(fw, fh, k)
            best, gain = None, -1
            for a in candidates(fw, nw):
                for b in candidates(fh, nh):
                    g = len(classes_of(fw, fh, a, b, k) - met)
                    if g > gain:
                        best, gain = (a, b), g
            tw[t], th[t] = best
            met |= classes_of(fw, fh, best[0], best[1], k)
        files.append((tw, th))
    return files


def met_classes(w, h, bw, bh, k, tw, th):
    out = set()
    for (_, _, fw, fh), a, b in zip(tile_rects(w, h, bw, bh), tw, th):
        out |= classes_of(fw, fh, int(a), int(b), k)
    return out


def random_slots(rng, tw, th, slot_px, c):
    """random stored bytes (RGBA: any alpha), the rest of each slot a pattern"""
    slots = np.full((tw.size, slot_px * c), POISON, np.uint8)
    for t in range(tw.size):
        n = int(tw[t]) * int(th[t]) * c
        slots[t, :n] = rng.integers(0, 256, n, dtype=np.uint8)
    return slots


def scaled_tiles_image(oracle, w, h, bw, bh, c, filt, k, tw, th, slots, base=None):
    """the image of the tiles at 1/2^k: (ceil(h/s), ceil(w/s), c).  A tile whose stored size is zero or exceeds its FULL place is
    skipped: its pixels keep what `base` (a scalar, default 0) says."""
    s = 1 << k
    assert bw % s == 0 and bh % s == 0
    out = np.full((ceil_div(h, s), ceil_div(w, s), c), 0 if base is None else base, np.uint8)
    for t, (x0, y0, fw, fh) in enumerate(tile_rects(w, h, bw, bh)):
        a, b = int(tw[t]), int(th[t])
        if a == 0 or b == 0 or a > fw or b > fh:
            continue
        nw, nh = target_of(fw, fh, k)
        tile = np.ascontiguousarray(slots[t, :a * b * c]).reshape(b, a, c)
        out[y0 // s:y0 // s + nh, x0 // s:x0 // s + nw] = oracle.resize(tile, nw, nh, filt)
    return out


def scaled_image(oracle, raw, c, filt, k):
    """the image a .pixlzr file (bytes) decodes to at 1/2^k"""
    d = oracle.decode_container(raw)
    return scaled_tiles_image(oracle, d["width"], d["height"], d["bw"], d["bh"], c, filt, k, d["tw"], d["th"], d["slots"])


def scaled_rect(rect, k):
    """(x, y, w, h) in full-resolution pixels -> (x0, y0, x1, y1) of the scaled image"""
    x, y, w, h = rect
    s = 1 << k
    return x // s, y // s, ceil_div(x + w, s), ceil_div(y + h, s)


class File:
    """one .pixlzr file whose stored sizes (tile_w, tile_h) are dealt for scale k, with random stored bytes, written by the oracle's writer; what it
    decodes to per (filter, scale), computed once"""

    def __init__(self, oracle, bw, bh, w, h, c, k, sizes, seed=0):
        self.bw, self.bh, self.w, self.h, self.c, self.k = bw, bh, w, h, c, k
        rng = np.random.default_rng(4000 * seed + 131 * k + bw * 7 + bh * 3 + w + h + c)
        self.tw, self.th = sizes
        self.slots = random_slots(rng, self.tw, self.th, bw * bh, c)
        values = rng.integers(0, 1 << 32, self.tw.size, dtype=np.uint64).astype(np.uint32).view(np.float32)
        self.raw = oracle.encode_container(w, h, bw, bh, c, 0, values, None, self.tw, self.th, self.slots)
        self.oracle, self._image = oracle, {}

    def image(self, filt, k=None):
        k = self.k if k is None else k
        if (filt, k) not in self._image:
            img = scaled_image(self.oracle, self.raw, self.c, filt, k)
            img.setflags(write=False)
            self._image[(filt, k)] = img
        return self._image[(filt, k)]


_files = {}


def files_of(oracle, bw, bh, w, h, c, k):
    """the files of one geometry dealt for scale k (deal_sizes: one, or as many as meet every class)"""
    key = (bw, bh, w, h, c, k)
    if key not in _files:
        _files[key] = [File(oracle, bw, bh, w, h, c, k, sizes, seed=r) for r, sizes in enumerate(deal_sizes(w, h, bw, bh, k))]
    return _files[key]
