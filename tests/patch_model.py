"""What a patch of pixel windows must give, from the oracle binding alone, and the fixtures the patch tests share.

The reference operation (decode_block gives every stored block a value, src/encoding/mod.rs:236-241; Pixlzr::shrink_by shrinks
only blocks without one, src/data_types/pixlzr.rs:166-170): open a file, replace the blocks a window covers by fresh full-size
blocks -- the stored block resized to its place with the new pixels written over it --, shrink, save.  Here:
  1. oracle.decode_container of the file;
  2. oracle.expand_image with the expand filter;
  3. the windows' new pixels written over the image;
  4. oracle.shrink_image of each window's hull (the covered tiles' rectangle, clipped to the image) on its own;
  5. oracle.encode_container of the mixed tile set: old values, sizes and bytes for the tiles no window covers, new ones for the
     covered tiles.
No new oracle function is needed: a tile's shrink result depends only on its own pixels, and the oracle's writer is canonical
over what its reader reads (tests/test_patch_host.py holds both on the fixtures).  The covering and disjointness logic of
pxz_patch_check stands here in Python too."""
import numpy as np

NEAREST, LANCZOS3 = 0, 4
SHRINK_BY, DIRECTIONAL = 0, 1


# ---- geometry -------------------------------------------------------------------------------------------------------------

def covered(rect, bw, bh):
    """(first column, first row, columns, rows) of the tile grid a pixel rectangle (x, y, w, h) covers"""
    x, y, w, h = rect
    c0, r0 = x // bw, y // bh
    return c0, r0, (x + w - 1) // bw - c0 + 1, (y + h - 1) // bh - r0 + 1


def hull(rect, size, bw, bh):
    """the tile-aligned rectangle of the covered tiles, clipped to the image: (x, y, w, h)"""
    c0, r0, cc, cr = covered(rect, bw, bh)
    x1, y1 = min((c0 + cc) * bw, size[0]), min((r0 + cr) * bh, size[1])
    return c0 * bw, r0 * bh, x1 - c0 * bw, y1 - r0 * bh


def covered_tiles(rect, size, bw, bh):
    """the image's tile numbers a rectangle covers, in the window layout's order"""
    cols = -(-size[0] // bw)
    c0, r0, cc, cr = covered(rect, bw, bh)
    return [(r0 + j) * cols + c0 + i for j in range(cr) for i in range(cc)]


def layout(windows, bw, bh):
    """pxz_window_layout's offsets for windows = [(image, x, y, w, h, ...), ...]"""
    offs = [0]
    for w in windows:
        _, _, cc, cr = covered(w[1:5], bw, bh)
        offs.append(offs[-1] + cc * cr)
    return offs


def first_overlap(windows, bw, bh):
    """the first window that covers a tile an earlier window of its image covers, or None: pxz_patch_check's rule"""
    seen = {}
    for k, w in enumerate(windows):
        c0, r0, cc, cr = covered(w[1:5], bw, bh)
        mine = {(w[0], c0 + i, r0 + j) for j in range(cr) for i in range(cc)}
        if any(t in seen for t in mine):
            return k
        for t in mine:
            seen[t] = k
    return None


# ---- the expected tiles and files -----------------------------------------------------------------------------------------

class Params:
    def __init__(self, mode, filt, factor, expand_filter):
        self.mode, self.filt, self.factor, self.expand_filter = mode, filt, factor, expand_filter


def decoded(oracle, raw, c):
    """decode_container with the slots cut to bw * bh * c bytes (the product's slot size)"""
    d = oracle.decode_container(raw)
    d["slots"] = np.ascontiguousarray(d["slots"][:, :d["bw"] * d["bh"] * c])
    return d


def patched_image(oracle, d, c, expand_filter, patches):
    """steps 2 and 3: the file's image with the new pixels over it; patches = [((x, y, w, h), pixels[h, w, c]), ...]"""
    img = oracle.expand_image(d["width"], d["height"], d["bw"], d["bh"], c, expand_filter, d["tw"], d["th"], d["slots"])
    for (x, y, w, h), px in patches:
        img[y:y + h, x:x + w] = px
    return img


def hull_tiles(oracle, img, rect, bw, bh, p):
    """step 4 for one window: (values, w, h, slots) of the covered tiles in the window layout's order"""
    hx, hy, hw, hh = hull(rect, (img.shape[1], img.shape[0]), bw, bh)
    return oracle.shrink_image(np.ascontiguousarray(img[hy:hy + hh, hx:hx + hw]), bw, bh, p.mode, p.filt, p.factor)


def patched_file(oracle, raw, c, p, patches):
    """all five steps for one file: -> (the new file, [(values, w, h, slots) per window])"""
    d = decoded(oracle, raw, c)
    bw, bh, size = d["bw"], d["bh"], (d["width"], d["height"])
    img = patched_image(oracle, d, c, p.expand_filter, patches)
    vals, tw, th, slots = d["values"].copy(), d["tw"].copy(), d["th"].copy(), d["slots"].copy()
    per_window = []
    for rect, _ in patches:
        nv, nw, nh, ns = hull_tiles(oracle, img, rect, bw, bh, p)
        per_window.append((nv, nw, nh, ns))
        for q, t in enumerate(covered_tiles(rect, size, bw, bh)):
            vals[t], tw[t], th[t], slots[t] = nv[q], nw[q], nh[q], ns[q]
    new = oracle.encode_container(size[0], size[1], bw, bh, c, d["filter"], vals, None, tw, th, slots)
    return new, per_window


# ---- fixtures -------------------------------------------------------------------------------------------------------------

def picture(width, height, c, bw, bh, seed):
    """a picture whose tiles alternate between smooth ramps (which the shrink stores small) and strong noise (which it keeps at full
    size); RGBA with an alpha that goes down to 0 in one corner"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:height, 0:width]
    img = np.zeros((height, width, c), np.float64)
    img[..., 0] = xx * 255.0 / max(width - 1, 1)
    img[..., 1] = yy * 255.0 / max(height - 1, 1)
    img[..., 2] = (xx + yy) * 255.0 / max(width + height - 2, 1)
    if c == 4:
        img[..., 3] = np.clip(40.0 + 3.0 * np.hypot(xx, yy), 0, 255)
        img[:6, :6, 3] = 0
    noisy = ((xx // bw + yy // bh) % 2 == 1)[..., None]
    noise = rng.integers(0, 256, (height, width, c)).astype(np.float64)
    return np.where(noisy, noise, img).round().clip(0, 255).astype(np.uint8)


def new_pixels(rect, c, seed):
    """a window's new pixels: noise in the upper left, a ramp elsewhere, RGBA with low alpha in one column"""
    x, y, w, h = rect
    rng = np.random.default_rng(seed * 7919 + x * 31 + y * 17 + w * 3 + h)
    yy, xx = np.mgrid[0:h, 0:w]
    px = np.zeros((h, w, c), np.float64)
    px[..., 0] = 255 - xx * 200.0 / max(w - 1, 1)
    px[..., 1] = 30 + yy * 200.0 / max(h - 1, 1)
    px[..., 2] = 128
    if c == 4:
        px[..., 3] = 255
        px[:, w // 2, 3] = 3
    noisy = ((xx < (w + 1) // 2) & (yy < (h + 1) // 2))[..., None]
    return np.where(noisy, rng.integers(0, 256, (h, w, c)), px).round().clip(0, 255).astype(np.uint8)


# name: (width, height, block_w, block_h, channels, mode, filter, factor, expand filter).  The factors were picked, per mode, so that
# the ramps come out small and the noise stays whole (test_patch_host.py asserts it and says what it saw)
FIXTURES = {
    "rgba-32-directional": (200, 136, 32, 32, 4, DIRECTIONAL, LANCZOS3, 10.0, LANCZOS3),
    "rgb-32-by": (200, 136, 32, 32, 3, SHRINK_BY, LANCZOS3, 0.3, LANCZOS3),
    "rgba-64-by": (130, 130, 64, 64, 4, SHRINK_BY, LANCZOS3, 0.3, LANCZOS3),
    "rgb-64-directional": (130, 130, 64, 64, 3, DIRECTIONAL, LANCZOS3, 10.0, LANCZOS3),
    "rgba-48x20-directional-nearest": (150, 70, 48, 20, 4, DIRECTIONAL, NEAREST, 10.0, NEAREST),
    "rgb-48x20-by": (150, 70, 48, 20, 3, SHRINK_BY, LANCZOS3, 0.3, LANCZOS3),
}


class Fixture:
    def __init__(self, oracle, name):
        self.name = name
        self.w, self.h, self.bw, self.bh, self.c, mode, filt, factor, xf = FIXTURES[name]
        self.p = Params(mode, filt, factor, xf)
        self.size = (self.w, self.h)
        self.cols, self.rows = -(-self.w // self.bw), -(-self.h // self.bh)
        self.image = picture(self.w, self.h, self.c, self.bw, self.bh, sum(map(ord, name)))
        v, tw, th, slots = oracle.shrink_image(self.image, self.bw, self.bh, mode, filt, factor)
        self.raw = oracle.encode_container(self.w, self.h, self.bw, self.bh, self.c, 0, v, None, tw, th, slots)
        self.tw, self.th = tw, th

    def windows(self):
        """name -> the rectangles of one call over this file (one, or two in one tile row)"""
        w, h, bw, bh = self.w, self.h, self.bw, self.bh
        return {
            "pixel": [(bw + 3, bh + 2, 1, 1)],
            "inside": [(bw + 1, bh + 2, bw - 3, bh - 5)],        # a tile of ramps, stored small
            "inside a whole tile": [(bw + 1, 2, bw - 3, bh - 5)],  # a tile of noise, stored at full size
            "tile": [(bw, bh, bw, bh)],
            "corner": [(bw - 3, bh - 5, 9, 11)],  # a 2x2 tile corner at odd offsets, odd width
            "edge": [(w - 37, h - 9, 37, 9)],     # the ragged right and bottom edges
            "whole": [(0, 0, w, h)],
            "two": [(1, bh + 1, bw - 2, bh - 2), ((self.cols - 1) * bw - 5, bh + 3, 7, 5)],
        }

    def stored_full(self, t):
        tx, ty = t % self.cols, t // self.cols
        fw = self.w - tx * self.bw if tx == self.cols - 1 else self.bw
        fh = self.h - ty * self.bh if ty == self.rows - 1 else self.bh
        return int(self.tw[t]) == fw and int(self.th[t]) == fh


_fixtures = {}


def fixture(oracle, name):
    if name not in _fixtures:
        _fixtures[name] = Fixture(oracle, name)
    return _fixtures[name]
