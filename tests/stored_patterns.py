"""Stored-tile patterns for the expand kernels (tests/test_expand_domain_host.py, tests/test_gpu_expand_domain.py).

The expand entry points take (tile_w, tile_h, slots) directly, so a pattern here is drawn AT THE STORED SIZE (tw, th) and put into
a slot: no shrink is involved, and stored sizes that no shrink produces (a side of 1 beside a side of 16, 3x8, ...) are reachable.
The tiles sit at the ends of the value domain, as those of value_patterns.py do on the encode side: 0/255 edges whose way up
overshoots in both passes, alpha in 0..3 and around 127/128 and 254/255, and tiles whose ONLY pixel that is not opaque (or not
transparent) sits at a chosen stored index -- the wave-wide "identity at alpha 255" gates of the decode side have otherwise only
seen "every lane" or "no lane".  What the patterns make the oracle do is asserted in test_expand_domain_host.py, without the
code under test.

Everything is pure numpy and deterministic (value_patterns.hash32: no generator state).  A side of 1 is allowed: the patterns
degenerate (a step of one column is white, a checker of one pixel is black) and the host module asserts what is left of them."""
import numpy as np

import value_patterns as vp

OPAQUE = ("checker", "v stripes", "h stripes", "v step", "h step", "corner step", "white pixel", "black pixel", "noise",
          "flat 0", "flat 255")
ALPHA = ("alpha 1..3", "alpha extremes", "alpha checker 0/255", "alpha checker 254/255", "alpha v stripes 3/255",
         "alpha h stripes 3/255", "white alpha 1", "white alpha 0")
# "<kind> @<stored index>": opaque but for one pixel of alpha 254 / of alpha 0; transparent but for one opaque pixel
ONE_PIXEL_KINDS = ("one 254", "one 0", "lone opaque")
# the four opaque patterns whose way up overshoots on both sides in both passes (test_expand_domain_host.py)
OVERSHOOT = ("checker", "corner step", "white pixel", "black pixel")
# the widths of the one-row tiles of a 32x32 tile: the matrix-core form's shortcut up to 16, the general form's beyond and between
ONE_ROW_WIDTHS = (1, 2, 4, 8, 16, 32, 31, 12, 3)
# what the 192x192 tiles (image in HBM) carry: a few of each kind
BIG_PATTERNS = OVERSHOOT + ("alpha 1..3", "alpha extremes", "alpha checker 254/255", "alpha v stripes 3/255", "one 254 @0", "one 0 @63",
                            "one 254 @64", "lone opaque @0", "flat 255", "noise")


def gate_indices(n):
    """The stored indices a one-pixel tile of n pixels is drawn at: 0 (served by the kernels' first-pixel prefetch, not by the slot
    read), 63 and 64 (either side of a 64-lane staging round), one in the middle of a later round, the last."""
    mid = 64 * max(2, (n // 64) // 2) + 29
    return sorted({i for i in (0, 63, 64, mid, n - 1) if 0 <= i < n})


def one_pixel_names(tw, th):
    return tuple(f"{kind} @{i}" for kind in ONE_PIXEL_KINDS for i in gate_indices(tw * th))


def names(tw, th, channels):
    """every pattern name of a tw x th stored tile"""
    return OPAQUE if channels == 3 else OPAQUE + ALPHA + one_pixel_names(tw, th)


def colours(tw, th, seed):
    """0/255 colours of the alpha tiles: a checker in red, its inverse in green, noise in blue"""
    y, x = np.mgrid[0:th, 0:tw]
    c = np.empty((th, tw, 3), np.uint8)
    c[..., 0] = (((x + y) & 1) == 1) * 255
    c[..., 1] = 255 - c[..., 0]
    c[..., 2] = vp.noise(tw, th, seed, 1)[..., 0]
    return c


def stored(name, tw, th, channels):
    """the pattern `name` drawn at tw x th: [th, tw, channels] uint8 (alpha 255 under the opaque patterns when channels == 4)"""
    assert channels in (3, 4) and tw >= 1 and th >= 1
    y, x = np.mgrid[0:th, 0:tw]
    seed = tw * 4099 + th * 17 + 0xE0
    centre = (x == tw // 2) & (y == th // 2)
    if name in OPAQUE:
        rgb = {
            "checker": lambda: vp.mono(((x + y) & 1) == 1),
            "v stripes": lambda: vp.mono((x & 1) == 1),
            "h stripes": lambda: vp.mono((y & 1) == 1),
            "v step": lambda: vp.mono(x >= tw // 2),
            "h step": lambda: vp.mono(y >= th // 2),
            "corner step": lambda: vp.mono((x >= tw // 2) & (y >= th // 2)),
            "white pixel": lambda: vp.mono(centre),
            "black pixel": lambda: vp.mono(~centre),
            "noise": lambda: vp.noise(tw, th, seed + 1),
            "flat 0": lambda: np.zeros((th, tw, 3), np.uint8),
            "flat 255": lambda: np.full((th, tw, 3), 255, np.uint8),
        }[name]()
        alpha = np.full((th, tw), 255)
    else:
        assert channels == 4, name
        white = np.full((th, tw, 3), 255, np.uint8)
        if name in ALPHA:
            rgb, alpha = {
                "alpha 1..3": lambda: (colours(tw, th, seed + 2), vp.pick(tw, th, seed + 3, (1, 2, 3))),
                "alpha extremes": lambda: (colours(tw, th, seed + 4), vp.pick(tw, th, seed + 5, (0, 1, 2, 127, 128, 254, 255))),
                "alpha checker 0/255": lambda: (colours(tw, th, seed + 6), np.where(((x + y) & 1) == 1, 255, 0)),
                "alpha checker 254/255": lambda: (colours(tw, th, seed + 7), np.where(((x + y) & 1) == 1, 255, 254)),
                "alpha v stripes 3/255": lambda: (colours(tw, th, seed + 8), np.where((x & 1) == 1, 3, 255)),
                "alpha h stripes 3/255": lambda: (colours(tw, th, seed + 9), np.where((y & 1) == 1, 3, 255)),
                "white alpha 1": lambda: (white, np.full((th, tw), 1)),
                "white alpha 0": lambda: (white, np.full((th, tw), 0)),
            }[name]()
        else:
            kind, at = name.split(" @")
            one = (y * tw + x) == int(at)
            assert kind in ONE_PIXEL_KINDS and one.sum() == 1, name
            rgb = colours(tw, th, seed + 10)
            alpha = {"one 254": np.where(one, 254, 255), "one 0": np.where(one, 0, 255), "lone opaque": np.where(one, 255, 0)}[kind]
    t = np.empty((th, tw, channels), np.uint8)
    t[..., :3] = rgb
    if channels == 4:
        t[..., 3] = alpha.astype(np.uint8)
    return t


def opaque_twin(tile):
    """the same colours at alpha 255"""
    t = tile.copy()
    t[..., 3] = 255
    return t


def pow2_below(n):
    return [1 << k for k in range(n.bit_length()) if (1 << k) < n]


def pairs(bw, bh):
    """The stored sizes the GPU module drives a full bw x bh tile at -> {class: [(tw, th)]}.
    square 16 / 32 / 64 (the matrix-core kernels): "pow2" every pair of powers of two below the side, "one pass" the side itself
    beside a power of two, "odd" sizes that take the general form, "clone".  Other tiles (the general form alone): the level
    pairs, sides of 1 and 2 beside larger ones, the one-pass pairs, odd sizes, the clone."""
    if bw == bh and bw in (16, 32, 64):
        p = pow2_below(bw)
        return {"pow2": [(a, b) for a in p for b in p],
                "one pass": [(bw, b) for b in p] + [(a, bh) for a in p],
                "odd": [(3, 8), (8, 5), (bw - 1, bh // 2), (12, 12)],
                "clone": [(bw, bh)]}
    if (bw, bh) == (192, 192):
        return {"pow2": [(1, 1), (2, 1), (1, 2), (2, 2), (1, 96), (96, 1)], "one pass": [(192, 24), (24, 192), (192, 1), (1, 192)],
                "odd": [(96, 96), (48, 48), (3, 5)], "clone": [(192, 192)]}
    ws, hs = vp.sides(bw), vp.sides(bh)
    n = max(len(ws), len(hs))
    level = [(ws[min(l, len(ws) - 1)], hs[min(l, len(hs) - 1)]) for l in range(1, n)]
    small = [(1, 1), (2, 1), (1, 2), (2, 2), (ws[1], 1), (1, hs[1]), (ws[1], 2), (2, hs[1])]
    return {"pow2": list(dict.fromkeys(level + small)),
            "one pass": [(bw, hs[1]), (bw, 2), (bw, 1), (ws[1], bh), (2, bh), (1, bh)],
            "odd": [(5, 3), (bw - 1, bh - 1)],
            "clone": [(bw, bh)]}


def all_pairs(bw, bh):
    return [p for cl in pairs(bw, bh).values() for p in cl]


def items(bw, bh, channels, classes=None, pattern_names=None):
    """[(pattern, tw, th)] over the pairs of `classes` (all by default): every pattern of each pair, or those of `pattern_names`
    that the pair has (a one-pixel name needs its index inside the tile)"""
    out = []
    for cl, ps in pairs(bw, bh).items():
        if classes is not None and cl not in classes:
            continue
        for tw, th in ps:
            have = names(tw, th, channels)
            out += [(n, tw, th) for n in (have if pattern_names is None else pattern_names) if n in have]
    return out


def group_items(specials, fillers, cols):
    """Row-major items for a grid of `cols` (even) full columns in which every 2x2 group of tiles -- what one wave of the 16x16
    kernel takes -- holds exactly one of `specials`, at position (group number mod 4) of the group, and three of `fillers`."""
    assert cols % 2 == 0
    gcols = cols // 2
    out, f = [], 0
    for r in range(2 * -(-len(specials) // gcols)):
        for c in range(cols):
            g = (r // 2) * gcols + c // 2
            if g < len(specials) and (r & 1) * 2 + (c & 1) == g % 4:
                out.append(specials[g])
            else:
                out.append(fillers[f % len(fillers)])
                f += 1
    return out


def layout(items_, bw, bh, channels, cols=None):
    """The (pattern, tw, th) of `items_` as the full tiles of one frame, row-major, over and over until the grid of cols x rows full
    tiles is full (cols: as square as it gets when None).  The last column of tiles is 7 px wide and the last row 5 px high, as in
    value_patterns.frame: the ragged tiles carry the patterns that come next, at stored sizes clipped to their place.
    Returns (width, height, tile_w uint32[T], tile_h uint32[T], slots uint8[T, bw*bh*channels], names[T]): a name is
    "<pattern> <tw>x<th>"."""
    items_ = list(items_)
    if cols is None:
        cols = int(np.ceil(np.sqrt(len(items_))))
    rows = -(-len(items_) // cols)
    W, H = cols * bw + 7, rows * bh + 5
    return (W, H) + fill(items_, W, H, bw, bh, channels)


def fill(items_, width, height, bw, bh, channels):
    """layout() for an image whose size is given: the items over the full tiles of its grid, row-major, then over the ragged ones,
    clipped to their place -> (tile_w, tile_h, slots, names)"""
    items_ = list(items_)
    cols, rows = -(-width // bw), -(-height // bh)
    T = cols * rows
    tile_w, tile_h = np.zeros(T, np.uint32), np.zeros(T, np.uint32)
    slots = np.zeros((T, bw * bh * channels), np.uint8)
    tile_names = [None] * T
    place = lambda r, c: (min(bw, width - c * bw), min(bh, height - r * bh))  # noqa: E731
    cells = [(r, c) for r in range(rows) for c in range(cols)]
    order = [rc for rc in cells if place(*rc) == (bw, bh)] + [rc for rc in cells if place(*rc) != (bw, bh)]
    for k, (r, c) in enumerate(order):
        name, tw, th = items_[k % len(items_)]
        fw, fh = place(r, c)
        tw, th = min(tw, fw), min(th, fh)
        if name not in names(tw, th, channels):      # a one-pixel index beyond the clipped tile: its last pixel instead
            name = f"{name.split(' @')[0]} @{tw * th - 1}"
        t = r * cols + c
        tile_w[t], tile_h[t] = tw, th
        slots[t, : tw * th * channels] = stored(name, tw, th, channels).ravel()
        tile_names[t] = f"{name} {tw}x{th}"
    return tile_w, tile_h, slots, tile_names
