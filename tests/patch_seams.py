"""Directed inputs for the two pieces of the patch that own their address arithmetic -- the overlay of patch_kernel (step 4,
pxz_patch.hip) and the splice (splice_*_kernel there, the piece list of pxz_splice_windows_device in pxz_api.cpp) -- and plain
restatements of that arithmetic, so that tests/test_patch_seams_host.py can assert on the CPU that every input reaches the class it
is named for and tests/test_gpu_patch_seams.py compares the kernels on inputs that discriminate.  The expected tiles and files
always come from patch_model / test_gpu_patch.model(), the oracle's expand, overlay, shrink and container writer.  No GPU and no
torch here; test_gpu_patch (for model() and records()) is imported where it is first needed."""
from collections import namedtuple

import numpy as np

import patch_model as pm

CHUNK = 16384  # kSpliceChunk: bytes of the output a block of splice_copy_kernel moves at a time
GUARD = 64
POISON = 0xA5


def _tp():
    import test_gpu_patch
    return test_gpu_patch


# ---- restatements ----------------------------------------------------------------------------------------------------------------

Row = namedtuple("Row", "at src_mod same head body tail row_bytes")
Part = namedtuple("Part", "rows n_rows whole interior tile_rect")


def overlay_classes(window, tile_rect, C, pitch, offset):
    """patch_kernel step 4 in plain integers for the part of one tile (tile_rect = (px0, py0, w, h) in image pixels, w and h the
    tile's full size) that lies inside window = (x, y, width, height), whose pixels stand at `offset` of a 16-byte aligned buffer
    with `pitch` bytes between rows.  Per row of the part: `at` (the row's place in the tile image, (row * w + cx0) * C), the
    source address modulo 4, whether the two agree (`same`: the dword body with a byte head and tail; else one byte loop, for
    which head and body are 0 and tail is the whole row), head, body (dwords), tail."""
    x, y, w, h = window
    px0, py0, tw, th = tile_rect
    cx0, cy0 = max(x - px0, 0), max(y - py0, 0)
    cx1, cy1 = min(x + w - px0, tw), min(y + h - py0, th)
    assert cx0 < cx1 and cy0 < cy1, "the window does not cover this tile"
    row_bytes = (cx1 - cx0) * C
    first = offset + (py0 + cy0 - y) * pitch + (px0 + cx0 - x) * C
    rows = []
    for row in range(cy0, cy1):
        s = first + (row - cy0) * pitch
        at = (row * tw + cx0) * C
        head = body = 0
        same = (s & 3) == (at & 3)
        if same:
            head = min((4 - (at & 3)) & 3, row_bytes)
            body = (row_bytes - head) >> 2
        rows.append(Row(at, s & 3, same, head, body, row_bytes - head - 4 * body, row_bytes))
    whole = (cx0, cy0, cx1, cy1) == (0, 0, tw, th)
    interior = cx0 > 0 and cy0 > 0 and cx1 < tw and cy1 < th
    return Part(rows, cy1 - cy0, whole, interior, tile_rect)


def overlay_parts(size, bw, bh, C, window):
    """overlay_classes for every tile that window = (image, x, y, w, h, pitch, offset) covers in an image of `size`"""
    cols = -(-size[0] // bw)
    out = []
    for t in pm.covered_tiles(window[1:5], size, bw, bh):
        tx, ty = t % cols, t // cols
        rect = (tx * bw, ty * bh, min(bw, size[0] - tx * bw), min(bh, size[1] - ty * bh))
        out.append(overlay_classes(window[1:5], rect, C, window[5], window[6]))
    return out


Piece = namedtuple("Piece", "image kind lo hi length")


def splice_pieces(sizes, rects, bw, bh, old=None, new=None):
    """The piece list of pxz_splice_windows_device (pxz_api.cpp, the loop over the images under "the structure of every new
    file", lines 3643-3676) for rects = [(image, x, y, w, h), ...]: per image without a window one "file" piece; otherwise a
    "header" piece (file start .. row 0), then per touched tile row and per window in it by first column a "gap" piece
    (cursor .. the first covered record) -- unless the cursor stands at this row's start and the window starts in column 0, the
    at_row_start rule -- and a "staging" piece, the cursor moving to the next row's start when the window reaches the last column
    and behind its last record otherwise; at the end a "tail" piece unless the cursor stands behind the last row.
    Bounds are ("file_start",), ("file_end",), ("row", r), ("rec_start", tile), ("rec_end", tile) with the image's tile numbers;
    a staging piece has lo = ("stage", first tile) and hi = ("stage_end", last tile).  With old and new (the old files and the
    expected new ones, bytes) every piece carries its length, from their record tables (test_gpu_patch.records)."""
    pieces = []
    for i, (W, H) in enumerate(sizes):
        mine = [r for r in rects if r[0] == i]
        if not mine:
            pieces.append((i, "file", ("file_start",), ("file_end",)))
            continue
        cols, n_rows = -(-W // bw), -(-H // bh)
        cursor = ("row", 0)
        pieces.append((i, "header", ("file_start",), cursor))
        touched = {}
        for r in mine:
            c0, r0, cc, cr = pm.covered(r[1:5], bw, bh)
            for j in range(cr):
                touched.setdefault(r0 + j, []).append((c0, cc))
        for r in sorted(touched):
            for c0, cc in sorted(touched[r]):
                t0, t1 = r * cols + c0, r * cols + c0 + cc - 1
                if not (cursor == ("row", r) and c0 == 0):
                    pieces.append((i, "gap", cursor, ("rec_start", t0)))
                pieces.append((i, "staging", ("stage", t0), ("stage_end", t1)))
                cursor = ("row", r + 1) if c0 + cc == cols else ("rec_end", t1)
        if cursor != ("row", n_rows):
            pieces.append((i, "tail", cursor, ("file_end",)))
    if old is None:
        return [Piece(*p, None) for p in pieces]
    records = _tp().records
    tables = {}

    def tab(i):
        if i not in tables:
            tables[i] = (records(old[i]), records(new[i]))
        return tables[i]

    def at(i, bound):
        if bound[0] == "file_start":
            return 0
        if bound[0] == "file_end":
            return len(old[i])
        rec = tab(i)[0]
        if bound[0] == "row":
            t = bound[1] * -(-sizes[i][0] // bw)
            return rec[t][0] if t < len(rec) else len(old[i])
        return rec[bound[1]][0] + (rec[bound[1]][1] if bound[0] == "rec_end" else 0)

    out = []
    for (i, kind, lo, hi) in pieces:
        if kind == "staging":
            n = sum(tab(i)[1][t][1] for t in range(lo[1], hi[1] + 1))
        else:
            n = at(i, hi) - at(i, lo)
        assert n >= 0
        out.append(Piece(i, kind, lo, hi, n))
    return out


def piece_offsets(pieces):
    """the output offset of every piece boundary: len(pieces) + 1 values"""
    return [0] + np.cumsum([p.length for p in pieces]).tolist()


# ---- sources ---------------------------------------------------------------------------------------------------------------------

class Src:
    """one file of a call (test_gpu_patch.Source's fields)"""

    def __init__(self, raw, w, h):
        self.raw, self.w, self.h = raw, w, h


def noise(w, h, c, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, c)).astype(np.uint8)


def encode(oracle, img, bw, bh, p):
    h, w, c = img.shape
    v, tw, th, slots = oracle.shrink_image(img, bw, bh, p.mode, p.filt, p.factor)
    return Src(oracle.encode_container(w, h, bw, bh, c, 0, v, None, tw, th, slots), w, h)


_tiny = {}


def tiny_file(oracle, c, bw, bh):
    """a valid .pixlzr file of one tile: 4x4 px of one colour"""
    if (c, bw, bh) not in _tiny:
        img = np.full((4, 4, c), 200, np.uint8)
        _tiny[c, bw, bh] = encode(oracle, img, bw, bh, pm.Params(pm.DIRECTIONAL, pm.LANCZOS3, 10.0, pm.LANCZOS3)).raw
    return _tiny[c, bw, bh]


def filler(oracle, c, bw, bh, length):
    """A valid one-tile .pixlzr file (4x4 px of one colour) followed by padding inside its span, `length` bytes in all.  As an image
    without a window it is one file_start .. file_end piece of the splice, copied unread, and shifts every later output offset by
    `length`: this puts a chosen piece boundary on a chosen offset modulo 16384 and modulo 16."""
    tiny = tiny_file(oracle, c, bw, bh)
    assert length >= len(tiny), (length, len(tiny))
    return Src(tiny + bytes((k * 29 + 7) & 255 for k in range(length - len(tiny))), 4, 4)


class Call:
    """one call's inputs; the expected files and tiles are computed once"""

    def __init__(self, sources, c, bw, bh, p, rects, patches):
        self.sources, self.c, self.bw, self.bh, self.p, self.rects, self.patches = sources, c, bw, bh, p, rects, patches
        self.sizes = [(s.w, s.h) for s in sources]
        self._want = None

    def want(self, oracle):
        if self._want is None:
            self._want = _tp().model(oracle, self.sources, self.c, self.p, self.rects, self.patches)
        return self._want

    def pieces(self, oracle):
        return splice_pieces(self.sizes, self.rects, self.bw, self.bh, [s.raw for s in self.sources], self.want(oracle)[0])


_calls = {}


def cached(key, make):
    if key not in _calls:
        _calls[key] = make()
    return _calls[key]


# ---- the overlay sweep -----------------------------------------------------------------------------------------------------------

# Noise under noise.  On the CPU the oracle keeps every tile of uniform noise at full size for shrink_by at any factor from 0.3 up
# (its level is 1.1 * factor at the least on these geometries and clamps at 1) and for shrink_directionally from 10 up (0.17 *
# factor at the least; at 1.0 and below every tile came out small): 1.0 and 20.0 leave a margin, and test_patch_seams_host.py
# asserts that every covered tile of the sweep is stored at full size after the patch.
NOISE_FACTOR = {pm.SHRINK_BY: 1.0, pm.DIRECTIONAL: 20.0}
FIXTURE_FACTOR = {pm.SHRINK_BY: 0.3, pm.DIRECTIONAL: 10.0}  # patch_model.FIXTURES': ramps come out small, noise stays whole
SMALL = (101, 51, 16, 8)   # 7x7 tiles, the last column 5 px wide, the last row 3 px tall
LONG = (202, 71, 96, 32)   # 3x3 tiles, the last column 10 px wide, the last row 7 px tall
VARIANTS = {SMALL: (0, 1), LONG: (0, 3)}  # added to every window's offset class: the second placement trades agreeing rows for others


def small_windows():
    """(x, y, w, h, ("abs", offset mod 4) | ("rel", offset - at of the first row, mod 4), pitch mod 4): 16 windows with the 16
    (offset, pitch) classes in tiles of their own -- left offsets 0..3 chosen so that an RGB window's first row agrees, widths 1..6,
    heights from 1 row to 13 (two tile rows) -- and directed ones behind them"""
    out = []
    heights = (1, 2, 3, 5, 7, 8, 11, 13)
    for k in range(16):
        off, pitch = k % 4, k // 4
        cx0, cy0 = (3 * off) % 4, k % 3
        col, trow = k % 6, 2 * (k // 6)
        out.append((16 * col + cx0, 8 * trow + cy0, 1 + k % 6, heights[(k + k // 8) % 8], ("abs", off), pitch))
    out += [
        (76, 33, 4, 2, ("rel", 0), 0),    # reaches its tile's right edge (tile (4, 4))
        (78, 41, 5, 3, ("rel", 1), 2),    # crosses the seam between tiles (4, 5) and (5, 5)
        (80, 32, 16, 8, ("rel", 0), 0),   # tile (5, 4) wholly
        (97, 1, 3, 5, ("rel", 0), 3),     # the 5 px wide last column: `at` changes its class from row to row
        (96, 8, 5, 8, ("rel", 2), 1),     # a ragged tile wholly
        (96, 17, 5, 6, ("rel", 0), 3),    # 15 bytes a row in the tile and in the buffer: RGB rows agree, with every head in turn
        (3, 48, 6, 3, ("rel", 0), 0),     # the 3 px tall last row
        (99, 49, 2, 2, ("rel", 3), 0),    # the corner tile
        (19, 48, 1, 3, ("abs", 1), 0),    # one pixel a row at at & 3 == 1: RGB's head is the whole row
        (32, 48, 1, 3, ("abs", 0), 0),    # one pixel a row at at & 3 == 0: no head, no body, a tail
        (50, 49, 5, 2, ("rel", 0), 0),    # RGB: head 2, body 3, tail 1
        (65, 48, 4, 3, ("rel", 0), 0),    # RGB: head 1, body 2, tail 3
    ]
    return out


def long_windows():
    return [
        (0, 1, 96, 30, ("rel", 0), 0),      # the tile's whole width: 72 (RGB) and 96 (RGBA) dwords a row
        (127, 0, 65, 9, ("rel", 0), 0),     # 65 px: RGB head 3, RGBA 65 dwords
        (5, 35, 80, 5, ("rel", 1), 0),      # disagreeing, 240 / 320 bytes
        (106, 34, 86, 20, ("rel", 1), 0),   # disagreeing, 258 / 344 bytes
        (76, 65, 90, 5, ("rel", 2), 0),     # across a seam in the 7 px tall last row: parts of 20 and 70 px
        (194, 3, 7, 20, ("rel", 0), 2),     # the 10 px wide last column
        (192, 32, 10, 32, ("rel", 0), 1),   # a ragged tile wholly
    ]


def place(specs, size, bw, bh, c, patches, variant=0):
    """the windows' new pixels in one buffer (to be uploaded to a 16-byte aligned address) with every window at its directed
    (offset mod 4, pitch mod 4) -> (windows with pitch and offset, host buffer).  This is the caller-made placement of Chain."""
    cols = -(-size[0] // bw)
    windows, cursor = [], GUARD
    for (x, y, w, h, (how, a), pm4), px in zip(specs, patches):
        if how == "rel":
            t = pm.covered_tiles((x, y, w, h), size, bw, bh)[0]
            tx, ty = t % cols, t // cols
            tw = min(bw, size[0] - tx * bw)
            a += ((max(y - ty * bh, 0) * tw + max(x - tx * bw, 0)) * c)
        off = ((cursor + 15) & ~15) + ((a + variant) & 3)
        pitch = w * c + 4 + len(windows) % 3 * 4
        pitch += (pm4 - pitch) & 3
        windows.append((0, x, y, w, h, pitch, off))
        cursor = off + pitch * h + GUARD
    buf = np.full(cursor, POISON, np.uint8)
    for (_, _, _, w, h, pitch, off), px in zip(windows, patches):
        np.lib.stride_tricks.as_strided(buf[off:], (h, w, c), (pitch, c, 1))[...] = px
    return windows, buf


def overlay_call(oracle, geom, c, mode, filt=pm.LANCZOS3, fixtures_factors=False):
    """one image of `geom` and every window of its list.  Noise under noise at NOISE_FACTOR, or, with fixtures_factors, the
    fixtures' picture (ramps and noise), new pixels and factors, where covered tiles are resampled"""
    def make():
        W, H, bw, bh = geom
        specs = small_windows() if geom == SMALL else long_windows()
        rects = [(0,) + s[:4] for s in specs]
        if fixtures_factors:
            p = pm.Params(mode, filt, FIXTURE_FACTOR[mode], filt)
            img = pm.picture(W, H, c, bw, bh, 31 + c)
            patches = [pm.new_pixels(r[1:], c, 21) for r in rects]
        else:
            p = pm.Params(mode, filt, NOISE_FACTOR[mode], filt)
            img = noise(W, H, c, 1000 + c + 10 * mode)
            patches = [noise(r[3], r[4], c, 2000 + k) for k, r in enumerate(rects)]
        call = Call([encode(oracle, img, bw, bh, p)], c, bw, bh, p, rects, patches)
        call.specs = specs
        return call
    return cached(("overlay", geom, c, mode, filt, fixtures_factors), make)


# ---- the splice: piece-list shapes -----------------------------------------------------------------------------------------------

SPLICE_CONFIGS = {"rgb-by": (3, pm.SHRINK_BY), "rgba-directional": (4, pm.DIRECTIONAL), "rgb-directional": (3, pm.DIRECTIONAL), "rgba-by": (4, pm.SHRINK_BY)}
B = 8  # the splice cases' block side


def splice_params(mode):
    return pm.Params(mode, pm.LANCZOS3, FIXTURE_FACTOR[mode], pm.LANCZOS3)


def pictures(oracle, sizes, c, p, seed):
    return [encode(oracle, pm.picture(w, h, c, B, B, seed + k), B, B, p) for k, (w, h) in enumerate(sizes)]


def finish(sources, c, p, rects, seed):
    return Call(sources, c, B, B, p, rects, [pm.new_pixels(r[1:], c, seed) for r in rects])


def many_pieces(oracle, config):
    """4 images of 320x112 (40x14 tiles) with a window of 1..3 px a side in every other tile, passed in an order that is not file
    order: a gap and a staging piece per window, more than 2048 pieces"""
    def make():
        c, mode = SPLICE_CONFIGS[config]
        p = splice_params(mode)
        rects = []
        for i in range(4):
            for ty in range(14):
                for tx in range(40):
                    if (tx + ty) % 2 == 0:
                        k = len(rects)
                        rects.append((i, B * tx + k % 6, B * ty + k % 5, 1 + k % 3, 1 + (k // 3) % 3))
        order = np.random.default_rng(5).permutation(len(rects))
        return finish(pictures(oracle, [(320, 112)] * 4, c, p, 300), c, p, [rects[k] for k in order], 31)
    return cached(("many", config), make)


TALL = (22, 1045)  # 3 columns (the last 6 px wide) x 131 tile rows (the last 5 px tall)
TALL_ROWS = (0, 63, 64, 65, 127, 128, 130)


def tall(oracle, config):
    """windows in the tile rows around the 64-entry trips of splice_line_sum and in the last one: the first and the last in column
    0, the others in the last column, so that the gaps behind them start at a row bound: sums of 64, 65, 66, 128 and 129 entries"""
    def make():
        c, mode = SPLICE_CONFIGS[config]
        p = splice_params(mode)
        rects = [(0, (0, 17)[0 < k < 6] + k % 3, B * r + k % 4, 2, 1 + k % 3 if r < 130 else 2) for k, r in enumerate(TALL_ROWS)]
        return finish(pictures(oracle, [TALL], c, p, 400), c, p, rects, 32)
    return cached(("tall", config), make)


def tall_every_row(oracle, config):
    """two such images with a window in every tile row, in columns 0, 2, 1 in turn (a gap from a row bound every third row): 262
    touched rows"""
    def make():
        c, mode = SPLICE_CONFIGS[config]
        p = splice_params(mode)
        rects = [(i, B * ((2 * r + i) % 3) + 1, B * r + r % 3, 2 + r % 2, 2) for i in range(2) for r in range(131)]
        return finish(pictures(oracle, [TALL, TALL], c, p, 410), c, p, rects, 33)
    return cached(("tall every row", config), make)


WRAP = (38, 45)  # 5 columns (the last 6 px wide) x 6 tile rows (the last 5 px tall)
WRAP_RECTS = [
    (0, 1, 1, 2, 2),      # column 0 of row 0: at_row_start from the first cursor
    (0, 10, 9, 3, 3),     # row 1: tile (1, 1) ...
    (0, 17, 10, 2, 4),    # ... its neighbour (2, 1): a gap of no bytes between them ...
    (0, 33, 12, 4, 2),    # ... and the last column, three in one row; the cursor moves to row 2's start
    (0, 2, 18, 5, 3),     # column 0 of row 2: at_row_start from a moved cursor, no gap piece
    (0, 9, 25, 10, 18),   # columns 1..2 of rows 3..5
    (0, 2, 34, 3, 3),     # one row, beside the middle row of the window above
    (0, 33, 41, 2, 2),    # the last tile of the last row: no tail piece
]


def wrapping(oracle, config):
    def make():
        c, mode = SPLICE_CONFIGS[config]
        p = splice_params(mode)
        return finish(pictures(oracle, [WRAP], c, p, 420), c, p, WRAP_RECTS, 34)
    return cached(("wrapping", config), make)


FLAGGED_SIZES = [(30, 20), (19, 11), (38, 45), (8, 8), (27, 30)]
FLAGGED_RECTS = [(0, 9, 9, 2, 2), (1, 1, 1, 3, 3), (2, 9, 1, 2, 2), (2, 17, 10, 2, 4), (2, 33, 41, 2, 2), (3, 0, 0, 8, 8), (4, 10, 20, 9, 5)]
FLAGGED_WINDOW = 3  # the window of the middle file whose one tile the test breaks


def flagged(oracle, config):
    """five files; the middle one carries three windows, so that once it is flagged seven of its pieces have no bytes"""
    def make():
        c, mode = SPLICE_CONFIGS[config]
        p = splice_params(mode)
        return finish(pictures(oracle, FLAGGED_SIZES, c, p, 430), c, p, FLAGGED_RECTS, 35)
    return cached(("flagged", config), make)


# ---- the splice: chunk, alignment and capacity sweeps ----------------------------------------------------------------------------

SEAM_DELTAS = (-17, -16, -15, -1, 0, 1, 15, 16, 17)
SEAM_BOUNDARIES = ("file start", "staging start", "staging end")


def windowed(oracle):
    """the rgb-32-by fixture with its "corner" window, tiles (0..1, 0..1): header, staging, gap, staging, tail"""
    def make():
        f = pm.fixture(oracle, "rgb-32-by")
        rect = (0,) + f.windows()["corner"][0]
        call = Call([Src(f.raw, f.w, f.h)], f.c, f.bw, f.bh, f.p, [rect], [pm.new_pixels(rect[1:], f.c, 41)])
        call.fixture = f
        return call
    return cached("windowed", make)


def behind_filler(oracle, length):
    """the windowed file as the second file of a call, behind a filler of `length` bytes; expected: the filler, then the model's file"""
    base = windowed(oracle)
    f = base.fixture
    call = Call([filler(oracle, f.c, f.bw, f.bh, length), base.sources[0]], f.c, f.bw, f.bh, f.p, [(1,) + base.rects[0][1:]], base.patches)
    call._want = ([call.sources[0].raw, base.want(oracle)[0][0]], base.want(oracle)[1])
    return call


def min_filler(oracle):
    f = windowed(oracle).fixture
    return len(tiny_file(oracle, f.c, f.bw, f.bh))


def seam_boundary(oracle, which):
    """the offset of a boundary inside the windowed file's output: its first byte, the start of its first staging piece, the end of
    its last one"""
    pieces = windowed(oracle).pieces(oracle)
    offs = piece_offsets(pieces)
    staging = [k for k, p in enumerate(pieces) if p.kind == "staging"]
    return {"file start": 0, "staging start": offs[staging[0]], "staging end": offs[staging[-1] + 1]}[which]


def seam_filler_length(oracle, which, d):
    """the filler's length that puts the boundary on 16384 * m + d, m the smallest that leaves room for the filler's file"""
    at = seam_boundary(oracle, which)
    m = 1
    while CHUNK * m + d - at < min_filler(oracle):
        m += 1
    return CHUNK * m + d - at


ALIGN_FILLER = 331
ALIGN_LEADS = (0, 5, 8, 15)


def cap_filler(oracle):
    """the filler's length for the capacity sweep: the windowed file's longest piece starts one byte behind a multiple of 16, so
    that 1, 15, 16 and 17 bytes into it are inside its head, at its head's end and in its body"""
    pieces = windowed(oracle).pieces(oracle)
    offs = piece_offsets(pieces)
    longest = max(range(len(pieces)), key=lambda k: pieces[k].length)
    n = min_filler(oracle)
    while (n + offs[longest]) % 16 != 1:
        n += 1
    return n


def capacities(oracle, lead_file):
    """{capacity: what it is} for the capacity sweep of a call whose windowed file starts at output offset lead_file"""
    call = windowed(oracle)
    pieces = call.pieces(oracle)
    offs = piece_offsets(pieces)
    out = {}
    for k, o in enumerate(offs):
        for d in (-1, 0, 1):
            if d <= 0 or k < len(pieces):
                out.setdefault(lead_file + o + d, f"piece boundary {k} {d:+d}")
    longest = max(range(len(pieces)), key=lambda k: pieces[k].length)
    for d in (1, 15, 16, 17):
        out.setdefault(lead_file + offs[longest] + d, f"{d} bytes into the longest piece ({pieces[longest].kind})")
    row = pm.covered(call.rects[0][1:5], call.bw, call.bh)[1]
    for b in range(5):
        out.setdefault(lead_file + 26 + 4 * row + b, f"{b} bytes of the line-table entry of row {row}")
    return out


def copy_spans(offsets, capacity=None, skew=0):
    """splice_copy_kernel in plain integers: for boundaries `offsets` (piece_offsets) and an output view that starts `skew` bytes
    behind a multiple of 16, every (piece, a, b, head, body, tail) a block moves: the piece's bytes [a, b) inside one 16 KB chunk
    below the capacity, as a byte head up to the next multiple of 16 of the destination, 16-byte stores and a byte tail"""
    total = offsets[-1]
    lim = total if capacity is None else min(total, capacity)
    out = []
    for c0 in range(0, lim, CHUNK):
        c1 = min(c0 + CHUNK, lim)
        for p in range(len(offsets) - 1):
            d0, d1 = offsets[p], offsets[p + 1]
            a, b = max(d0, c0), min(d1, c1)
            if a >= b:
                continue
            n = b - a
            head = min((16 - (a + skew) % 16) % 16, n)
            body = (n - head) >> 4
            out.append((p, a, b, head, body, n - head - 16 * body))
    return out
