"""Position sweeps for the stream kernels' seams (tests/test_stream_seams_host.py, tests/test_gpu_stream_seams.py).

The device writer cuts a tile's QOI stream into segments and stitches them together, the reader walks rows of records in staged
chunks and batches and consumes ops through refilled windows.  Instead of aiming at those joins, every family below puts ONE
event -- a run's end, a run's start, a run of one, an index eviction, the end of a gradient -- at pixel position p of a tile, and
a sweep is one tile per p: whatever the segmentation of a stored size is, every one of its seams meets the event.  The tests
know no kernel constant; a failure names the family, the stored size and p.

Everything here is pure numpy and deterministic: no random numbers, no state between calls."""
import numpy as np

FAMILIES = ("run|lit", "lit|run", "run|run", "run|run black", "run|run zero", "odd one", "evict", "grad|run")

# Stored sizes in 64x64 slots, every family, RGBA and RGB.  (w, h, why)
SIZES_64 = [
    (64, 64, "4096 px: the full slot, the largest number of segments; 4097 tiles cross the 4096-tile blocks of the scans"),
    (40, 25, "1000 px: the last segment is shorter than the others"),
    (50, 41, "2050 px: the segment length rounds up so far that a trailing segment stays empty"),
    (17, 15, "255 px: one below a power of two, odd width and height"),
    (13, 10, "130 px: just above the smallest size that is cut at all"),
    (16, 8, "128 px: the smallest size that is cut, segments of equal length"),
    (9, 7, "63 px: a single segment, one pixel above a run's flush at 62"),
]
# Stored sizes in 128x128 slots: RGBA with run|lit and the three run|run variants, RGB with run|lit.
SIZES_128 = [
    (128, 128, "16384 px: the full slot, the longest segments"),
    (82, 50, "4100 px: three trailing segments stay empty"),
    (91, 90, "8190 px: segments of 128 pixels, the last one short by two"),
]
FAMILIES_128 = {4: ("run|lit", "run|run", "run|run black", "run|run zero"), 3: ("run|lit",)}

# the colours of the runs: none of them is a literal pixel (their g, RGB: their r, is 64 or more: see literals())
COLOUR_A = (200, 100, 50, 77)
COLOUR_B = (90, 180, 20, 200)
BLACK = (0, 0, 0, 255)   # the encoder's implicit previous pixel: a stream that opens with it opens with a run
ZERO = (0, 0, 0, 0)      # what the index holds before anything is written to it: the first such pixel is an INDEX hit
# evict: three colours with three different QOI hashes; RGBA: three different alphas, so that every op that is no INDEX is an RGBA op
CYCLE = ((10, 70, 200, 40), (150, 220, 30, 120), (80, 5, 111, 250))


def families_of(c):
    """(0, 0, 0, 0) needs an alpha channel: RGB pixels are opaque and never equal the index's initial entries"""
    return tuple(f for f in FAMILIES if c == 4 or f != "run|run zero")


def qoi_hash(px):
    px = [int(v) for v in px]
    return (px[0] * 3 + px[1] * 5 + px[2] * 7 + (px[3] if len(px) == 4 else 255) * 11) % 64


def colour(rgba, c):
    return np.array(rgba[:c], np.uint8)


def literals(n, c):
    """n pixels that each cost a full RGBA (c = 4) or RGB (c = 3) op, wherever in a tile they start.  Pixel i is distinct from
    every other one, so nothing hits the index: RGBA has i in (r, g), RGB in (g, r) with g a bijection of i mod 256.  RGBA: alpha
    moves by 37 at every pixel and starts at 1, not at the implicit 255.  RGB: green moves by 67 (mod 256) at every pixel and
    starts at 100, a step that neither DIFF (-2..1) nor LUMA (-32..31) can say.  n <= 16384 keeps g (RGB: r) below 64, so no
    literal is one of the run colours."""
    assert n <= 16384
    i = np.arange(n, dtype=np.int64)
    px = np.zeros((n, c), np.uint8)
    if c == 4:
        px[:, 0], px[:, 1], px[:, 2], px[:, 3] = i & 255, i >> 8, (i * 13) & 255, (i * 37 + 1) & 255
    else:
        # (g alone has period 256; r = i >> 8 tells the periods apart)
        px[:, 0], px[:, 1], px[:, 2] = i >> 8, (i * 67 + 100) & 255, (i * 13) & 255
    return px


def gradient(n, c):
    """n pixels, each one step of +-1..2 per colour channel from the one before (never zero: no pixel repeats), alpha
    constant: DIFF where all three steps are -2..1, LUMA otherwise, now and then an INDEX hit -- ops of one or two bytes"""
    i = np.arange(n)
    steps = np.stack([np.array([1, 2, 1, -1, 2])[i % 5], np.array([2, 1, -2, 1, 1, 2, -1])[i % 7],
                      np.array([-1, 2, 1, 1, -2, 2, 1, 1, 2, -1, 1])[i % 11]], axis=1)
    px = np.full((n, c), 255, np.uint8)
    px[:, :3] = (np.cumsum(steps, axis=0) + np.array([40, 90, 160])) & 255
    return px


def intruder_of(px):
    """the same QOI hash (r * 3: 64 * 3 is a multiple of 64), another colour"""
    out = np.array(px, np.uint8).copy()
    out[0] = (int(out[0]) + 64) & 255
    return out


def sweep(family, n, c, positions):
    """the tiles of `family` for every p in positions: uint8 [len(positions), n, c]"""
    assert family in families_of(c), (family, c)
    p = np.asarray(positions, np.int64)[:, None]
    assert p.min() >= 0 and p.max() <= n
    i = np.arange(n)[None, :]
    before = (i < p)[..., None]
    A, B = colour(COLOUR_A, c), colour(COLOUR_B, c)
    if family == "run|lit":
        return np.where(before, A, literals(n, c)[None])
    if family == "lit|run":
        return np.where(before, literals(n, c)[None], A)
    if family.startswith("run|run"):
        first = {"run|run": A, "run|run black": colour(BLACK, c), "run|run zero": colour(ZERO, c)}[family]
        return np.where(before, first, B)
    if family == "odd one":
        return np.where((i == p)[..., None], B, A)   # (p = n: the plain tile)
    if family == "grad|run":
        return np.where(before, gradient(n, c)[None], A)
    assert family == "evict"
    cyc = np.array([q[:c] for q in CYCLE], np.uint8)
    assert len({qoi_hash(q[:c]) for q in CYCLE}) == 3
    base = cyc[np.arange(n) % 3]
    intr = np.stack([intruder_of(q) for q in cyc])[np.arange(n) % 3]  # pixel p's own colour with r + 64: evicts it
    return np.where((i == p)[..., None], intr[None], base[None])


def tile(family, w, h, c, p):
    """one tile: uint8 [h, w, c]"""
    return sweep(family, w * h, c, [p])[0].reshape(h, w, c)


def positions_of(w, h):
    """every p in 0..n up to 4160 pixels and for 91x90; 128x128: every p in 0..600 and n-600..n, and k*256 + d for k = 1..63,
    d = -3..3 -- around every multiple of the longest segment and of every shorter power of two"""
    n = w * h
    if (w, h) != (128, 128):
        return list(range(n + 1))
    s = set(range(601)) | set(range(n - 600, n + 1)) | {k * 256 + d for k in range(1, 64) for d in range(-3, 4)}
    return sorted(s)


def parts_of(w, h, slot_bytes, limit=112 << 20):
    """the sweep's positions in runs whose slots stay below `limit` bytes: what one test case uploads"""
    pos = positions_of(w, h)
    per = max(1, limit // slot_bytes)
    k = -(-len(pos) // per)
    size = -(-len(pos) // k)
    return [pos[j:j + size] for j in range(0, len(pos), size)]


class Frame:
    """tiles of any stored sizes as one frame of bw x bh slots: the image is cols*bw x rows*bh, so no edge tile limits a stored
    size.  Spare tiles of the last row are 1x1 (spare = None) or copies of tile `spare`.  Values are arbitrary, all different."""

    def __init__(self, tiles, sizes, bw, bh, c, cols, spare=None):
        m = len(tiles)
        self.bw, self.bh, self.c, self.cols, self.rows = bw, bh, c, cols, -(-m // cols)
        self.m, self.T = m, self.cols * self.rows
        self.W, self.H = self.cols * bw, self.rows * bh
        self.tw, self.th = np.ones(self.T, np.uint32), np.ones(self.T, np.uint32)
        self.slots = np.zeros((self.T, bw * bh * c), np.uint8)
        self.slots[m:, :c] = colour(COLOUR_B, c)
        for t in range(m):
            w, h = sizes[t]
            self.tw[t], self.th[t] = w, h
        same = len(set(sizes)) == 1
        if same and isinstance(tiles, np.ndarray):
            self.slots[:m, : tiles.shape[1] * c] = tiles.reshape(m, -1)
        else:
            for t in range(m):
                self.slots[t, : tiles[t].size] = tiles[t].reshape(-1)
        if spare is not None:
            self.tw[m:], self.th[m:], self.slots[m:] = self.tw[spare], self.th[spare], self.slots[spare]
        self.values = (np.arange(self.T, dtype=np.float32) * np.float32(0.37) - np.float32(5.0)).astype(np.float32)

    def encode(self, oracle):
        return oracle.encode_container(self.W, self.H, self.bw, self.bh, self.c, 0, self.values, None, self.tw, self.th, self.slots)

    def valid(self):
        """which bytes of the slots are stored pixels"""
        return np.arange(self.slots.shape[1])[None, :] < (self.tw.astype(np.int64) * self.th * self.c)[:, None]


def sweep_frame(family, w, h, slot, c, positions, spare=None, cols=None):
    n = w * h
    tiles = sweep(family, n, c, positions)
    return Frame(tiles, [(w, h)] * len(positions), slot, slot, c, cols or (64 if slot == 64 else 32), spare)


MIXED_SIZES = [(64, 64), (40, 25), (50, 41), (13, 10), (9, 7)]


def mixed_frame(family, c):
    """the sweeps of five stored sizes of one family dealt tile by tile, in turn, until each has run out: units that are only
    partly filled, and tiles of every class next to each other in the order the writer sorts by class"""
    sweeps = [(w, h, sweep(family, w * h, c, positions_of(w, h))) for (w, h) in MIXED_SIZES]
    tiles, sizes, labels = [], [], []
    for k in range(max(len(s[2]) for s in sweeps)):
        for (w, h, s) in sweeps:
            if k < len(s):
                tiles.append(s[k]); sizes.append((w, h)); labels.append((w, h, k))
    return Frame(tiles, sizes, 64, 64, c, 64), labels


def records_of(raw, cols, rows):
    """(start, length) of every record of a file, row by row, from the records' own length fields; the line table must agree"""
    pos = 26 + 4 * rows
    out = []
    for r in range(rows):
        row0 = pos
        for _ in range(cols):
            assert raw[pos:pos + 5] == b"block", (r, pos)
            ln = 13 + int.from_bytes(raw[pos + 9:pos + 13], "big")
            out.append((pos - row0, ln))
            pos += ln
        assert pos - row0 == int.from_bytes(raw[26 + 4 * r:30 + 4 * r], "big")
    assert pos == len(raw)
    return out


# ---- rows for the reader's index walk ----------------------------------------------------------------------------------

CHUNK = 8192               # the bytes of a row the index pass stages at a time
SEAM_OFFSETS = range(-40, 9)   # where a record's header starts, relative to a chunk's end: its 23 bytes fit, straddle, or lie behind it


class Sized:
    """lit|run tiles of 32x32 slots by record length: the lengths are measured with the oracle's encoder, never predicted (the
    estimate of five bytes per literal only says where to look)"""

    def __init__(self, oracle):
        self.oracle, self.by_len, self.tried = oracle, {}, set()

    def measure(self, w, h, p):
        # the record: "block", value, length (13 bytes), then the QOI stream without its 4-byte magic
        return 13 + len(self.oracle.qoi_encode(tile("lit|run", w, h, 4, p))) - 4

    def of_length(self, length):
        for w in range(32, 23, -1):
            for h in range(32, 23, -1):
                if length in self.by_len:
                    return self.by_len[length]
                for p in range(max(0, length // 5 - 12), min(w * h, length // 5) + 1):
                    if (w, h, p) not in self.tried:
                        self.tried.add((w, h, p))
                        self.by_len.setdefault(self.measure(w, h, p), (w, h, p))
        assert length in self.by_len, f"no lit|run tile of 32x32 slots has a record of {length} bytes"
        return self.by_len[length]


def walk_frame(oracle, which):
    """one row per offset d in SEAM_OFFSETS.  which = 1: [full, sized, SEAM, after] -- the SEAM record's header starts at
    CHUNK + d from the row's first byte.  which = 2: [full, sized, full, sized, SEAM, after] -- the third record starts at CHUNK
    exactly, so the second chunk begins there whatever the rule for a header at the very end is, and the SEAM record's header
    starts at 2 CHUNK + d.  -> (Frame, seam column)"""
    sized = Sized(oracle)
    full = (32, 32, 1024)   # all literals
    l_full = sized.measure(*full)
    tiles, sizes = [], []
    for d in SEAM_OFFSETS:
        row = [full, sized.of_length(CHUNK + d - l_full)] if which == 1 else \
              [full, sized.of_length(CHUNK - l_full), full, sized.of_length(CHUNK + d - l_full)]
        row += [(32, 32, 500 + d), (7, 5, 20)]   # the seam record and the one behind it
        for (w, h, p) in row:
            tiles.append(tile("lit|run", w, h, 4, p)); sizes.append((w, h))
    cols = 4 if which == 1 else 6
    return Frame(tiles, sizes, 32, 32, 4, cols), cols - 2


BATCH_COLS = (63, 64, 65, 128, 129, 200)   # tiles per row around the 64 records the index pass takes per batch


def batch_frame(cols):
    """three rows of `cols` 1x1 stored tiles in 8x8 slots, every pixel another colour"""
    t = np.arange(3 * cols)
    px = np.stack([t & 255, (t * 7 + 64) & 255, t >> 8, (t * 29 + 3) & 255], axis=1).astype(np.uint8)
    return Frame(px[:, None, :], [(1, 1)] * len(t), 8, 8, 4, cols)


def batch_seams(cols):
    """the records a window ends and starts around: the first of every further batch of 64, and the row's last"""
    return sorted({s for s in (64, 128, 192) if s < cols} | {cols - 1})


def seam_windows(fr, seams):
    """windows over one tile row each: the last column is the record before, at and behind a seam record, the first column is
    the row's first, or lies on either side of the seam record -> [(image 0, x, y, w, h, pitch, offset)], [(row, c0, c1)]"""
    wins, cover = [], []
    for r in range(fr.rows):
        for s in seams:
            for (c0, c1) in ((0, s - 1), (0, s), (0, s + 1), (s - 1, s), (s, s), (s, s + 1), (s + 1, s + 1), (s - 1, s + 1)):
                if 0 <= c0 <= c1 < fr.cols and (r, c0, c1) not in cover:
                    cover.append((r, c0, c1))
                    w = (c1 - c0 + 1) * fr.bw
                    wins.append((0, c0 * fr.bw, r * fr.bh, w, fr.bh, w * fr.c, 0))
    return wins, cover
