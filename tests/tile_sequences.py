"""Frames whose tiles come in a chosen ORDER (tests/test_tile_sequences_host.py, tests/test_gpu_tile_sequences.py).

Every hot kernel is a persistent loop: a wave or block walks many tiles and carries state from one to the next -- the parked
output of the previous tile, prefetched pixels, values that travel two tiles ahead, list batches of 16 entries, the detectors'
software pipeline over batches of 15 / 14 / 3 tiles and the alpha bytes a producer wave keeps from one of them to the next.  The frames here put tile KINDS in a known sequence along the flat tile
order, so that with a small launch (PXZ_CUS, PXZ_WPB, PXZ_CHUNK_LG) one wave meets "a clone followed by a skipped tile", "the
16th listed tile" or "a partial batch after two full ones" by construction.

A kind is what the ORACLE does with a tile (its stored size), never what the product does (section e: the alpha plane laid over a
tile, which is the input itself).  Tiles are drawn from a two-parameter
family -- a 0/1 profile along x times an amplitude plus a profile along y times another -- whose members the oracle classifies;
every draw is a hash of an index (value_patterns.hash32), no generator state is involved."""
import numpy as np

import value_patterns as vp

DIRECTIONAL, SHRINK_BY = 1, 0
LANCZOS3, NEAREST = 4, 0
FACTOR = 16.0      # the benchmark's caller and factor (frames a, c)
BY_FACTOR = 1.0    # shrink_by: noise tiles are stored whole, flat ones are not (asserted on the oracle)
AMPS = (0, 1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64, 96, 128)

# ---- tiles and their kinds ------------------------------------------------------------------------------------------------------

OPAQUE_KINDS = ("whole", "one", "width kept", "height kept", "mid", "narrow", "sliver")
ALPHA, RAGGED = "alpha 254", "ragged"


def kind_of(w, h, bw, bh):
    """the kind of a full bw x bh tile the oracle stores at w x h (for 32x32: whole, 1x1, width kept, height kept, the 16 x (2|1)
    class that shrink32_kernel hands on, narrow w <= 4 and 1 < h <= 16, both sides in 4..16)"""
    if (w, h) == (bw, bh):
        return "whole"
    if (w, h) == (1, 1):
        return "one"
    if w == bw:
        return "width kept"
    if h == bh:
        return "height kept"
    if w == bw // 2 and h <= 2:
        return "sliver"
    if w <= bw // 8 and 1 < h <= bh // 2:
        return "narrow"
    if bw // 8 <= w <= bw // 2 and bh // 8 <= h <= bh // 2:
        return "mid"
    return "other"


def family(bw, bh, channels, seed):
    """len(AMPS)^2 opaque tiles: base + ax * profile(x) + ay * profile(y), each colour channel with profiles and a base of its own"""
    x, y = np.arange(bw, dtype=np.uint64), np.arange(bh, dtype=np.uint64)
    fx = np.stack([((vp.hash32(x, seed + 11 * c + 1) >> 9) & 1) for c in range(3)], axis=1).astype(np.int32)  # [bw, 3]
    fy = np.stack([((vp.hash32(y, seed + 11 * c + 2) >> 9) & 1) for c in range(3)], axis=1).astype(np.int32)  # [bh, 3]
    base = np.array([40, 61, 87], np.int32) + (seed % 23)
    tiles = []
    for ax in AMPS:
        for ay in AMPS:
            t = np.empty((bh, bw, channels), np.uint8)
            t[..., :3] = np.clip(base[None, None, :] + ax * fx[None, :, :] + ay * fy[:, None, :], 0, 255)
            if channels == 4:
                t[..., 3] = 255
            tiles.append(t)
    return tiles


def strip(tiles):
    """the tiles side by side in one row"""
    return np.concatenate(tiles, axis=1)


_pools = {}


def pool(oracle, bw, bh, channels, mode, factor):
    """{kind: [tile]} over three families, classified by the oracle (once per geometry)"""
    key = (bw, bh, channels, mode, factor)
    if key not in _pools:
        tiles = [t for seed in (7, 1013, 40009) for t in family(bw, bh, channels, seed)]
        _, w, h, _ = oracle.shrink_image(strip(tiles), bw, bh, mode, LANCZOS3, factor, want_pixels=False)
        out = {}
        for t, tw, th in zip(tiles, w.tolist(), h.tolist()):
            t.setflags(write=False)
            out.setdefault(kind_of(tw, th, bw, bh), []).append(t)
        _pools[key] = out
    return _pools[key]


def draws(n, seed, k):
    """n draws in 0..k-1"""
    return ((vp.hash32(np.arange(n, dtype=np.uint64), seed) >> 8) % k).astype(np.int64)


def with_alpha_254(tile, seed):
    """the tile with alpha 254 in ONE pixel"""
    t = tile.copy()
    bh, bw = t.shape[:2]
    i = int(vp.hash32(np.array([5], np.uint64), seed)[0] % (bw * bh))
    t[i // bw, i % bw, 3] = 254
    return t


def paste(img, r, c, bw, bh, tile):
    part = img[r * bh:(r + 1) * bh, c * bw:(c + 1) * bw]
    part[...] = tile[: part.shape[0], : part.shape[1]]


def kinds_of_frame(img, bw, bh, ow, oh):
    """the kind of every tile of img, from the frame and the oracle's stored sizes alone: ragged (not bw x bh), alpha 254 (a full
    RGBA tile with a pixel that is not opaque), else kind_of"""
    H, W, C = img.shape
    cols, rows = -(-W // bw), -(-H // bh)
    out = []
    for r in range(rows):
        for c in range(cols):
            part = img[r * bh:(r + 1) * bh, c * bw:(c + 1) * bw]
            t = r * cols + c
            if part.shape[:2] != (bh, bw):
                out.append(RAGGED)
            elif C == 4 and (part[..., 3] != 255).any():
                out.append(ALPHA)
            else:
                out.append(kind_of(int(ow[t]), int(oh[t]), bw, bh))
    return out


# ---- a. pairs ---------------------------------------------------------------------------------------------------------------------

STRIDES = tuple(range(1, 9))
PAIR_COLS, PAIR_ROWS = 9, 54   # 8 full tiles and a ragged one (7 px wide) per tile row: 486 tiles
# the seed of each (block, channels) frame: the first one at which missing_pairs() is empty (find_pair_seed, on the CPU)
PAIR_SEEDS = {(16, 4): 2, (16, 3): 0, (32, 4): 2, (32, 3): 0, (64, 4): 2, (64, 3): 0}


def pair_kinds(channels):
    return OPAQUE_KINDS + ((ALPHA,) if channels == 4 else ())


def planned_pair_kinds(channels, seed):
    """the kind of every tile in flat order: a draw per full tile, RAGGED in the last column"""
    free = pair_kinds(channels)
    d = draws(PAIR_COLS * PAIR_ROWS, seed, len(free))
    return [RAGGED if t % PAIR_COLS == PAIR_COLS - 1 else free[d[t]] for t in range(PAIR_COLS * PAIR_ROWS)]


def missing_pairs(kinds, channels):
    """[(stride, kind at i, kind at i + stride)] that do NOT occur.  Wanted, for every stride in 1..8: every ordered pair of the
    kinds a full tile can be given, and every such kind before and after a ragged tile.  A ragged tile ends a tile row, so two of
    them are a multiple of the row length (9) apart: (ragged, ragged) cannot occur at these strides and is not wanted."""
    free = pair_kinds(channels)
    missing = []
    for g in STRIDES:
        seen = set(zip(kinds[:-g], kinds[g:]))
        want = [(a, b) for a in free for b in free] + [(a, RAGGED) for a in free] + [(RAGGED, b) for b in free]
        missing += [(g, a, b) for a, b in want if (a, b) not in seen]
    return missing


def find_pair_seed(channels, limit=20000):
    for seed in range(limit):
        if not missing_pairs(planned_pair_kinds(channels, seed), channels):
            return seed
    raise AssertionError("no seed")


def pair_frame(oracle, block, channels):
    """(image, planned kinds).  The ragged tiles carry the first 7 columns of a tile of a drawn kind."""
    seed = PAIR_SEEDS[(block, channels)]
    kinds = planned_pair_kinds(channels, seed)
    p = pool(oracle, block, block, channels, DIRECTIONAL, FACTOR)
    free = pair_kinds(channels)
    img = np.zeros((PAIR_ROWS * block, (PAIR_COLS - 1) * block + 7, channels), np.uint8)
    pick = draws(len(kinds), seed + 77, 1 << 20)
    under = draws(len(kinds), seed + 78, 5)
    for t, kind in enumerate(kinds):
        if kind == RAGGED:
            kind = free[pick[t] % len(OPAQUE_KINDS)]
        if kind == ALPHA:  # alpha is not looked at by the directional detector: any opaque tile under the pixel
            base = p[("whole", "width kept", "height kept", "mid", "narrow")[under[t]]]
            tile = with_alpha_254(base[pick[t] % len(base)], seed + t)
        else:
            tile = p[kind][pick[t] % len(p[kind])]
        paste(img, t // PAIR_COLS, t % PAIR_COLS, block, block, tile)
    img.setflags(write=False)
    return img, kinds


# ---- b. shrink_by triples ---------------------------------------------------------------------------------------------------------

TRIPLE_COLS, TRIPLE_ROWS = 12, 16   # full tiles only: 192 of them
TRIPLE_SEEDS = {(16, 4): 0, (16, 3): 0, (32, 4): 0, (32, 3): 0, (64, 4): 0, (64, 3): 0}


def planned_triple_kinds(seed):
    return [("whole", "reduced")[k] for k in draws(TRIPLE_COLS * TRIPLE_ROWS, seed + 500, 2)]


def missing_triples(kinds):
    """[(stride, kind at i, at i + stride, at i + 2 stride)] over {whole, reduced} that do not occur, strides 1..8"""
    missing = []
    for g in STRIDES:
        seen = set(zip(kinds[:-2 * g], kinds[g:-g], kinds[2 * g:]))
        missing += [(g, a, b, c) for a in ("whole", "reduced") for b in ("whole", "reduced") for c in ("whole", "reduced") if (a, b, c) not in seen]
    return missing


def find_triple_seed(limit=20000):
    for seed in range(limit):
        if not missing_triples(planned_triple_kinds(seed)):
            return seed
    raise AssertionError("no seed")


def by_pools(oracle, bw, bh, channels):
    """(tiles the oracle stores whole in shrink_by at BY_FACTOR, tiles it reduces) -- plus, among the first, one of pure noise"""
    p = pool(oracle, bw, bh, channels, SHRINK_BY, BY_FACTOR)
    whole = list(p.get("whole", []))
    noise = np.empty((bh, bw, channels), np.uint8)
    noise[..., :3] = vp.noise(bw, bh, 0xB0 + bw)
    if channels == 4:
        noise[..., 3] = 255
    whole.insert(0, noise)
    reduced = [t for k, ts in sorted(p.items()) if k != "whole" for t in ts]
    return whole, reduced


def whole_or_reduced(ow, oh, bw, bh):
    return ["whole" if (int(w), int(h)) == (bw, bh) else "reduced" for w, h in zip(ow, oh)]


def sequence_frame(oracle, bw, bh, channels, kinds, cols, seed):
    """full tiles of the two shrink_by kinds in the given order, `cols` per tile row"""
    whole, reduced = by_pools(oracle, bw, bh, channels)
    rows = -(-len(kinds) // cols)
    assert rows * cols == len(kinds)
    img = np.zeros((rows * bh, cols * bw, channels), np.uint8)
    pick = draws(len(kinds), seed + 79, 1 << 20)
    for t, kind in enumerate(kinds):
        src = whole if kind == "whole" else reduced
        paste(img, t // cols, t % cols, bw, bh, src[pick[t] % len(src)])
    img.setflags(write=False)
    return img


def triple_frame(oracle, block, channels):
    seed = TRIPLE_SEEDS[(block, channels)]
    kinds = planned_triple_kinds(seed)
    return sequence_frame(oracle, block, block, channels, kinds, TRIPLE_COLS, seed), kinds


# ---- c. list batches --------------------------------------------------------------------------------------------------------------

LIST_COUNTS = (15, 16, 17, 31, 32, 33)   # either side of one and two batches of kListBatch = 16 entries
LIST_SIDE = 8                            # 8 x 8 full tiles
# what the rest of such a frame is made of: opaque, and none of them handed on by shrink32_kernel
LIST_FILLERS = ("whole", "one", "width kept", "height kept", "mid", "narrow")


# shrink64_kernel keeps its list batches per BLOCK, and a one-CU launch of it (launch_fast64: 160 KB of LDS / lds64_dwords(3)) has
# four blocks, of which block c walks tiles c, c + 4, c + 8, ... in that order: the listed tiles of a tall frame all sit on ONE
# residue class, so that one block lists exactly n of them.  18 rows of 8 tiles: 36 tiles per class.
LIST_TALL_ROWS, LIST_CLASS = 18, 4


def list_frame(oracle, block, n_alpha, n_sliver, seed=0, rows=LIST_SIDE, on_class=None):
    """rows x 8 full RGBA tiles (8 x 8 by default): n_alpha of them with ONE pixel of alpha 254, n_sliver of the (block / 2) x (2|1)
    class -- for 32x32 tiles the class shrink32_kernel hands on to the worklist kernel -- the rest opaque tiles of the other kinds.
    on_class = (r, m): the tiles with the pixel and the slivers are drawn among the tiles t with t % m == r alone.
    -> (image, bool[n] has the pixel, bool[n] planned sliver)"""
    n = rows * LIST_SIDE
    where = np.arange(n) if on_class is None else np.arange(on_class[0], n, on_class[1])
    assert n_alpha + n_sliver <= len(where)
    p = pool(oracle, block, block, 4, DIRECTIONAL, FACTOR)
    order = where[np.argsort(vp.hash32(where.astype(np.uint64), 0xC0FFEE + seed + 64 * n_alpha + n_sliver), kind="stable")]
    alpha, sliver = np.zeros(n, bool), np.zeros(n, bool)
    alpha[order[:n_alpha]] = True
    sliver[order[n_alpha:n_alpha + n_sliver]] = True
    pick = draws(n, seed + 80, 1 << 20)
    img = np.zeros((rows * block, LIST_SIDE * block, 4), np.uint8)
    for t in range(n):
        kind = "sliver" if sliver[t] else LIST_FILLERS[pick[t] % len(LIST_FILLERS)]
        tile = p[kind][(pick[t] >> 4) % len(p[kind])]
        if alpha[t]:
            tile = with_alpha_254(tile, seed + t)
        paste(img, t // LIST_SIDE, t % LIST_SIDE, block, block, tile)
    img.setflags(write=False)
    return img, alpha, sliver


def tall_list_frame(oracle, n_alpha):
    """64x64 tiles, 18 rows of 8: n_alpha tiles with the pixel, every one of them on residue class 0 of LIST_CLASS"""
    return list_frame(oracle, 64, n_alpha, 0, seed=3, rows=LIST_TALL_ROWS, on_class=(0, LIST_CLASS))


# ---- d. detector batch seams ------------------------------------------------------------------------------------------------------

# tiles per batch of the detector kernels (pxz_oklab.hip): kOkTiles = 15 (oklab_kernel: run-time geometry, PXZ_OKLAB_V1),
# Ok2Geom<16|32>::kTiles = kOk2Prod = 14, Ok2Geom<64>::kTiles = 3
DETECTOR_BATCHES = (15, 14, 3)
# every count k b and k b + 1 for k = 1, 2, 3 batches of each size b, and 1, 2, 13, 29, 44: fewer tiles than a batch, odd ones between
SEAM_COUNTS = (1, 2, 3, 4, 6, 7, 9, 10, 13, 14, 15, 16, 28, 29, 30, 31, 42, 43, 44, 45, 46)
SEAM_GEOMS = ((16, 16), (32, 32), (64, 64), (24, 24))


def seam_frame(oracle, bw, bh, channels, n):
    """one row of n full tiles, whole and reduced ones in a drawn order"""
    kinds = [("whole", "reduced")[k] for k in draws(n, 900 + n, 2)]
    return sequence_frame(oracle, bw, bh, channels, kinds, n, 900 + n), kinds


# ---- e. detector alpha sequences --------------------------------------------------------------------------------------------------

# The pipelined Oklab detectors carry a tile's alpha from period to period per PRODUCER WAVE (pxz_oklab.hip: al_cur / al_old and
# the three opaque flags of oklab2_kernel, alpha_px[] or the parked alpha word of oklab_kernel), and a one-block launch hands a
# wave the items w, w + b, w + 2b, ... with b tiles per batch.  A kind is an alpha plane laid over an opaque base tile; the
# alpha plane is summed on its own, so what a tile's value tells is the MULTISET of alphas the tile was credited with -- every
# tile therefore has a signature (pixel count, alpha value) of its own.
ALPHA_KINDS = ("opaque", "full", "top", "bottom", "middle", "one 254")
ALPHA_DRAWN = ("opaque",) + ALPHA_KINDS           # opaque twice in seven: (opaque, opaque, opaque) is a wanted triple
ALPHA_PIXELS = {"top": 3, "bottom": 2, "middle": 5, "one 254": 1}   # pixels that are not opaque (full: all of them)
ALPHA_BASE = {"top": 0, "bottom": 80, "middle": 160}               # their alpha is (base + 7 item) % 240: never that of item - 3, 14, 15
ALPHA_STRIDES = (3, 14, 15)                       # = sorted DETECTOR_BATCHES
ALPHA_COLS, ALPHA_ROWS = 14, 15                   # 210 full tiles, a multiple of 3, 14 and 15
ALPHA_SHORT_ROW = 8                               # 32x32, 64x64: a last tile row the square detectors still take (whole bands)
ALPHA_RAGGED = {(24, 24): (6, 10), (40, 32): (6, 12)}   # run-time geometry: (width of the right column, height of the bottom row)
ALPHA_GEOMS = ((16, 16), (32, 32), (64, 64), (24, 24), (40, 32))
# the first seed at which missing_alpha_pairs() is empty (find_alpha_seed, on the CPU).  Square frames: every stride; the run-time
# geometry is oklab_kernel's alone (15 tiles per batch), and its 14th grid column is the ragged one
ALPHA_SEEDS = {(16, 16): 7, (32, 32): 7, (64, 64): 7, (24, 24): 6, (40, 32): 6}


def planned_alpha_kinds(seed, n):
    return [ALPHA_DRAWN[k] for k in draws(n, seed + 700, len(ALPHA_DRAWN))]


def missing_alpha_pairs(kinds, strides=ALPHA_STRIDES, sequenced=None):
    """[(stride, kind at i, kind at i + stride)] and [(stride, o at i, o at i + stride, o at i + 2 stride)], o = "opaque" | "not
    opaque", that do NOT occur among the items flagged in `sequenced` (all of them when None).  Wanted at every stride: all 36
    ordered pairs of kinds, and all eight triples over {opaque, not opaque} -- the state lives across three periods (conversion,
    re-delivery, the band that awaits its store)."""
    n = len(kinds)
    ok = [True] * n if sequenced is None else list(sequenced)
    o = ["opaque" if k == "opaque" else "not opaque" for k in kinds]
    missing = []
    for g in strides:
        seen = {(kinds[i], kinds[i + g]) for i in range(n - g) if ok[i] and ok[i + g]}
        missing += [(g, a, b) for a in ALPHA_KINDS for b in ALPHA_KINDS if (a, b) not in seen]
        seen3 = {(o[i], o[i + g], o[i + 2 * g]) for i in range(n - 2 * g) if ok[i] and ok[i + g] and ok[i + 2 * g]}
        both = ("opaque", "not opaque")
        missing += [(g, a, b, c) for a in both for b in both for c in both if (a, b, c) not in seen3]
    return missing


def alpha_layout(bw, bh, edge_w=0, edge_h=0):
    """(grid columns, grid rows, per item: is it one of the SEQUENCED tiles -- those the detector's main launch takes, whose item
    number is the flat tile index).  Without a ragged column 14 x 15 full tiles; with one, 13 full columns and the ragged one.
    A short last row without a ragged column (the square variants) stands behind one more full row, see alpha_sequence_frame."""
    cols = ALPHA_COLS
    full_cols = cols if edge_w == 0 else cols - 1
    full_rows = ALPHA_ROWS + (1 if edge_h and not edge_w else 0)
    rows = full_rows + (1 if edge_h else 0)
    # the square detectors take a last row of whole bands (8 rows: two bands of 32x32, one super-band of 64x64)
    taken_rows = rows if edge_h and not edge_w and bw == bh and bw in (32, 64) and edge_h % 8 == 0 else full_rows
    return cols, rows, [c < full_cols and r < taken_rows for r in range(rows) for c in range(cols)]


def find_alpha_seed(ragged=False, limit=20000):
    cols, rows, seq = alpha_layout(24, 24, *ALPHA_RAGGED[(24, 24)]) if ragged else alpha_layout(32, 32)
    for seed in range(limit):
        if not missing_alpha_pairs(planned_alpha_kinds(seed, cols * rows), (15,) if ragged else ALPHA_STRIDES, seq):
            return seed
    raise AssertionError("no seed")


def alpha_plane(kind, t, w, h):
    """the alpha bytes [h, w] of item t's kind.  top / bottom / middle: ALPHA_PIXELS[kind] pixels of ONE row, in drawn columns, all
    of one alpha that no neighbour at the detectors' strides shares.  middle: a row r with r % 8 // 2 in (1, 2) -- for 64x64 tiles
    rows 0, r and h - 1 then belong to three different producer waves of oklab2_kernel<64> (wave j: rows 8k + 2j, 8k + 2j + 1).
    one 254: the SAME pixel in every tile of a shape, so two of them in a row carry equal planes."""
    assert h >= 8 and w >= 4
    a = np.full((h, w), 255, np.uint8)
    if kind == "opaque":
        return a
    if kind == "full":
        i = np.arange(h * w, dtype=np.uint64).reshape(h, w)
        return (vp.hash32(i, 0xA1FA + 977 * t) % 255).astype(np.uint8)
    if kind == "one 254":
        i = int(vp.hash32(np.array([w], np.uint64), 0x254 + h)[0] % (w * h))
        a[i // w, i % w] = 254
        return a
    if kind == "middle":
        d = int(vp.hash32(np.array([t], np.uint64), 0x3D)[0])
        row = 8 * (d % (h // 8)) + 2 + (d >> 8) % 4
    else:
        row = 0 if kind == "top" else h - 1
    cols = np.argsort(vp.hash32(np.arange(w, dtype=np.uint64), 0xC015 + 131 * t), kind="stable")[:ALPHA_PIXELS[kind]]
    a[row, cols] = (ALPHA_BASE[kind] + 7 * t) % 240
    return a


def alpha_sequence_frame(oracle, bw, bh, edge_w=0, edge_h=0):
    """(image, planned kind of every grid tile in flat order).  RGBA; the bases are opaque tiles of by_pools(), drawn from the tiles
    the oracle stores whole and from those it reduces alike, so transparent tiles are both copied ahead and resampled.
    edge_w, edge_h = 0: 14 x 15 full tiles, the flat index is the detector's item number.
    edge_h alone (square tiles): the same 210 tiles, then a row of `full` tiles, then a row edge_h px high of drawn kinds -- with
    14 tiles per batch a short tile follows a tile that is transparent in every band in every wave.
    edge_w and edge_h (run-time geometry): 13 full columns and one edge_w px wide, 15 full rows and one edge_h px high; the ragged
    tiles are cut from the top left of full ones and get the alpha plane of their kind at their own size."""
    cols, rows, _ = alpha_layout(bw, bh, edge_w, edge_h)
    seed = ALPHA_SEEDS[(bw, bh)]
    kinds = planned_alpha_kinds(seed, cols * rows)
    if edge_h and not edge_w:
        kinds[ALPHA_ROWS * cols:(ALPHA_ROWS + 1) * cols] = ["full"] * cols
    whole, reduced = by_pools(oracle, bw, bh, 4)
    pick = draws(cols * rows, seed + 81, 1 << 20)
    W = cols * bw if edge_w == 0 else (cols - 1) * bw + edge_w
    H = rows * bh if edge_h == 0 else (rows - 1) * bh + edge_h
    img = np.zeros((H, W, 4), np.uint8)
    for t, kind in enumerate(kinds):
        src = whole if pick[t] & 1 else reduced
        r, c = t // cols, t % cols
        paste(img, r, c, bw, bh, src[(pick[t] >> 1) % len(src)])
        part = img[r * bh:(r + 1) * bh, c * bw:(c + 1) * bw]
        part[..., 3] = alpha_plane(kind, t, part.shape[1], part.shape[0])
    img.setflags(write=False)
    return img, kinds
