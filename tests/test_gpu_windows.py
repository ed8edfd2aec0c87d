"""Pixel windows of .pixlzr files (pxz_decode_windows_device, pxz_expand_windows_device, pxz_decode_windows_files).  The files are
built on the CPU: stored sizes dealt by hand as in tests/test_gpu_distortion.py (full size, lower, narrower, both smaller and
not a power of two, 1x1), random stored bytes, written by the oracle's writer.  The expected pixels of a window are
oracle.decode_container + oracle.expand_image of its file, cropped with numpy; each case is also held against the library's
own full varied decode + expand, cropped.  Every comparison is exact.  The outputs are pre-filled, and every byte that belongs
to no window -- row padding, the gaps between windows, the guard bytes around them -- must still hold the pattern afterwards:
that is the check that a clipped store does not spill."""
import ctypes as C
import os

import numpy as np
import pytest
from PIL import Image

from test_gpu_distortion import BOTH, FULL, LOWER, NARROWER, ONE, class_of, random_slots, shape_of, tile_rects
from test_gpu_varied_decode import decode_varied, expand_varied, image_of, poisoned, upload_files

pytestmark = pytest.mark.gpu

POISON = 0xA5
FILTERS = (0, 1, 2, 3, 4)
INVALID_ARG, UNSUPPORTED = -1, -5
GUARD = 64
# block_w, block_h, image width, image height: each a few tiles, with ragged edges
GEOMS = [(32, 32, 100, 70), (64, 64, 130, 65), (16, 16, 50, 33), (48, 20, 100, 37)]
KINDS = ("alpha", "rgb")  # RGBA with any alpha, RGB


@pytest.fixture(scope="module")
def gpu(product):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    h = product.Handle(0)
    yield h
    h.close()


# ---- files, windows and what to expect ---------------------------------------------------------------------------------

def deal_sizes(rects):
    """the five shapes dealt in turn over a file's tiles, largest tiles first and "both smaller" before the others, so that even a
    file of six tiles has a tile of the full block size that is stored smaller on both axes"""
    order = sorted(range(len(rects)), key=lambda t: (-rects[t][2] * rects[t][3], t))
    tw, th = np.zeros(len(rects), np.uint32), np.zeros(len(rects), np.uint32)
    for rank, t in enumerate(order):
        tw[t], th[t] = shape_of(rects[t][2], rects[t][3], (BOTH, FULL, LOWER, NARROWER, ONE)[rank % 5], third=(rank // 5) % 2 == 1)
    return tw, th


class File:
    """one .pixlzr file with hand-dealt stored sizes and random stored bytes; what it expands to per filter, computed once"""

    def __init__(self, oracle, bw, bh, w, h, kind, seed=0, tw=None, th=None):
        self.bw, self.bh, self.w, self.h, self.kind = bw, bh, w, h, kind
        self.c = 3 if kind == "rgb" else 4
        self.cols, self.rows = -(-w // bw), -(-h // bh)
        rng = np.random.default_rng(1000 * seed + bw * 7 + bh * 3 + w + h + self.c)
        self.rects = tile_rects(w, h, bw, bh)
        if tw is None:
            tw, th = deal_sizes(self.rects)
        self.tw, self.th = tw, th
        self.slots = random_slots(rng, tw, th, bw * bh, self.c, kind)
        self.values = rng.integers(0, 1 << 32, len(self.rects), dtype=np.uint64).astype(np.uint32).view(np.float32)
        self.raw = oracle.encode_container(w, h, bw, bh, self.c, 0, self.values, None, tw, th, self.slots)
        self.oracle, self._image = oracle, {}

    def classes(self):
        return [class_of(r[2], r[3], int(a), int(b)) for r, a, b in zip(self.rects, self.tw, self.th)]

    def image(self, filt):
        if filt not in self._image:
            d = self.oracle.decode_container(self.raw)
            assert (d["tw"] == self.tw).all() and (d["th"] == self.th).all()
            self._image[filt] = self.oracle.expand_image(self.w, self.h, self.bw, self.bh, self.c, filt, d["tw"], d["th"], d["slots"])
        return self._image[filt]


_files = {}


def file_of(oracle, geom, kind):
    if (geom, kind) not in _files:
        _files[(geom, kind)] = File(oracle, *geom, kind)
    return _files[(geom, kind)]


def covered_grid(f, rect):
    x, y, w, h = rect
    c0, r0 = x // f.bw, y // f.bh
    return c0, r0, (x + w - 1) // f.bw - c0 + 1, (y + h - 1) // f.bh - r0 + 1


def covered_tiles(f, rect):
    """the image's tile numbers a rectangle covers, in the window layout's order"""
    c0, r0, cc, cr = covered_grid(f, rect)
    return [(r0 + j) * f.cols + c0 + i for j in range(cr) for i in range(cc)]


def cut_on_four_sides(f, rect, t):
    x, y, w, h = rect
    tx, ty, fw, fh = f.rects[t]
    return tx < x and ty < y and x + w < tx + fw and y + h < ty + fh


def rects_of(f):
    """the rectangles every geometry is read through"""
    bw, bh, w, h = f.bw, f.bh, f.w, f.h
    ex, ey = (f.cols - 1) * bw, (f.rows - 1) * bh  # the edge tile's first pixel
    # a tile of the full block size stored smaller on both axes, for the window that cuts it on all four sides
    inner = next(t for t, (r, k) in enumerate(zip(f.rects, f.classes())) if k == BOTH and (r[2], r[3]) == (bw, bh))
    ix, iy = f.rects[inner][:2]
    sy = bh - 5  # (odd: every block height here is even)
    rects = [
        (0, 0, w, h),                                   # the whole image
        (0, 0, 1, 1), (w - 1, 0, 1, 1), (0, h - 1, 1, 1), (w - 1, h - 1, 1, 1),  # 1x1 at each corner
        (ex, ey, 1, 1),                                 # 1x1 in the edge tile
        (ix + 1, iy + 2, bw - 3, bh - 5),               # strictly inside one tile
        (bw - 3, sy, 9, min(11, h - sy)),               # straddles a four-tile corner at odd x and y
        (0, min(bh + 1, h - 1), w, 1),                  # full width, one pixel high
        (bw + 1, 0, 1, h),                              # full height, one pixel wide
        (w - 7, h - 5, 7, 5),                           # ends on the image's last pixel
        (bw // 2, 1, bw, min(bh, h - 1)), (bw // 2 + 5, 3, bw + 2, min(bh, h - 3)),  # two that overlap
    ]
    assert (bw - 3) % 2 == 1 and sy % 2 == 1 and len(set(covered_tiles(f, rects[7]))) == 4
    assert cut_on_four_sides(f, rects[6], inner)
    return rects


def place(rects_with_image, c, flip=0):
    """windows with outputs of their own in one buffer, GUARD bytes before, between and behind them.  RGBA: every other window
    (flip picks which) on dwords with a pitch of a multiple of 4, the others at an odd address with an odd pitch; RGB: all at
    odd offsets with pitches that are no multiple of 4.  -> (windows, bytes)"""
    windows, at = [], GUARD
    for k, (i, x, y, w, h) in enumerate(rects_with_image):
        if c == 4 and (k + flip) % 2 == 0:
            at = (at + 3) & ~3
            pitch = w * 4 + 8
        else:
            at |= 1
            pitch = w * c + 5
            while pitch % 4 == 0:
                pitch += 1
        windows.append((i, x, y, w, h, pitch, at))
        at += pitch * h + GUARD
    return windows, at


def window_view(buf, win, c):
    _, _, _, w, h, pitch, off = win
    return np.lib.stride_tricks.as_strided(buf[off:], (h, w, c), (pitch, c, 1))


def outside_mask(total, windows, c):
    m = np.ones(total, bool)
    for (_, _, _, w, h, pitch, off) in windows:
        for y in range(h):
            m[off + y * pitch: off + y * pitch + w * c] = False
    return m


def decode_windows(gpu, product, files, windows, lead=3):
    """-> (tile offsets, (values, w, h, slots) host arrays, window flags, status, the device tensors)"""
    import torch
    f0 = files[0]
    sizes = [(f.w, f.h) for f in files]
    buf, offs = upload_files([f.raw for f in files], lead)
    to = product.window_layout(sizes, windows, f0.bw, f0.bh)
    out, flags = poisoned(int(to[-1]), f0.bw * f0.bh * f0.c, len(windows))
    gpu.decode_windows_device(buf, offs, sizes, windows, f0.c, f0.bw, f0.bh, out=out, window_flags=flags)
    status = gpu.decode_status()
    torch.cuda.synchronize()
    vals, ow, oh, slots = out
    host = (vals.cpu().numpy(), ow.cpu().numpy().astype(np.uint32), oh.cpu().numpy().astype(np.uint32), slots.cpu().numpy())
    return to, host, flags.cpu().numpy(), status, out


def expand_windows(gpu, files, windows, total, filt, dev_tiles):
    """-> (the pre-filled buffer after the call as a host array, window flags, status)"""
    import torch
    f0 = files[0]
    out = torch.full((total,), POISON, dtype=torch.uint8, device="cuda")
    flags = torch.full((len(windows),), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    _, ow, oh, slots = dev_tiles
    gpu.expand_windows_device([(f.w, f.h) for f in files], windows, f0.c, f0.bw, f0.bh, filt, ow, oh, slots, out, window_flags=flags)
    status = gpu.decode_status()
    torch.cuda.synchronize()
    return out.cpu().numpy(), flags.cpu().numpy(), status


def full_decode(gpu, product, files):
    """the library's own whole-image reader over the same files"""
    f0 = files[0]
    return decode_varied(gpu, product, [f.raw for f in files], [(f.w, f.h) for f in files], f0.c, f0.bw, f0.bh)


def full_images(gpu, files, filt, dev_tiles):
    """... and its whole-image expand: one tightly packed image per file"""
    f0 = files[0]
    descs, at = [], 0
    for f in files:
        descs.append((f.w, f.h, f.w * f.c, at))
        at += f.w * f.h * f.c
    buf, flags, status = expand_varied(gpu, descs, at, f0.c, f0.bw, f0.bh, filt, dev_tiles)
    assert status == 0
    return [image_of(buf, d, f0.c) for d in descs]


def assert_covered_tiles_equal(files, windows, to, got, full_to, full, what):
    """value bits, sizes and the valid slot bytes of every covered tile against the whole-image reader's for that tile"""
    for k, win in enumerate(windows):
        f = files[win[0]]
        for j, t in enumerate(covered_tiles(f, win[1:5])):
            a, b = int(to[k]) + j, int(full_to[win[0]]) + t
            assert got[1][a] == full[1][b] and got[2][a] == full[2][b], f"{what}: window {k} tile {j}: {got[1][a]}x{got[2][a]}, whole image {full[1][b]}x{full[2][b]}"
            assert got[0].view(np.uint32)[a] == full[0].view(np.uint32)[b], f"{what}: window {k} tile {j}: value bits"
            n = int(full[1][b]) * int(full[2][b]) * f.c
            assert (got[3][a, :n] == full[3][b, :n]).all(), f"{what}: window {k} tile {j}: slot bytes"
        assert int(to[k + 1]) - int(to[k]) == len(covered_tiles(f, win[1:5]))


def check_windows(buf, files, windows, filt, product_images, what):
    c = files[0].c
    for k, win in enumerate(windows):
        i, x, y, w, h = win[:5]
        got = window_view(buf, win, c)
        exp = files[i].image(filt)[y:y + h, x:x + w]
        bad = (got != exp).any(axis=2)
        assert not bad.any(), f"{what} window {k} {win}: {int(bad.sum())} of {w * h} pixels differ from the oracle's crop"
        if product_images is not None:
            assert (got == product_images[i][y:y + h, x:x + w]).all(), f"{what} window {k} {win}: differs from the whole-image expand, cropped"
    assert (buf[outside_mask(buf.size, windows, c)] == POISON).all(), f"{what}: bytes outside the windows were written"


# ---- every geometry, kind and filter through the same set of windows ------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: f"{g[0]}x{g[1]}-{g[2]}x{g[3]}")
def test_windows_equal_the_oracle_crops(gpu, product, oracle, geom, kind):
    f = file_of(oracle, geom, kind)
    rects = rects_of(f)
    # conditions on the inputs, checked before the GPU is used
    classes = f.classes()
    covered = set(t for r in rects for t in covered_tiles(f, r))
    met = {classes[t] for t in covered}
    assert FULL in met and BOTH in met and (LOWER in met or BOTH in met) and (NARROWER in met or BOTH in met), sorted(met)
    assert any(classes[t] == BOTH and cut_on_four_sides(f, rects[6], t) for t in covered_tiles(f, rects[6]))
    assert {FULL, LOWER, NARROWER, BOTH, ONE} <= set(classes)

    full_to, full, full_flags, full_status, full_dev = full_decode(gpu, product, [f])
    assert full_status == 0
    for flip in (0, 1):
        windows, total = place([(0,) + r for r in rects], f.c, flip)
        if f.c == 3:
            assert all(w[6] % 2 == 1 and w[5] % 4 != 0 for w in windows)
        else:
            assert any(w[6] % 4 == 0 and w[5] % 4 == 0 for w in windows) and any(w[6] % 2 == 1 for w in windows)
        to, got, flags, status, dev = decode_windows(gpu, product, [f], windows)
        assert status == 0 and (flags == 0).all(), f"decode: status {status}, flags {flags}"
        assert_covered_tiles_equal([f], windows, to, got, full_to, full, f"{geom} {kind}")
        for filt in FILTERS:
            buf, flags, status = expand_windows(gpu, [f], windows, total, filt, dev)
            assert status == 0 and (flags == 0).all(), f"filter {filt}: status {status}, flags {flags}"
            mine = full_images(gpu, [f], filt, full_dev) if flip == 0 else None
            check_windows(buf, [f], windows, filt, mine, f"{geom} {kind} filter {filt} layout {flip}")


@pytest.mark.parametrize("kind", KINDS)
def test_windows_of_three_differently_sized_files_in_one_call(gpu, product, oracle, kind):
    bw = bh = 32
    files = [File(oracle, bw, bh, w, h, kind, seed=5) for (w, h) in ((1, 1), (45, 40), (97, 61))]
    rects = [(2, 30, 29, 40, 9), (0, 0, 0, 1, 1), (1, 0, 0, 45, 40), (2, 95, 1, 2, 60), (1, 31, 31, 3, 3), (2, 0, 0, 97, 61), (1, 44, 39, 1, 1),
             (2, 63, 31, 2, 2)]
    full_to, full, _, full_status, full_dev = full_decode(gpu, product, files)
    assert full_status == 0
    windows, total = place(rects, files[0].c, 1)
    to, got, flags, status, dev = decode_windows(gpu, product, files, windows)
    assert status == 0 and (flags == 0).all()
    assert_covered_tiles_equal(files, windows, to, got, full_to, full, kind)
    for filt in (0, 2, 4):
        buf, flags, status = expand_windows(gpu, files, windows, total, filt, dev)
        assert status == 0 and (flags == 0).all()
        check_windows(buf, files, windows, filt, full_images(gpu, files, filt, full_dev), f"three files {kind} filter {filt}")


# ---- more windows than a block keeps first tiles of in LDS ------------------------------------------------------------------

MANY = 2049  # one more than kVxImages (pxz_device.h): the owner search reads the table itself


def many_windows(rng, files, c):
    """MANY windows of 1 .. 11 px on a side over the files in turn, each starting inside a tile on both axes, its output at an odd
    byte offset with a pitch one byte above its row -> (windows, bytes)"""
    windows, at = [], 7
    for k in range(MANY):
        f = files[k % len(files)]
        x, y = int(rng.integers(1, f.w)), int(rng.integers(1, f.h))
        x, y = x - (x % f.bw == 0), y - (y % f.bh == 0)
        w, h = int(rng.integers(1, min(11, f.w - x) + 1)), int(rng.integers(1, min(11, f.h - y) + 1))
        at |= 1
        windows.append((k % len(files), x, y, w, h, w * c + 1, at))
        at += (w * c + 1) * h + 3
    return windows, at + 7


@pytest.mark.parametrize("kind", KINDS)
def test_2049_windows_find_their_tiles_in_the_table_itself(gpu, product, oracle, kind):
    bw = bh = 8
    files = [File(oracle, bw, bh, w, h, kind, seed=11) for (w, h) in ((29, 23), (40, 17), (13, 35))]
    c = files[0].c
    windows, total = many_windows(np.random.default_rng(2049 + c), files, c)
    # conditions on the inputs, checked before the GPU is used
    assert len(windows) == MANY
    assert all(x % bw and y % bh and 1 <= w <= 11 and 1 <= h <= 11 and off % 2 == 1 and pitch == w * c + 1 for (_, x, y, w, h, pitch, off) in windows)
    assert {len(covered_tiles(files[i], (x, y, w, h))) for (i, x, y, w, h, _, _) in windows} >= {1, 2, 4}
    assert any(w == 11 and h == 11 for (_, _, _, w, h, _, _) in windows) and any(w == 1 for (_, _, _, w, _, _, _) in windows)
    for f in files:
        f.image(0), f.image(4)  # (the oracle reads and expands every file alone)
    full_to, full, _, full_status, _ = full_decode(gpu, product, files)
    assert full_status == 0
    to, got, flags, status, dev = decode_windows(gpu, product, files, windows)
    assert status == 0 and (flags == 0).all(), f"decode: status {status}, flags of {np.flatnonzero(flags).tolist()}"
    assert_covered_tiles_equal(files, windows, to, got, full_to, full, f"{MANY} windows {kind}")
    for filt in (0, 4):
        buf, flags, status = expand_windows(gpu, files, windows, total, filt, dev)
        assert status == 0 and (flags == 0).all(), f"filter {filt}: status {status}, flags of {np.flatnonzero(flags).tolist()}"
        check_windows(buf, files, windows, filt, None, f"{MANY} windows {kind} filter {filt}")


# ---- what is read of a file, and what that means for damage --------------------------------------------------------------

def record_at(raw, rows, ty, tx):
    """the position of record (ty, tx) of a file: from the line table and the records' own length fields"""
    lens = [int.from_bytes(raw[26 + 4 * r: 30 + 4 * r], "big") for r in range(rows)]
    pos = 26 + 4 * rows + sum(lens[:ty])
    for _ in range(tx):
        assert raw[pos:pos + 5] == b"block"
        pos += 13 + int.from_bytes(raw[pos + 9:pos + 13], "big")
    assert raw[pos:pos + 5] == b"block"
    return pos


def break_record(raw, rows, ty, tx):
    pos = record_at(raw, rows, ty, tx)
    return raw[:pos] + b"c" + raw[pos + 1:]  # "clock"


class Broken:
    def __init__(self, f, raw):
        self.__dict__.update(f.__dict__)
        self.raw = raw
        self.image = f.image


def test_damage_outside_what_a_window_reads_does_not_flag_it(gpu, product, oracle):
    f = file_of(oracle, GEOMS[0], "alpha")  # 100x70 in 32x32: a 4x3 grid
    rect = (0, 20, 10, 40, 40)              # columns 0..1, rows 0..1
    windows, total = place([rect], 4)
    for what, (ty, tx) in (("a tile row below the window", (2, 1)), ("right of the window in a covered row", (1, 3)),
                           ("right of the window in its first row", (0, 2))):
        bad = Broken(f, break_record(f.raw, f.rows, ty, tx))
        _, _, full_flags, full_status, _ = full_decode(gpu, product, [bad])
        assert full_status == 2 and full_flags.tolist() == [2], f"{what}: the whole-image reader must see it"
        to, got, flags, status, dev = decode_windows(gpu, product, [bad], windows)
        assert status == 0 and flags.tolist() == [0], f"{what}: status {status}, flags {flags}"
        buf, flags, status = expand_windows(gpu, [bad], windows, total, 2, dev)
        assert status == 0 and flags.tolist() == [0]
        check_windows(buf, [f], windows, 2, None, what)


def test_damage_left_of_a_window_flags_it_and_leaves_the_others(gpu, product, oracle):
    f = file_of(oracle, GEOMS[0], "alpha")
    good2 = File(oracle, 32, 32, 45, 40, "alpha", seed=9)
    bad = Broken(f, break_record(f.raw, f.rows, 1, 0))
    files = [bad, good2]
    rects = [(0, 10, 5, 20, 20),     # row 0 of the broken file: intact
             (0, 70, 40, 30, 30),    # columns 2..3, rows 1..2: row 1 is lost behind the broken record, row 2 is not
             (1, 3, 3, 40, 30),      # another file
             (0, 0, 64, 100, 6)]     # row 2 of the broken file
    windows, total = place(rects, 4)
    to, got, flags, status, dev = decode_windows(gpu, product, files, windows)
    assert status == 2 and gpu.decode_status() & 2
    assert flags.tolist() == [0, 2, 0, 0]
    a = int(to[1])
    assert got[1][a:a + 2].tolist() == [0, 0] and got[2][a:a + 2].tolist() == [0, 0]            # the covered tiles of row 1
    assert got[1][a + 2:a + 4].tolist() == [int(f.tw[10]), int(f.tw[11])] and (got[2][a + 2:a + 4] == f.th[10:12]).all()  # row 2
    buf, xflags, xstatus = expand_windows(gpu, files, windows, total, 4, dev)
    assert xstatus == 1 and xflags.tolist() == [0, 1, 0, 0]  # the 0x0 tiles are skipped and flagged by the expand
    for k in (0, 2, 3):
        i, x, y, w, h = windows[k][:5]
        src = f if i == 0 else good2
        assert (window_view(buf, windows[k], 4) == src.image(4)[y:y + h, x:x + w]).all(), f"window {k} beside a flagged one"
    v = window_view(buf, windows[1], 4)
    assert (v[:24] == POISON).all() and (v[24:] == f.image(4)[64:70, 70:100]).all()  # rows 40..63 are tile row 1: untouched
    assert (buf[outside_mask(buf.size, windows, 4)] == POISON).all()


def test_line_table_off_by_one_flags_every_window_of_the_file(gpu, product, oracle):
    f = file_of(oracle, GEOMS[0], "rgb")
    other = File(oracle, 32, 32, 45, 40, "rgb", seed=9)
    n = int.from_bytes(f.raw[30:34], "big") + 1
    bad = Broken(f, f.raw[:30] + n.to_bytes(4, "big") + f.raw[34:])
    windows, total = place([(0, 0, 0, 10, 10), (1, 5, 5, 30, 30), (0, 50, 40, 40, 30)], 3)
    to, got, flags, status, dev = decode_windows(gpu, product, [bad, other], windows)
    assert status == 2 and flags.tolist() == [2, 0, 2]
    for k in (0, 2):
        assert (got[1][int(to[k]):int(to[k + 1])] == 0).all() and (got[2][int(to[k]):int(to[k + 1])] == 0).all()
    buf, xflags, xstatus = expand_windows(gpu, [bad, other], windows, total, 1, dev)
    assert xflags.tolist() == [1, 0, 1]
    assert (window_view(buf, windows[1], 3) == other.image(1)[5:35, 5:35]).all()
    assert (window_view(buf, windows[0], 3) == POISON).all() and (window_view(buf, windows[2], 3) == POISON).all()


def test_invalid_stored_sizes_are_skipped_and_flagged(gpu, product, oracle):
    """a covered tile with stored size 0, or beyond its place: its pixels stay as they were, its window gets flag 1"""
    import torch
    f = file_of(oracle, GEOMS[0], "alpha")
    rects = [(0, 20, 10, 50, 40), (0, 90, 60, 10, 10), (0, 0, 0, 30, 30)]
    windows, total = place(rects, 4, 1)
    to, got, flags, status, dev = decode_windows(gpu, product, [f], windows)
    assert status == 0
    ow, oh = dev[1].clone(), dev[2].clone()
    ow[int(to[0]) + 4] = 0                   # window 0 covers columns 0..2 of rows 0..1: image tile (1, 1)
    oh[int(to[1]) + 3] = 7                   # window 1: the 4x6 corner tile, stored 7 high
    buf, xflags, xstatus = expand_windows(gpu, [f], windows, total, 3, (dev[0], ow, oh, dev[3]))
    assert xstatus == 1 and xflags.tolist() == [1, 1, 0]
    exp = f.image(3)
    v0, v1, v2 = (window_view(buf, w, 4) for w in windows)
    assert (v2 == exp[0:30, 0:30]).all()
    keep0 = np.zeros((40, 50), bool)
    keep0[22:, 12:44] = True                 # tile (1, 1) is pixels 32..63 both ways: from window (12, 22) on, 32 wide
    assert (v0[keep0] == POISON).all() and (v0[~keep0] == exp[10:50, 20:70][~keep0]).all()
    keep1 = np.zeros((10, 10), bool)
    keep1[4:, 6:] = True                     # the corner tile begins at pixel (96, 64) = window (6, 4)
    assert (v1[keep1] == POISON).all() and (v1[~keep1] == exp[60:70, 90:100][~keep1]).all()
    assert (buf[outside_mask(buf.size, windows, 4)] == POISON).all()


# ---- errors ---------------------------------------------------------------------------------------------------------------

def test_errors_name_the_window_and_write_nothing(gpu, product, oracle):
    import torch
    L = product.binding.load_library()
    P, descs_of, wins_of = product.binding.Params, product.binding.image_descs, product.binding.window_descs
    f = file_of(oracle, GEOMS[2], "alpha")   # 50x33 in 16x16
    bw, bh, c = f.bw, f.bh, f.c
    good = [(0, 3, 3, 20, 20, 80, 64), (0, 30, 10, 20, 23, 81, 4001)]
    total = 8192
    geo = [(f.w, f.h, 0, 0)]
    buf, offs = upload_files([f.raw])
    T = int(product.window_layout([(f.w, f.h)], good, bw, bh)[-1])
    ok = P(bw, bh, 0, 4, 0.0, 0)
    cases = [
        (geo, 1, [good[0], (0, 31, 10, 20, 23, 81, 4001)], 2, ok, INVALID_ARG, "window 1"),   # leaves the image on the right
        (geo, 1, [(0, 3, 14, 20, 20, 80, 64), good[1]], 2, ok, INVALID_ARG, "window 0"),      # ... below
        (geo, 1, [good[0], (1, 30, 10, 20, 23, 81, 4001)], 2, ok, INVALID_ARG, "window 1"),   # image index out of range
        (geo, 1, [good[0], (0, 30, 10, 0, 23, 81, 4001)], 2, ok, INVALID_ARG, "window 1"),    # empty
        (geo, 1, good, 0, ok, INVALID_ARG, None),                                             # no windows
        ([(f.w, 0, 0, 0)], 1, good, 2, ok, INVALID_ARG, "image 0"),                           # a descriptor pxz_varied_layout refuses
    ]

    def decode(geoms, n, wins, k, pd, out, flags):
        vals, ow, oh, slots = out
        return L.pxz_decode_windows_device(gpu._h, C.cast(descs_of(geoms), C.c_void_p), n, C.cast(wins_of(wins), C.c_void_p), k, c, C.byref(pd),
                                           C.c_void_p(buf.data_ptr()), C.c_void_p(offs.data_ptr()), C.c_void_p(vals.data_ptr()),
                                           C.c_void_p(ow.data_ptr()), C.c_void_p(oh.data_ptr()), C.c_void_p(slots.data_ptr()), C.c_void_p(flags.data_ptr()))

    def expand(geoms, n, wins, k, pd, tiles, out, flags):
        _, ow, oh, slots = tiles
        return L.pxz_expand_windows_device(gpu._h, C.cast(descs_of(geoms), C.c_void_p), n, C.cast(wins_of(wins), C.c_void_p), k, c, C.byref(pd),
                                           C.c_void_p(ow.data_ptr()), C.c_void_p(oh.data_ptr()), C.c_void_p(slots.data_ptr()), C.c_void_p(out.data_ptr()),
                                           C.c_void_p(flags.data_ptr()))

    for geoms, n, wins, k, pd, code, name in cases:
        out, flags = poisoned(T, bw * bh * c, 2)
        rc = decode(geoms, n, wins, k, pd, out, flags)
        assert rc == code, (wins, rc)
        if name:
            assert name in L.pxz_last_error(gpu._h).decode()
        torch.cuda.synchronize()
        vals, ow, oh, slots = out
        assert (vals.view(torch.int32) == 0x7F7F7F7F).all() and (ow == 0x5A5A5A5A).all() and (oh == 0x5A5A5A5A).all()
        assert (slots == POISON).all() and (flags == 0x5A5A5A5A).all()

    to, got, fl, st, tiles = decode_windows(gpu, product, [f], good)
    assert st == 0
    cases += [
        (geo, 1, [good[0], (0, 30, 10, 20, 23, 79, 4001)], 2, ok, INVALID_ARG, "window 1"),   # pitch below a row
        (geo, 1, good, 2, P(bw, bh, 0, 5, 0.0, 0), INVALID_ARG, None),                        # filter 5
        (geo, 1, good, 2, P(128, 129, 0, 4, 0.0, 0), UNSUPPORTED, None),                      # 128 * 129 * 4 > 65536 bytes
    ]
    for geoms, n, wins, k, pd, code, name in cases:
        out = torch.full((total,), POISON, dtype=torch.uint8, device="cuda")
        flags = torch.full((2,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        rc = expand(geoms, n, wins, k, pd, tiles, out, flags)
        assert rc == code, (wins, rc)
        if name:
            assert name in L.pxz_last_error(gpu._h).decode()
        torch.cuda.synchronize()
        assert (out == POISON).all() and (flags == 0x5A5A5A5A).all()
    # RGB blocks whose image a wave cannot keep in LDS: the varied expand moves them to HBM, the windows have no such form
    with pytest.raises(product.PxzError) as e:
        gpu.expand_windows_device([(300, 300)], [(0, 0, 0, 10, 10, 30, 0)], 3, 145, 145, 4, tiles[1], tiles[2], tiles[3],
                                  torch.full((total,), POISON, dtype=torch.uint8, device="cuda"))
    assert e.value.code == UNSUPPORTED


# ---- host form ------------------------------------------------------------------------------------------------------------

def test_host_form_reads_reference_files(gpu, product, oracle, golden_dir):
    base = open(os.path.join(golden_dir, "base.pixlzr"), "rb").read()
    img = np.ascontiguousarray(np.asarray(Image.open(os.path.join(golden_dir, "image.png")).convert("RGBA")))
    h, w = img.shape[:2]
    vals, tw, th, slots = oracle.shrink_image(img, 32, 32, 0, 4, 0.5)
    made = oracle.encode_container(w, h, 32, 32, 4, 0, vals, None, tw, th, slots)
    for raw, filt in ((base, 2), (made, 4)):
        fw, fh, bw, bh, c, _ = product.file_header(raw)
        d = oracle.decode_container(raw)
        exp = oracle.expand_image(fw, fh, bw, bh, c, filt, d["tw"], d["th"], d["slots"])
        rects = [(0, 0, 0, fw, fh), (0, fw // 3 | 1, fh // 3 | 1, min(bw + 7, fw - (fw // 3 | 1)), min(bh + 3, fh - (fh // 3 | 1))), (0, fw - 1, fh - 1, 1, 1)]
        crops, flags = gpu.decode_windows_files([raw], rects, c, bw, bh, filt)
        assert (flags == 0).all() and len(crops) == 3
        for (i, x, y, ww, hh), crop in zip(rects, crops):
            assert crop.shape == (hh, ww, c) and (crop == exp[y:y + hh, x:x + ww]).all(), (x, y, ww, hh)
        # trim gives the scratch back; the same call after it gives the same bytes
        gpu.trim()
        again, flags = gpu.decode_windows_files([raw], rects, c, bw, bh, filt)
        assert (flags == 0).all() and all((a == b).all() for a, b in zip(again, crops))


def test_host_form_refuses_a_header_that_disagrees(gpu, product, oracle):
    f = file_of(oracle, GEOMS[0], "alpha")
    other = File(oracle, 32, 32, 45, 40, "alpha", seed=9)
    windows, total = place([(0, 0, 0, 10, 10), (1, 5, 5, 30, 30)], 4)
    out = np.full(total, POISON, np.uint8)
    with pytest.raises(product.PxzError) as e:
        gpu.decode_windows_files([f.raw, other.raw], windows, 4, 32, 32, 2, sizes=[(100, 70), (45, 41)], out=out)
    assert e.value.code == INVALID_ARG and "image 1" in str(e.value)
    assert (out == POISON).all()
    # the same call with the right sizes, into padded rows at odd offsets; nothing outside the windows is written
    res, flags = gpu.decode_windows_files([f.raw, other.raw], windows, 4, 32, 32, 2, sizes=[(100, 70), (45, 40)], out=out)
    assert (flags == 0).all()
    assert (window_view(out, windows[0], 4) == f.image(2)[0:10, 0:10]).all() and (window_view(out, windows[1], 4) == other.image(2)[5:35, 5:35]).all()
    assert (out[outside_mask(out.size, windows, 4)] == POISON).all()
    # a window that would end behind the buffer is refused before anything is written
    out[:] = POISON
    with pytest.raises(product.PxzError) as e:
        gpu.decode_windows_files([f.raw, other.raw], windows, 4, 32, 32, 2, sizes=[(100, 70), (45, 40)], out=out[:windows[1][6] + 100])
    assert e.value.code == -7 and "window 1" in str(e.value)
    assert (out == POISON).all()
