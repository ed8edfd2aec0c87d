"""The decode side of batches of differently sized images (pxz_decode_varied_frames_device, pxz_expand_varied_frames_device,
pxz_decode_varied_files): every image's tiles and pixels equal the single-geometry calls on that file alone and the oracle, bit
for bit -- value bits, stored sizes, the valid slot bytes, every byte of the expanded image -- with every output poisoned before
each call.  The stored sizes are drawn (test_varied_decode_host.draw_tiles), not taken from the shrinker, so that every
resample form is met."""
import os
import struct

import numpy as np
import pytest
from PIL import Image

from test_gpu_varied import make_image, random_sizes
from test_varied_decode_host import ANY, FULL, HALVED, draw_tiles

pytestmark = pytest.mark.gpu

POISON = 0xA5
TILES = [(16, 16), (32, 32), (64, 64), (48, 20), (37, 61)]
INVALID_ARG, UNSUPPORTED = -1, -5


@pytest.fixture(scope="module")
def gpu(product):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    h = product.Handle(0)
    yield h
    h.close()


# ---- inputs -----------------------------------------------------------------------------------------------------------

def batch_sizes(rng, bw, bh, n_random):
    """a 1x1 image, one a pixel short of a tile, one a pixel past a tile (ragged on both axes), one ragged on each axis alone,
    and n_random images with sides up to 300, shuffled"""
    sizes = [(1, 1), (max(bw - 1, 1), max(bh - 1, 1)), (bw + 1, bh + 1), (2 * bw + 3, bh), (bw, 2 * bh + 5)]
    sizes += random_sizes(rng, n_random, 1, 300)
    return [sizes[k] for k in rng.permutation(len(sizes))]


class Batch:
    """files of the oracle's writer for drawn tiles, and what the oracle's reader makes of them"""

    def __init__(self, oracle, rng, sizes, bw, bh, c, check=True):
        self.sizes, self.bw, self.bh, self.c = sizes, bw, bh, c
        counts = [-(-w // bw) * -(-h // bh) for (w, h) in sizes]
        dealt = np.split(rng.permutation(np.arange(sum(counts)) % 3), np.cumsum(counts)[:-1])  # the classes, evenly over the batch
        self.tiles = [draw_tiles(rng, w, h, bw, bh, c, cl) for (w, h), cl in zip(sizes, dealt)]
        self.files = [oracle.encode_container(w, h, bw, bh, c, 0, t[0], None, t[1], t[2], t[3]) for (w, h), t in zip(sizes, self.tiles)]
        if check:
            self.check_conditions()

    def check_conditions(self):
        bw, bh = self.bw, self.bh
        classes = np.concatenate([t[4] for t in self.tiles])
        for k in (FULL, HALVED, ANY):
            assert (classes == k).sum() * 5 >= classes.size, f"class {k} holds {(classes == k).sum()} of {classes.size} tiles"
        assert (1, 1) in self.sizes
        assert any(w < bw and h < bh for (w, h) in self.sizes) or (bw == 1 and bh == 1)
        assert any(w > bw and w % bw for (w, h) in self.sizes) and any(h > bh and h % bh for (w, h) in self.sizes)


def upload_files(files, lead=3):
    """the files back to back in one CUDA buffer that starts `lead` bytes into its allocation -> (files, int64 offsets)"""
    import torch
    raw = b"".join(files)
    whole = torch.full((lead + len(raw),), POISON, dtype=torch.uint8, device="cuda")
    whole[lead:] = torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda()
    offs = torch.tensor(np.concatenate([[0], np.cumsum([len(f) for f in files])]), dtype=torch.int64).cuda()
    return whole[lead:], offs


def poisoned(T, slot, n_images):
    import torch
    dev = torch.device("cuda")
    vals = torch.full((T,), 0x7F7F7F7F, dtype=torch.int32, device=dev).view(torch.float32)
    ow = torch.full((T,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    oh = torch.full((T,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    slots = torch.full((T, slot), POISON, dtype=torch.uint8, device=dev)
    flags = torch.full((n_images,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    return (vals, ow, oh, slots), flags


def decode_varied(gpu, product, files, sizes, c, bw, bh, lead=3):
    """-> (tile offsets, (values, w, h, slots) as host arrays, per-image flags, pxz_decode_status)"""
    import torch
    buf, offs = upload_files(files, lead)
    to = product.varied_layout([(w, h, w * c, 0) for (w, h) in sizes], bw, bh)
    out, flags = poisoned(int(to[-1]), bw * bh * c, len(sizes))
    gpu.decode_varied_frames_device(buf, offs, sizes, c, bw, bh, out=out, image_flags=flags)
    status = gpu.decode_status()
    torch.cuda.synchronize()
    vals, ow, oh, slots = out
    host = (vals.cpu().numpy(), ow.cpu().numpy().astype(np.uint32), oh.cpu().numpy().astype(np.uint32), slots.cpu().numpy())
    return to, host, flags.cpu().numpy(), status, out


def decode_single(gpu, raw, size, c, bw, bh):
    """pxz_decode_frames_device on one file alone -> ((values, w, h, slots), status)"""
    import torch
    buf, offs = upload_files([raw], 1)
    vals, ow, oh, slots = gpu.decode_frames_device(buf, offs, (1, size[1], size[0], c), bw, bh)
    status = gpu.decode_status()
    torch.cuda.synchronize()
    return (vals[0].cpu().numpy(), ow[0].cpu().numpy().astype(np.uint32), oh[0].cpu().numpy().astype(np.uint32), slots[0].cpu().numpy()), status


def image_tiles(to, host, i):
    a, b = int(to[i]), int(to[i + 1])
    return tuple(x[a:b] for x in host)


def assert_tiles_equal(got, exp, c, what):
    gv, gw, gh, gs = got
    ev, ew, eh, es = exp
    assert (gw == ew).all() and (gh == eh).all(), f"{what}: stored sizes differ on {int(((gw != ew) | (gh != eh)).sum())} tiles"
    assert (gv.view(np.uint32) == ev.view(np.uint32)).all(), f"{what}: value bits differ"
    valid = ew.astype(np.int64) * eh * c
    width = min(gs.shape[1], es.shape[1])  # (the oracle's slots have room for four channels)
    idx = np.arange(width)[None, :] < valid[:, None]
    diff = (gs[:, :width] != es[:, :width]) & idx
    assert not diff.any(), f"{what}: {int(diff.sum())} slot bytes differ in {int(diff.any(axis=1).sum())} tiles"


def oracle_tiles(oracle, raw):
    d = oracle.decode_container(raw)
    return d["values"], d["tw"], d["th"], d["slots"]


def layout(sizes, c, pad=0, misalign=0):
    """descriptors of images at odd offsets (misalign) with padded rows (pad) in one buffer -> (descs, bytes)"""
    descs, at = [], 0
    for k, (w, h) in enumerate(sizes):
        pitch = w * c + pad * (k % 3)
        at += misalign * (k % 5) if misalign else 0
        descs.append((w, h, pitch, at))
        at += pitch * h
    return descs, at


def expand_varied(gpu, descs, total, c, bw, bh, filt, dev_tiles):
    """-> (the poisoned buffer after the call as a host array, per-image flags, status)"""
    import torch
    out = torch.full((total,), POISON, dtype=torch.uint8, device="cuda")
    flags = torch.full((len(descs),), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    _, ow, oh, slots = dev_tiles
    gpu.expand_varied_frames_device(descs, c, bw, bh, filt, ow, oh, slots, out, image_flags=flags)
    status = gpu.decode_status()
    torch.cuda.synchronize()
    return out.cpu().numpy(), flags.cpu().numpy(), status


def image_of(buf, desc, c):
    w, h, pitch, off = desc
    return np.lib.stride_tricks.as_strided(buf[off:], (h, w, c), (pitch, c, 1))


def expand_single(gpu, size, c, bw, bh, filt, dev_tiles, a, b):
    import torch
    _, ow, oh, slots = dev_tiles
    out = gpu.expand_frames_device((1, size[1], size[0], c), bw, bh, filt, ow[a:b][None].contiguous(), oh[a:b][None].contiguous(),
                                   slots[a:b][None].contiguous())
    torch.cuda.synchronize()
    return out[0].cpu().numpy()


def check_expand(gpu, oracle, batch, to, dev_tiles, host, filt, pad, misalign, what, with_single=True):
    c, bw, bh = batch.c, batch.bw, batch.bh
    descs, total = layout(batch.sizes, c, pad, misalign)
    buf, flags, status = expand_varied(gpu, descs, total, c, bw, bh, filt, dev_tiles)
    assert status == 0 and (flags == 0).all(), f"{what}: status {status}, flags {flags}"
    covered = np.zeros(total, bool)
    for i, (d, size) in enumerate(zip(descs, batch.sizes)):
        a, b = int(to[i]), int(to[i + 1])
        got = image_of(buf, d, c)
        exp = oracle.expand_image(size[0], size[1], bw, bh, c, filt, host[1][a:b], host[2][a:b], host[3][a:b])
        bad = (got != exp).any(axis=2)
        assert not bad.any(), f"{what} image {i} {size}: {int(bad.sum())} pixels differ from the oracle"
        if with_single:
            one = expand_single(gpu, size, c, bw, bh, filt, dev_tiles, a, b)
            assert (got == one).all(), f"{what} image {i} {size}: differs from pxz_expand_frames_device"
        for y in range(size[1]):
            covered[d[3] + y * d[2]: d[3] + y * d[2] + size[0] * c] = True
    assert (buf[~covered] == POISON).all(), f"{what}: bytes outside the images were written"


# ---- reader and expand against the single calls and the oracle ------------------------------------------------------------

@pytest.mark.parametrize("c", [3, 4])
@pytest.mark.parametrize("tile", TILES, ids=lambda t: f"{t[0]}x{t[1]}")
def test_batches_equal_single_calls_and_oracle(gpu, product, oracle, tile, c):
    """reader: values, sizes and valid slot bytes per image; expand: all five filters, images at odd offsets with padded rows"""
    bw, bh = tile
    seed = bw * 131 + bh * 7 + c
    rng = np.random.default_rng(seed)
    batch = Batch(oracle, rng, batch_sizes(rng, bw, bh, int(rng.integers(0, 7))), bw, bh, c)
    assert 3 <= len(batch.sizes) <= 11
    to, host, flags, status, dev = decode_varied(gpu, product, batch.files, batch.sizes, c, bw, bh, lead=seed % 7 + 1)
    assert status == 0 and (flags == 0).all()
    for i, (raw, size) in enumerate(zip(batch.files, batch.sizes)):
        got = image_tiles(to, host, i)
        one, st = decode_single(gpu, raw, size, c, bw, bh)
        assert st == 0
        assert_tiles_equal(got, one, c, f"{bw}x{bh} C{c} image {i} {size} vs pxz_decode_frames_device")
        assert_tiles_equal(got, oracle_tiles(oracle, raw), c, f"{bw}x{bh} C{c} image {i} {size} vs oracle")
        assert_tiles_equal(got, batch.tiles[i][:4], c, f"{bw}x{bh} C{c} image {i} {size} vs what was written")
    for filt in range(5):
        check_expand(gpu, oracle, batch, to, dev, host, filt, pad=4 * (seed % 3) + 3, misalign=seed % 7 + 1,
                     what=f"{bw}x{bh} C{c} filter {filt}")
    # rows and offsets that are multiples of 4 (RGBA: the 16-byte stores)
    check_expand(gpu, oracle, batch, to, dev, host, 4, pad=16, misalign=0, what=f"{bw}x{bh} C{c} aligned")


def test_n_images_1_equals_the_single_calls(gpu, product, oracle):
    rng = np.random.default_rng(3)
    for (w, h, c, bw, bh) in [(333, 217, 4, 32, 32), (640, 360, 3, 64, 64), (17, 5, 4, 16, 16)]:
        batch = Batch(oracle, rng, [(w, h)], bw, bh, c, check=False)
        to, host, flags, status, dev = decode_varied(gpu, product, batch.files, batch.sizes, c, bw, bh)
        assert status == 0 and flags.tolist() == [0]
        one, _ = decode_single(gpu, batch.files[0], (w, h), c, bw, bh)
        assert_tiles_equal(image_tiles(to, host, 0), one, c, f"n=1 {w}x{h}")
        for filt in (0, 2, 4):
            check_expand(gpu, oracle, batch, to, dev, host, filt, pad=0, misalign=0, what=f"n=1 {w}x{h} filter {filt}")


def test_equal_geometries_equal_the_frames_calls(gpu, product, oracle):
    import torch
    rng = np.random.default_rng(4)
    n, w, h, c, bw, bh = 5, 200, 136, 4, 32, 32
    batch = Batch(oracle, rng, [(w, h)] * n, bw, bh, c, check=False)
    to, host, flags, status, dev = decode_varied(gpu, product, batch.files, batch.sizes, c, bw, bh)
    buf, offs = upload_files(batch.files, 5)
    vals, ow, oh, slots = gpu.decode_frames_device(buf, offs, (n, h, w, c), bw, bh)
    torch.cuda.synchronize()
    T = int(to[1])
    frames = (vals.cpu().numpy().reshape(-1), ow.cpu().numpy().astype(np.uint32).reshape(-1), oh.cpu().numpy().astype(np.uint32).reshape(-1),
              slots.cpu().numpy().reshape(n * T, -1))
    assert_tiles_equal(host, frames, c, "equal geometries, reader")
    for filt in (0, 1, 4):
        descs = [(w, h, w * c, k * w * h * c) for k in range(n)]
        got, fl, st = expand_varied(gpu, descs, n * w * h * c, c, bw, bh, filt, dev)
        exp = gpu.expand_frames_device((n, h, w, c), bw, bh, filt, ow, oh, slots)
        torch.cuda.synchronize()
        assert st == 0 and (got == exp.cpu().numpy().reshape(-1)).all(), f"equal geometries, expand filter {filt}"


# ---- end to end -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c,mode,factor", [(4, 0, 0.06), (3, 1, 2.0)])
def test_shrink_encode_decode_expand_chain(gpu, product, oracle, c, mode, factor):
    import torch
    bw = bh = 32
    rng = np.random.default_rng(31 + c)
    sizes = [(w if w % bw != 1 else w + 1, h if h % bh != 1 else h + 1) for (w, h) in random_sizes(rng, 7, 2, 300)] + [(2, 2), (bw + 2, bh - 1)]
    images = [make_image(rng, w, h, c, ["opaque", "partial", "clear"][k % 3]) for k, (w, h) in enumerate(sizes)]
    descs, total = layout(sizes, c)
    host_buf = np.zeros(total, np.uint8)
    for d, img in zip(descs, images):
        image_of(host_buf, d, c)[...] = img
    buf = torch.from_numpy(host_buf).cuda()
    to, vals, ow, oh, slots = gpu.shrink_varied_frames_device(buf, bw, bh, mode, 4, factor, descs=descs, channels=c)
    foffs, fbuf = gpu.encode_varied_frames_device(sizes, c, bw, bh, vals, ow, oh, slots)
    T = int(to[-1])
    out, flags = poisoned(T, bw * bh * c, len(sizes))
    gpu.decode_varied_frames_device(fbuf, foffs, sizes, c, bw, bh, out=out, image_flags=flags)
    assert gpu.decode_status() == 0 and (flags == 0).all()
    torch.cuda.synchronize()
    hw, hh = ow.cpu().numpy(), oh.cpu().numpy()
    assert len(set(zip(hw.tolist(), hh.tolist()))) >= 8  # the factor spreads the levels
    for filt in (0, 4):
        got, fl, st = expand_varied(gpu, descs, total, c, bw, bh, filt, out)
        assert st == 0 and (fl == 0).all()
        for i, img in enumerate(images):
            ev, ew, eh, es = oracle.shrink_image(np.ascontiguousarray(img), bw, bh, mode, 4, factor, nthreads=8)
            raw = oracle.encode_container(sizes[i][0], sizes[i][1], bw, bh, c, 0, ev, None, ew, eh, es)
            d = oracle.decode_container(raw)
            exp = oracle.expand_image(sizes[i][0], sizes[i][1], bw, bh, c, filt, d["tw"], d["th"], d["slots"][:, : bw * bh * c].copy())
            assert (image_of(got, descs[i], c) == exp).all(), f"mode {mode} filter {filt} image {i} {sizes[i]}"


def test_big_ruscher_in_a_batch_expands_to_its_png(gpu, product, oracle, golden_dir):
    raw = open(os.path.join(golden_dir, "Big-Ruscher.pix"), "rb").read()
    ref = np.asarray(Image.open(os.path.join(golden_dir, "Big-Ruscher.pix.png")))[..., :3]
    w, h, bw, bh, c, _ = product.file_header(raw)
    assert c == 3
    rng = np.random.default_rng(8)
    others = Batch(oracle, rng, [(97, 61), (5, 3), (300, 120)], bw, bh, 3, check=False)
    files = [others.files[0], raw, others.files[1], others.files[2]]
    sizes = [others.sizes[0], (w, h), others.sizes[1], others.sizes[2]]
    to, host, flags, status, dev = decode_varied(gpu, product, files, sizes, 3, bw, bh)
    assert status == 0 and (flags == 0).all()
    descs, total = layout(sizes, 3, pad=5, misalign=1)
    got, fl, st = expand_varied(gpu, descs, total, 3, bw, bh, 0, dev)
    assert st == 0
    assert (image_of(got, descs[1], 3) == ref).all()


@pytest.mark.parametrize("block", [8, 64])
def test_reference_container_tests_as_varied_batches(gpu, product, oracle, golden_dir, block):
    """src/bin/main.rs:299-356: image.png cut into tiles at full size, written without values (has_value = 0), file -> image ==
    input; here in a batch with a second, differently sized image treated the same way"""
    first = np.array(Image.open(os.path.join(golden_dir, "image.png")).convert("RGBA"))
    second = make_image(np.random.default_rng(12), 75, 131, 4, "partial")
    files, sizes = [], []
    for img in (first, second):
        h, w, _ = img.shape
        cols, rows = -(-w // block), -(-h // block)
        n = cols * rows
        tw, th = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        slots = np.zeros((n, block * block * 4), np.uint8)
        for t in range(n):
            ty, tx = divmod(t, cols)
            tile = img[ty * block:(ty + 1) * block, tx * block:(tx + 1) * block]
            th[t], tw[t] = tile.shape[:2]
            slots[t, : tile.size] = tile.ravel()
        files.append(oracle.encode_container(w, h, block, block, 4, 0, np.zeros(n, np.float32), np.zeros(n, np.uint8), tw, th, slots))
        sizes.append((w, h))
    to, host, flags, status, dev = decode_varied(gpu, product, files, sizes, 4, block, block)
    assert status == 0 and (flags == 0).all() and (host[0].view(np.uint32) == 0).all()
    descs, total = layout(sizes, 4, pad=3, misalign=1)
    got, fl, st = expand_varied(gpu, descs, total, 4, block, block, 0, dev)
    assert st == 0
    for d, img in zip(descs, (first, second)):
        assert (image_of(got, d, 4) == img).all()


# ---- more images than a block keeps first tiles of in LDS --------------------------------------------------------------------

MANY = 2049                                       # one more than kVxImages (pxz_device.h): the owner search reads the table itself
MANY_SIZES = [(4, 4), (5, 3), (3, 6), (9, 4)]     # in 4x4 blocks: 1, 2, 2 and 3 tiles, edge tiles 1 and 3 wide, 3 and 2 high


class ManyImages:
    """MANY images of a few pixels each in 4x4 blocks, the sizes of MANY_SIZES in turn.  Stored sizes by hand, five shapes dealt in
    turn over the batch's tiles (full, lower, narrower, a pixel less on both axes, 1x1); random source pixels and stored bytes, a
    tile stored at its full size holds its source (what a shrinker stores there, and what the distortion calls assume).  Every
    file passes the oracle's reader alone, and the oracle's per-image expand is computed once per filter -- all on the CPU."""
    bw = bh = 4

    def __init__(self, oracle, c):
        rng = np.random.default_rng(2049 * c)
        self.oracle, self.c, self._expected = oracle, c, {}
        self.sizes = [MANY_SIZES[i % len(MANY_SIZES)] for i in range(MANY)]
        self.images, self.tiles, self.files, rank = [], [], [], 0
        for (w, h) in self.sizes:
            img = rng.integers(0, 256, (h, w, c), dtype=np.uint8)
            cols, rows = -(-w // 4), -(-h // 4)
            n = cols * rows
            vals = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32).view(np.float32)
            tw, th, slots = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros((n, 16 * c), np.uint8)
            for t in range(n):
                x, y = t % cols * 4, t // cols * 4
                fw, fh = min(4, w - x), min(4, h - y)
                sw, sh = [(fw, fh), (fw, max(fh // 2, 1)), (max(fw // 2, 1), fh), (max(fw - 1, 1), max(fh - 1, 1)), (1, 1)][rank % 5]
                rank += 1
                tw[t], th[t] = sw, sh
                px = img[y:y + fh, x:x + fw] if (sw, sh) == (fw, fh) else rng.integers(0, 256, (sh, sw, c), dtype=np.uint8)
                slots[t, :sw * sh * c] = px.reshape(-1)
            raw = oracle.encode_container(w, h, 4, 4, c, 0, vals, None, tw, th, slots)
            d = oracle.decode_container(raw)  # valid for the reference alone: nothing refused, every tile as written
            assert (d["tw"] == tw).all() and (d["th"] == th).all() and (d["values"].view(np.uint32) == vals.view(np.uint32)).all()
            self.images.append(img), self.tiles.append((vals, tw, th, slots)), self.files.append(raw)
        self.flat = tuple(np.concatenate([t[k] for t in self.tiles]) for k in range(4))
        counts = {n: sum(1 for t in self.tiles if t[1].size == n) for n in (1, 2, 3)}
        assert all(counts.values()) and sum(counts.values()) == MANY, counts
        full = self.flat[1] * self.flat[2] == 16
        assert full.any() and (self.flat[1] == 1).any() and (self.flat[1] == 3).any() and not full.all()

    def expected(self, filt):
        """the oracle's expand of every image"""
        if filt not in self._expected:
            self._expected[filt] = [self.oracle.expand_image(w, h, 4, 4, self.c, filt, t[1], t[2], t[3]) for (w, h), t in zip(self.sizes, self.tiles)]
        return self._expected[filt]


_many = {}


def many_images(oracle, c):
    if c not in _many:
        _many[c] = ManyImages(oracle, c)
    return _many[c]


@pytest.mark.parametrize("c", [3, 4])
def test_2049_images_find_their_tiles_in_the_table_itself(gpu, product, oracle, c):
    """reader (one wave per tile row, one thread per tile) and expand (Nearest, Lanczos3) of MANY images: every tile as written,
    every image byte for byte the oracle's; then the LAST image's first tile with stored width 0: its flag alone"""
    m = many_images(oracle, c)
    to, host, flags, status, dev = decode_varied(gpu, product, m.files, m.sizes, c, 4, 4)
    assert status == 0 and (flags == 0).all()
    assert int(to[-1]) == m.flat[1].size
    assert_tiles_equal(host, m.flat, c, f"C{c} {MANY} images vs what was written")
    descs, total = layout(m.sizes, c, pad=3, misalign=1)
    covered = np.zeros(total, bool)
    for (w, h, pitch, off) in descs:
        for y in range(h):
            covered[off + y * pitch: off + y * pitch + w * c] = True
    for filt in (0, 4):
        buf, fl, st = expand_varied(gpu, descs, total, c, 4, 4, filt, dev)
        assert st == 0 and (fl == 0).all(), f"filter {filt}: status {st}, flags of {np.flatnonzero(fl).tolist()}"
        bad = [i for i, (d, exp) in enumerate(zip(descs, m.expected(filt))) if not (image_of(buf, d, c) == exp).all()]
        print(f"C{c} filter {filt}: {len(bad)} of {MANY} images differ from the oracle")
        assert not bad, f"C{c} filter {filt}: images {bad[:10]} differ from the oracle"
        assert (buf[~covered] == POISON).all(), f"C{c} filter {filt}: bytes outside the images were written"
    last = MANY - 1
    assert int(to[last + 1]) - int(to[last]) == 1  # (a 4x4 image: one tile)
    ow = dev[1].clone()
    ow[int(to[last])] = 0
    buf, fl, st = expand_varied(gpu, descs, total, c, 4, 4, 4, (dev[0], ow, dev[2], dev[3]))
    assert st == 1 and fl.tolist() == [0] * last + [1]
    assert (image_of(buf, descs[last], c) == POISON).all()
    bad = [i for i in range(last) if not (image_of(buf, descs[i], c) == m.expected(4)[i]).all()]
    assert not bad, f"C{c}: images {bad[:10]} beside the flagged one are not complete"
    assert (buf[~covered] == POISON).all()


# ---- malformed files in a batch ------------------------------------------------------------------------------------------

def one_tile_file(w, h, bw, bh, c, ops):
    """a .pixlzr file of one w x h image in bw x bh blocks whose only tile has the QOI op stream `ops`, laid out as encode_block does"""
    body = struct.pack(">IIBB", w, h, c, 0) + bytes(ops) + bytes([0, 0, 0, 0, 0, 0, 0, 1])
    rec = b"block" + struct.pack(">f", 0.5) + struct.pack(">I", len(body)) + body
    return b"PIXLZR" + bytes([0, 0, 2, 0]) + struct.pack(">IIII", w, h, bw, bh) + struct.pack(">I", len(rec)) + rec


def malform(kind, raw, size, bw, bh, c):
    """-> (the file, the size its descriptor announces)"""
    rows = -(-size[1] // bh)
    first = 26 + 4 * rows
    b = bytearray(raw)
    if kind == "magic":
        b[0] = ord("Q")
    elif kind == "size":
        return raw, (size[0] + 1, size[1])
    elif kind == "truncated":
        b = b[:-5]
    elif kind == "length":
        b[first + 9:first + 13] = struct.pack(">I", 0x00ffffff)
    elif kind == "channels":
        b[first + 21] = 7 - c
    else:
        raise ValueError(kind)
    return bytes(b), size


@pytest.mark.parametrize("place", ["first", "middle", "last"])
def test_malformed_files_leave_the_other_images_alone(gpu, product, oracle, place):
    bw = bh = 32
    c = 4
    rng = np.random.default_rng(77)
    sizes = batch_sizes(rng, bw, bh, 3)
    batch = Batch(oracle, rng, sizes, bw, bh, c)
    n = len(sizes)
    clean_to, clean, flags, status, _ = decode_varied(gpu, product, batch.files, sizes, c, bw, bh)
    assert status == 0 and (flags == 0).all()
    k = {"first": 0, "middle": n // 2, "last": n - 1}[place]
    for kind in ("magic", "size", "truncated", "length", "channels", "dry"):
        files, descs = list(batch.files), list(sizes)
        if kind == "dry":  # an op stream that ends after one pixel of a 5 x 3 tile
            files[k], descs[k] = one_tile_file(5, 3, bw, bh, c, [0xfe, 1, 2, 3]), (5, 3)
        else:
            files[k], descs[k] = malform(kind, batch.files[k], sizes[k], bw, bh, c)
        to, host, flags, status, dev = decode_varied(gpu, product, files, descs, c, bw, bh)
        assert status & 2, kind
        assert flags.tolist() == [2 if i == k else 0 for i in range(n)], f"{kind} at {place}: {flags}"
        one, st = decode_single(gpu, files[k], descs[k], c, bw, bh)
        assert st == 2
        gw, gh = image_tiles(to, host, k)[1:3]
        assert (gw == one[1]).all() and (gh == one[2]).all(), f"{kind} at {place}: sizes of the flagged image"
        assert (gw == 0).any()
        usable = gw != 0
        if usable.any():  # what the single call could read of it, the batch reads too
            assert_tiles_equal(tuple(x[usable] for x in image_tiles(to, host, k)), tuple(x[usable] for x in one), c, f"{kind}: usable tiles")
        for i in range(n):
            if i != k:
                got, exp = image_tiles(to, host, i), image_tiles(clean_to, clean, i)
                assert all((g == e).all() for g, e in zip((got[0].view(np.uint32),) + got[1:], (exp[0].view(np.uint32),) + exp[1:])), \
                    f"{kind} at {place}: image {i} differs from the clean batch"
        # expand of the flagged tiles: bit 0 and flag 1 for that image only, its unusable places untouched
        d, total = layout(descs, c, pad=3, misalign=1)
        got, fl, st = expand_varied(gpu, d, total, c, bw, bh, 4, dev)
        assert st == 1 and fl.tolist() == [1 if i == k else 0 for i in range(n)], f"{kind} at {place}: expand flags {fl}"
        for i in range(n):
            if i != k:
                a, b = int(to[i]), int(to[i + 1])
                exp = oracle.expand_image(descs[i][0], descs[i][1], bw, bh, c, 4, host[1][a:b], host[2][a:b], host[3][a:b])
                assert (image_of(got, d[i], c) == exp).all()


def test_stored_size_above_its_place_flags_that_image_only(gpu, product, oracle):
    import torch
    bw = bh = 32
    c = 4
    rng = np.random.default_rng(78)
    sizes = batch_sizes(rng, bw, bh, 2)
    batch = Batch(oracle, rng, sizes, bw, bh, c)
    to, host, flags, status, dev = decode_varied(gpu, product, batch.files, sizes, c, bw, bh)
    k = next(i for i, s in enumerate(sizes) if s == (bw + 1, bh + 1))
    bad_t = int(to[k]) + 1  # the 1 x 32 tile of the ragged column
    ow = dev[1].clone()
    ow[bad_t] = 2
    d, total = layout(sizes, c, pad=3, misalign=1)
    got, fl, st = expand_varied(gpu, d, total, c, bw, bh, 2, (dev[0], ow, dev[2], dev[3]))
    assert st == 1 and fl.tolist() == [1 if i == k else 0 for i in range(len(sizes))]
    img = image_of(got, d[k], c)
    assert (img[:bh, bw:] == POISON).all()  # the place is untouched
    a, b = int(to[k]), int(to[k + 1])
    exp = oracle.expand_image(bw + 1, bh + 1, bw, bh, c, 2, host[1][a:b], host[2][a:b], host[3][a:b])
    assert (img[:bh, :bw] == exp[:bh, :bw]).all() and (img[bh:] == exp[bh:]).all()


# ---- host form ------------------------------------------------------------------------------------------------------------

def test_host_form_equals_the_oracle_per_image(gpu, product, oracle):
    rng = np.random.default_rng(9)
    for c, (bw, bh), filt in ((4, (32, 32), 4), (3, (48, 20), 1)):
        sizes = random_sizes(rng, 8, 1, 400) + [(1, 1), (bw - 1, bh)]
        batch = Batch(oracle, rng, sizes, bw, bh, c, check=False)
        images, flags = gpu.decode_varied_files(batch.files, c, bw, bh, filt)
        assert (flags == 0).all() and len(images) == 10
        for i, (w, h) in enumerate(sizes):
            t = batch.tiles[i]
            assert (images[i] == oracle.expand_image(w, h, bw, bh, c, filt, t[1], t[2], t[3])).all(), f"C{c} image {i} ({w}x{h})"
        # a header that disagrees with its descriptor names the file and writes nothing
        descs, total = layout(sizes, c, pad=2, misalign=1)
        wrong = list(descs)
        wrong[6] = (descs[6][0], descs[6][1] + 1, descs[6][2], descs[6][3])
        out = np.full(total + 400 * c, POISON, np.uint8)
        with pytest.raises(product.PxzError) as e:
            gpu.decode_varied_files(batch.files, c, bw, bh, filt, out=out, descs=wrong)
        assert e.value.code == INVALID_ARG and "image 6" in str(e.value)
        assert (out == POISON).all()
        # a file broken past its header comes back flagged, the others complete, gaps and padding untouched
        files = list(batch.files)
        files[3] = files[3][:-9]
        with pytest.raises(product.PxzError) as e:
            gpu.decode_varied_files(files, c, bw, bh, filt, out=out, descs=descs)
        assert e.value.code == INVALID_ARG and "image 3" in str(e.value)
        assert [int(f != 0) for f in e.value.flags] == [int(i == 3) for i in range(10)] and e.value.flags[3] & 2
        covered = np.zeros(out.size, bool)
        for i, (d, (w, h)) in enumerate(zip(descs, sizes)):
            for y in range(h):
                covered[d[3] + y * d[2]: d[3] + y * d[2] + w * c] = True
            if i != 3:
                t = batch.tiles[i]
                assert (image_of(out, d, c) == oracle.expand_image(w, h, bw, bh, c, filt, t[1], t[2], t[3])).all(), f"image {i} beside a broken file"
        assert (out[~covered] == POISON).all()


# ---- errors ---------------------------------------------------------------------------------------------------------------

def test_errors_name_the_image_and_write_nothing(gpu, product, oracle):
    import torch
    L = product.binding.load_library()
    rng = np.random.default_rng(2)
    bw = bh = 16
    c = 4
    sizes = [(40, 40), (33, 20), (50, 60)]
    batch = Batch(oracle, rng, sizes, bw, bh, c, check=False)
    buf, offs = upload_files(batch.files)
    T = int(product.varied_layout([(w, h, w * c, 0) for (w, h) in sizes], bw, bh)[-1])
    good, total = layout(sizes, c)
    import ctypes as C
    P, descs_of = product.binding.Params, product.binding.image_descs

    def call_decode(geoms, n, channels, pd, out, flags, files=buf, file_offs=offs):
        vals, ow, oh, slots = out
        return L.pxz_decode_varied_frames_device(gpu._h, C.cast(descs_of(geoms), C.c_void_p) if geoms is not None else None, n, channels,
                                                 C.byref(pd) if pd is not None else None, C.c_void_p(files.data_ptr()) if files is not None else None,
                                                 C.c_void_p(file_offs.data_ptr()), C.c_void_p(vals.data_ptr()), C.c_void_p(ow.data_ptr()),
                                                 C.c_void_p(oh.data_ptr()), C.c_void_p(slots.data_ptr()), C.c_void_p(flags.data_ptr()))

    def call_expand(geoms, n, channels, pd, tiles, out, flags, null_slots=False):
        _, ow, oh, slots = tiles
        return L.pxz_expand_varied_frames_device(gpu._h, C.cast(descs_of(geoms), C.c_void_p) if geoms is not None else None, n, channels,
                                                 C.byref(pd) if pd is not None else None, C.c_void_p(ow.data_ptr()), C.c_void_p(oh.data_ptr()),
                                                 None if null_slots else C.c_void_p(slots.data_ptr()), C.c_void_p(out.data_ptr()),
                                                 C.c_void_p(flags.data_ptr()))

    geo = [(w, h, w * c, 0) for (w, h) in sizes]
    ok = P(bw, bh, 0, 4, 0.0, 0)
    decode_cases = [
        (geo, 3, c, None, True, INVALID_ARG, None),                                     # null params
        (geo, 3, c, ok, None, INVALID_ARG, None),                                       # null files
        (None, 3, c, ok, True, INVALID_ARG, None),                                      # null descriptors
        (geo, 0, c, ok, True, INVALID_ARG, None),                                       # empty batch
        (geo, 3, 5, ok, True, INVALID_ARG, None),                                       # channels
        (geo, 3, c, P(0, bh, 0, 4, 0.0, 0), True, INVALID_ARG, None),                   # zero block side
        ([geo[0], geo[1], (0, 10, 40, 0)], 3, c, ok, True, INVALID_ARG, "image 2"),     # zero side
        ([geo[0], geo[1] + (1,), geo[2]], 3, c, ok, True, INVALID_ARG, "image 1"),      # reserved set
        ([geo[0], ((1 << 24) + 1, 4, 4, 0), geo[2]], 3, c, ok, True, UNSUPPORTED, "image 1"),  # side above 2^24
    ]
    for geoms, n, ch, pd, files, code, name in decode_cases:
        out, flags = poisoned(T, bw * bh * c, 3)
        rc = call_decode(geoms, n, ch, pd, out, flags, files=buf if files else None)
        assert rc == code, (geoms, n, ch, rc)
        if name:
            assert name in L.pxz_last_error(gpu._h).decode()
        torch.cuda.synchronize()
        vals, ow, oh, slots = out
        assert (vals.view(torch.int32) == 0x7F7F7F7F).all() and (ow == 0x5A5A5A5A).all() and (oh == 0x5A5A5A5A).all()
        assert (slots == POISON).all() and (flags == 0x5A5A5A5A).all()

    to, host, fl, st, tiles = decode_varied(gpu, product, batch.files, sizes, c, bw, bh)
    expand_cases = [
        (good, 3, c, None, False, INVALID_ARG, None),                                                   # null params
        (good, 3, c, ok, True, INVALID_ARG, None),                                                      # null slots
        (None, 3, c, ok, False, INVALID_ARG, None),
        (good, 0, c, ok, False, INVALID_ARG, None),
        (good, 3, 2, ok, False, INVALID_ARG, None),
        (good, 3, c, P(bw, bh, 0, 5, 0.0, 0), False, INVALID_ARG, None),                                # filter 5
        (good, 3, c, P(bw, 0, 0, 4, 0.0, 0), False, INVALID_ARG, None),
        ([good[0], (good[1][0], good[1][1], 4, good[1][3]), good[2]], 3, c, ok, False, INVALID_ARG, "image 1"),  # pitch below a row
        ([good[0], good[1], (10, 0, 40, 0)], 3, c, ok, False, INVALID_ARG, "image 2"),                  # zero side
        ([good[0] + (1,), good[1], good[2]], 3, c, ok, False, INVALID_ARG, "image 0"),                  # reserved set
        (good, 3, c, P(160, 160, 0, 4, 0.0, 0), False, UNSUPPORTED, None),                              # 160x160 RGBA blocks
    ]
    for geoms, n, ch, pd, null_slots, code, name in expand_cases:
        out = torch.full((total,), POISON, dtype=torch.uint8, device="cuda")
        flags = torch.full((3,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        rc = call_expand(geoms, n, ch, pd, tiles, out, flags, null_slots)
        assert rc == code, (geoms, n, ch, rc)
        if name:
            assert name in L.pxz_last_error(gpu._h).decode()
        torch.cuda.synchronize()
        assert (out == POISON).all() and (flags == 0x5A5A5A5A).all()
    # the reader has no such limit: nothing of a tile is staged
    big = Batch(oracle, rng, [(170, 163), (3, 3)], 160, 160, 4, check=False)
    to, host, fl, st, _ = decode_varied(gpu, product, big.files, big.sizes, 4, 160, 160)
    assert st == 0
    assert_tiles_equal(image_tiles(to, host, 0), big.tiles[0][:4], 4, "160x160 blocks through the reader")


# ---- handle state -----------------------------------------------------------------------------------------------------------

def test_single_varied_single_sequence_on_one_handle_equals_fresh_handles(gpu, product, oracle):
    import torch
    rng = np.random.default_rng(21)
    single = Batch(oracle, rng, [(300, 200)] * 2, 32, 32, 4, check=False)
    a = Batch(oracle, rng, batch_sizes(rng, 32, 32, 2), 32, 32, 4)
    b = Batch(oracle, rng, batch_sizes(rng, 64, 64, 3), 64, 64, 4)
    steps = [("single", single), ("varied", a), ("single", single), ("trim", None), ("varied", b), ("varied", a), ("single", single)]

    def run(h, step):
        kind, bt = step
        if kind == "trim":
            h.trim()
            return []
        if kind == "single":
            buf, offs = upload_files(bt.files, 1)
            vals, ow, oh, slots = h.decode_frames_device(buf, offs, (2, 200, 300, 4), 32, 32)
            img = h.expand_frames_device((2, 200, 300, 4), 32, 32, 4, ow, oh, slots)
            st = h.decode_status()
            torch.cuda.synchronize()
            return [vals.view(torch.int32).cpu().numpy(), ow.cpu().numpy(), oh.cpu().numpy(), img.cpu().numpy(), np.array([st])]
        to, host, flags, st, dev = decode_varied(h, product, bt.files, bt.sizes, bt.c, bt.bw, bt.bh)
        descs, total = layout(bt.sizes, bt.c, pad=3, misalign=1)
        img, fl, st2 = expand_varied(h, descs, total, bt.c, bt.bw, bt.bh, 4, dev)
        valid = (host[1].astype(np.int64) * host[2] * bt.c)[:, None]
        slots = np.where(np.arange(host[3].shape[1])[None, :] < valid, host[3], 0)
        return [host[0].view(np.uint32), host[1], host[2], slots, img, flags, fl, np.array([st, st2])]

    shared = [run(gpu, s) for s in steps]
    for k, (s, got) in enumerate(zip(steps, shared)):
        fresh = product.Handle(0)
        try:
            exp = run(fresh, s)
        finally:
            fresh.close()
        for g, e in zip(got, exp):
            assert (g == e).all(), f"step {k} ({s[0]}) on a used handle differs from a fresh one"


# ---- scale ------------------------------------------------------------------------------------------------------------------

def test_full_size_frames_mixed_with_hundreds_of_small_images(gpu, product, oracle):
    """three 8K frames' files shuffled among 300 files of images up to 120 px, 64x64 blocks: the 8K images and every tenth small
    one equal their single calls; then the 8K images behind a 4.2-GB gap of the output buffer (64-bit offsets)"""
    import torch
    rng = np.random.default_rng(99)
    bw = bh = 64
    c = 4
    frames = gpu.synth_frames_device(3, 4320, 7680, c, dist=product.DIST_ALPHA)
    vals, ow, oh, slots = gpu.shrink_frames_device(frames, bw, bh, 1, 4, 16.0)
    foffs, fbuf = gpu.encode_frames_device(tuple(frames.shape), bw, bh, vals, ow, oh, slots)
    torch.cuda.synchronize()
    del frames, vals, ow, oh, slots
    fo = foffs.cpu().numpy()
    big_files = [fbuf[int(fo[k]):int(fo[k + 1])].cpu().numpy().tobytes() for k in range(3)]
    del fbuf
    torch.cuda.empty_cache()
    small = Batch(oracle, rng, random_sizes(rng, 300, 1, 120), bw, bh, c, check=False)
    files = big_files + small.files
    sizes = [(7680, 4320)] * 3 + small.sizes
    order = rng.permutation(len(files))
    files, sizes = [files[k] for k in order], [sizes[k] for k in order]
    buf, offs = upload_files(files, 1)
    to = product.varied_layout([(w, h, w * c, 0) for (w, h) in sizes], bw, bh)
    out, flags = poisoned(int(to[-1]), bw * bh * c, len(sizes))
    gpu.decode_varied_frames_device(buf, offs, sizes, c, bw, bh, out=out, image_flags=flags)
    assert gpu.decode_status() == 0 and (flags == 0).all()
    torch.cuda.synchronize()
    picked = [i for i, s in enumerate(sizes) if s[0] == 7680 or i % 10 == 0]
    for i in picked:
        a, b = int(to[i]), int(to[i + 1])
        got = (out[0][a:b].cpu().numpy(), out[1][a:b].cpu().numpy().astype(np.uint32), out[2][a:b].cpu().numpy().astype(np.uint32),
               out[3][a:b].cpu().numpy())
        one, st = decode_single(gpu, files[i], sizes[i], c, bw, bh)
        assert st == 0
        assert_tiles_equal(got, one, c, f"image {i} {sizes[i]}")
    # expand: small images first, then the 8K images behind a gap so that their offsets pass 4 GiB
    descs, at = [None] * len(sizes), 0
    for i, (w, h) in enumerate(sizes):
        if w != 7680:
            descs[i] = (w, h, w * c + 4, at + 1)
            at += (w * c + 4) * h + 1
    at = 4_200_000_000 + 3
    for i, (w, h) in enumerate(sizes):
        if w == 7680:
            descs[i] = (w, h, w * c, at)
            at += w * h * c
    total = at
    img = torch.empty(total, dtype=torch.uint8, device="cuda")
    gpu.expand_varied_frames_device(descs, c, bw, bh, 4, out[1], out[2], out[3], img)
    assert gpu.decode_status() == 0
    torch.cuda.synchronize()
    for i in picked:
        w, h, pitch, off = descs[i]
        a, b = int(to[i]), int(to[i + 1])
        one = gpu.expand_frames_device((1, h, w, c), bw, bh, 4, out[1][a:b][None].contiguous(), out[2][a:b][None].contiguous(),
                                       out[3][a:b][None].contiguous())
        got = torch.as_strided(img, (h, w * c), (pitch, 1), off)
        assert bool((got == one[0].reshape(h, w * c)).all()), f"expanded image {i} {sizes[i]}"
    del img, out
    torch.cuda.empty_cache()
