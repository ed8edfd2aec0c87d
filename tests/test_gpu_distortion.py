"""Squared error of stored tiles against their source (pxz_distortion_frames_device, pxz_distortion_varied_frames_device,
pxz_rate_distortion_image).  Every comparison is exact integer equality, and the expected value is always a numpy sum per
tile of (source - oracle.expand_image(...))^2 -- never anything the library computed.  The stored sizes of the first tests
are made by hand and the stored bytes are random (a tile stored at full size holds its source, see fill_clones), so the kernel
is exercised independently of any detector."""
import ctypes as C
import os

import numpy as np
import pytest
from PIL import Image

pytestmark = pytest.mark.gpu

POISON = 0xA5
POISON64 = 0x5A5A5A5A5A5A5A5A
FILTERS = (0, 1, 2, 3, 4)
INVALID_ARG, UNSUPPORTED = -1, -5
FULL, LOWER, NARROWER, BOTH, ONE = range(5)  # the five shapes a stored tile is given
# block_w, block_h, frame width, frame height, bytes added to a row, bytes before the first frame
GEOMS = [(32, 32, 100, 70, 8, 0),   # edge tiles 4x6
         (64, 64, 130, 65, 0, 0),   # edge 2x1
         (16, 16, 50, 33, 4, 0),
         (48, 20, 100, 37, 0, 0),
         (32, 32, 45, 40, 3, 1)]    # a pitch that is no multiple of 4 (RGBA 183, RGB 138) at an odd offset
KINDS = ("opaque", "alpha", "rgb")


@pytest.fixture(scope="module")
def gpu(product):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    h = product.Handle(0)
    yield h
    h.close()


# ---- inputs and the expected sums ---------------------------------------------------------------------------------------

def tile_rects(w, h, bw, bh):
    cols, rows = -(-w // bw), -(-h // bh)
    return [(tx * bw, ty * bh, min(bw, w - tx * bw), min(bh, h - ty * bh)) for ty in range(rows) for tx in range(cols)]


def smaller_not_pow2(n, third):
    """a size below n that is no power of two where n leaves room for one (n >= 4)"""
    m = n // 3 if third else 3 * n // 4
    while m > 2 and m & (m - 1) == 0:
        m -= 1
    return max(m, 1)


def shape_of(fw, fh, k, third=False):
    return [(fw, fh), (fw, max(fh // 2, 1)), (max(fw // 2, 1), fh), (smaller_not_pow2(fw, third), smaller_not_pow2(fh, third)), (1, 1)][k]


def class_of(fw, fh, tw, th):
    """what a stored size IS for its tile (a 64x1 tile cannot be stored lower, whatever it was dealt)"""
    if (tw, th) == (fw, fh):
        return FULL
    if (tw, th) == (1, 1):
        return ONE
    if tw == fw:
        return LOWER
    if th == fh:
        return NARROWER
    return BOTH if (tw & (tw - 1)) or (th & (th - 1)) else -1


def hand_sizes(rects_per_frame, n_frames):
    """the five shapes dealt in turn over the batch's tiles, largest tiles first, so that every shape meets a tile with room for it"""
    rects = rects_per_frame * n_frames
    order = sorted(range(len(rects)), key=lambda t: (-rects[t][2] * rects[t][3], t))
    tw, th = np.zeros(len(rects), np.uint32), np.zeros(len(rects), np.uint32)
    for rank, t in enumerate(order):
        tw[t], th[t] = shape_of(rects[t][2], rects[t][3], rank % 5, third=(rank // 5) % 2 == 1)
    return tw, th


def random_pixels(rng, shape, kind):
    px = rng.integers(0, 256, size=shape, dtype=np.uint8)
    if kind == "opaque":
        px[..., 3] = 255
    return px


def random_slots(rng, tw, th, slot_px, c, kind):
    slots = np.full((tw.size, slot_px * c), POISON, np.uint8)
    for t in range(tw.size):
        n = int(tw[t]) * int(th[t])
        slots[t, :n * c] = random_pixels(rng, (n, c), kind).reshape(-1)
    return slots


def fill_clones(slots, img, rects, tw, th):
    """A tile stored at its full size is the source itself (PixlzrBlock::resize clones it, block.rs:279-281, and no shrinker stores
    anything else at that size): such slots carry the source's pixels, so that the oracle's expand agrees with the definition the
    library uses -- the squared error of a clone is 0, and its slot is not read (test_clones_... hands garbage over for that)."""
    for t, (x, y, fw, fh) in enumerate(rects):
        if (int(tw[t]), int(th[t])) == (fw, fh):
            slots[t, :fw * fh * img.shape[2]] = img[y:y + fh, x:x + fw].reshape(-1)


def expected_tiles(oracle, src, bw, bh, filt, tw, th, slots):
    """numpy, per tile and channel: sum of (source - what the oracle expands)^2 of one image -> int64 [tiles, channels]"""
    h, w, c = src.shape
    exp = oracle.expand_image(w, h, bw, bh, c, filt, tw, th, slots)
    d = (src.astype(np.int64) - exp.astype(np.int64)) ** 2
    return np.array([d[y:y + fh, x:x + fw].sum(axis=(0, 1)) for (x, y, fw, fh) in tile_rects(w, h, bw, bh)], np.int64).reshape(-1, c)


def device_frames(imgs, pad, lead, gap=64):
    """host images of one size -> a CUDA view [N,H,W,C] with rows of W*C + pad bytes, a frame stride larger than a frame and the
    first frame `lead` bytes into its allocation"""
    import torch
    n = len(imgs)
    h, w, c = imgs[0].shape
    pitch = w * c + pad
    stride = pitch * h + gap + pad
    buf = np.full(lead + n * stride, POISON, np.uint8)
    for f, img in enumerate(imgs):
        np.lib.stride_tricks.as_strided(buf[lead + f * stride:], (h, w, c), (pitch, c, 1))[...] = img
    whole = torch.from_numpy(buf).cuda()
    return torch.as_strided(whole, (n, h, w, c), (stride, pitch, c, 1), lead)


class Case:
    """two frames of one geometry and pixel kind, hand-made stored sizes, random stored bytes; expected sums per filter, computed once"""

    def __init__(self, oracle, geom, kind, n_frames=2):
        import torch
        self.bw, self.bh, self.w, self.h, pad, lead = geom
        self.c = 3 if kind == "rgb" else 4
        self.kind, self.n = kind, n_frames
        if kind == "rgb":
            lead |= 1  # RGB frames start at an odd byte offset
        rng = np.random.default_rng(sum(geom) * 7 + KINDS.index(kind))
        self.rects = tile_rects(self.w, self.h, self.bw, self.bh)
        self.T = len(self.rects)
        self.imgs = [random_pixels(rng, (self.h, self.w, self.c), kind) for _ in range(n_frames)]
        self.tw, self.th = hand_sizes(self.rects, n_frames)
        self.slots = random_slots(rng, self.tw, self.th, self.bw * self.bh, self.c, kind)
        for f in range(n_frames):
            fill_clones(self.slots[f * self.T:(f + 1) * self.T], self.imgs[f], self.rects, self.tw[f * self.T:], self.th[f * self.T:])
        self.frames = device_frames(self.imgs, pad, lead)
        self.d_tw = torch.from_numpy(self.tw.astype(np.int32)).cuda().reshape(n_frames, self.T)
        self.d_th = torch.from_numpy(self.th.astype(np.int32)).cuda().reshape(n_frames, self.T)
        self.d_slots = torch.from_numpy(self.slots).cuda().reshape(n_frames, self.T, -1)
        self.oracle, self._expected = oracle, {}

    def classes(self):
        return [class_of(r[2], r[3], int(a), int(b)) for r, a, b in zip(self.rects * self.n, self.tw, self.th)]

    def expected(self, filt):
        """int64 [frames, tiles, channels]"""
        if filt not in self._expected:
            T = self.T
            self._expected[filt] = np.stack([expected_tiles(self.oracle, self.imgs[f], self.bw, self.bh, filt, self.tw[f * T:(f + 1) * T],
                                                            self.th[f * T:(f + 1) * T], self.slots[f * T:(f + 1) * T]) for f in range(self.n)])
        return self._expected[filt]


_cases = {}


def case_of(oracle, geom, kind):
    if (geom, kind) not in _cases:
        _cases[(geom, kind)] = Case(oracle, geom, kind)
    return _cases[(geom, kind)]


def poisoned_out(shape_tiles, shape_totals):
    import torch
    return (torch.full(shape_tiles, POISON64, dtype=torch.int64, device="cuda"), torch.full(shape_totals, POISON64, dtype=torch.int64, device="cuda"))


def run_frames(gpu, frames, bw, bh, filt, ow, oh, slots, want_tiles=True):
    """-> (tile sums | None, totals, pxz_decode_status) as host arrays, the outputs poisoned before the call"""
    import torch
    n, h, w, c = frames.shape
    T = -(-w // bw) * -(-h // bh)
    k = ow.numel() // (n * T)
    tiles, totals = poisoned_out((k, n, T, c), (k, n, c))
    gpu.distortion_frames_device(frames, bw, bh, filt, ow, oh, slots, out=(tiles if want_tiles else None, totals))
    status = gpu.decode_status()
    torch.cuda.synchronize()
    return (tiles.cpu().numpy() if want_tiles else None), totals.cpu().numpy(), status


# ---- every class of tile ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: f"{g[0]}x{g[1]}-{g[2]}x{g[3]}")
def test_hand_made_sizes_equal_the_oracle(gpu, oracle, geom, kind):
    """all five up-scaling filters; two frames, frame stride larger than a frame, RGB at an odd offset"""
    case = case_of(oracle, geom, kind)
    got_classes = set(case.classes())
    assert {FULL, LOWER, NARROWER, BOTH, ONE} <= got_classes, f"classes met: {sorted(got_classes)}"  # a condition, not a measurement
    assert case.frames.stride(0) > case.frames.stride(1) * case.h
    if kind == "rgb":
        assert case.frames.data_ptr() % 2 == 1
    if geom[4] == 3:
        assert case.frames.stride(1) % 4 != 0
    for filt in FILTERS:
        tiles, totals, status = run_frames(gpu, case.frames, case.bw, case.bh, filt, case.d_tw, case.d_th, case.d_slots)
        exp = case.expected(filt)
        print(f"{geom} {kind} filter {filt}: {int((tiles[0] != exp).any(axis=2).sum())} of {exp.shape[0] * exp.shape[1]} tiles differ, "
              f"totals {totals[0].tolist()} expected {exp.sum(axis=1).tolist()}")
        assert status == 0
        assert (tiles[0] == exp).all(), f"filter {filt}: tiles {np.argwhere((tiles[0] != exp).any(axis=2)).tolist()} differ"
        assert (totals[0] == exp.sum(axis=1)).all(), f"filter {filt}: totals"


def test_totals_are_the_sums_of_the_tiles_with_and_without_tile_output(gpu, oracle):
    for geom, kind in ((GEOMS[0], "alpha"), (GEOMS[4], "rgb")):
        case = case_of(oracle, geom, kind)
        tiles, totals, _ = run_frames(gpu, case.frames, case.bw, case.bh, 4, case.d_tw, case.d_th, case.d_slots)
        _, alone, status = run_frames(gpu, case.frames, case.bw, case.bh, 4, case.d_tw, case.d_th, case.d_slots, want_tiles=False)
        assert status == 0
        assert (totals == tiles.sum(axis=2)).all()
        assert (alone == totals).all() and (alone[0] == case.expected(4).sum(axis=1)).all()


@pytest.mark.parametrize("c", [4, 3])
def test_clones_are_zero_and_their_slots_are_not_needed(gpu, oracle, c):
    """every tile stored at its full size: the slots are handed over as garbage"""
    import torch
    bw, bh, w, h = 32, 32, 100, 70
    rng = np.random.default_rng(5 + c)
    imgs = [rng.integers(0, 256, size=(h, w, c), dtype=np.uint8) for _ in range(2)]
    frames = device_frames(imgs, 5, 1)
    rects = tile_rects(w, h, bw, bh)
    ow = torch.tensor([[r[2] for r in rects]] * 2, dtype=torch.int32, device="cuda")
    oh = torch.tensor([[r[3] for r in rects]] * 2, dtype=torch.int32, device="cuda")
    slots = torch.from_numpy(rng.integers(0, 256, size=(2, len(rects), bw * bh * c), dtype=np.uint8)).cuda()
    for filt in (0, 4):
        tiles, totals, status = run_frames(gpu, frames, bw, bh, filt, ow, oh, slots)
        assert status == 0 and (tiles == 0).all() and (totals == 0).all()


# ---- sets -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode,factors", [(1, [16.0, 4.0, 64.0]), (0, [0.5, 0.125, 2.0])], ids=["directional", "shrink_by"])
def test_three_rungs_in_one_call_equal_three_calls_and_the_oracle(gpu, oracle, mode, factors):
    import torch
    bw = bh = 32
    w, h, c, n = 128, 96, 4, 2
    imgs = [oracle.synth_frame(w, h, c, 3 + f, 0) for f in range(n)]
    frames = torch.from_numpy(np.stack(imgs)).cuda()
    vals, ow, oh, slots = gpu.shrink_ladder_frames_device(frames, bw, bh, mode, 4, factors)
    torch.cuda.synchronize()
    hw, hh, hs = ow.cpu().numpy().astype(np.uint32), oh.cpu().numpy().astype(np.uint32), slots.cpu().numpy()
    assert len({(int(a), int(b)) for a, b in zip(hw.ravel(), hh.ravel())}) >= 3  # the rungs differ
    for filt in (0, 4):
        tiles, totals, status = run_frames(gpu, frames, bw, bh, filt, ow, oh, slots)
        assert status == 0 and tiles.shape == (3, n, 12, c)
        for r in range(3):
            one, one_totals, _ = run_frames(gpu, frames, bw, bh, filt, ow[r], oh[r], slots[r])
            assert (tiles[r] == one[0]).all() and (totals[r] == one_totals[0]).all(), f"mode {mode} filter {filt} rung {r} vs n_sets = 1"
            for f in range(n):
                exp = expected_tiles(oracle, imgs[f], bw, bh, filt, hw[r, f], hh[r, f], hs[r, f])
                assert (tiles[r, f] == exp).all(), f"mode {mode} filter {filt} rung {r} frame {f} vs oracle"
                assert (totals[r, f] == exp.sum(axis=0)).all()


def test_windows_kept_across_sets_that_repeat_a_stored_size(gpu, oracle):
    """three hand-made sets: every tile stored smaller on both axes, then at full size (a clone set in between), then with the first
    set's width and another height (even tiles) or the first set's height and another width (odd tiles): the axis whose stored
    size repeats reuses the windows staged two sets earlier, the other is staged again"""
    import torch
    bw, bh, w, h, c, n = 48, 20, 100, 37, 4, 2
    rng = np.random.default_rng(77)
    rects = tile_rects(w, h, bw, bh)
    T = len(rects)
    imgs = [random_pixels(rng, (h, w, c), "alpha") for _ in range(n)]
    first = [shape_of(r[2], r[3], BOTH, third=t % 2 == 1) for t, r in enumerate(rects)]
    third = [(a, max(b // 2, 1)) if t % 2 == 0 else (max(a // 2, 1), b) for t, (a, b) in enumerate(first)]
    sets = [first, [(r[2], r[3]) for r in rects], third]
    tw = np.array([[[s[t][0] for t in range(T)]] * n for s in sets], np.uint32)  # [3, n, T]
    th = np.array([[[s[t][1] for t in range(T)]] * n for s in sets], np.uint32)
    same_w = [t for t, r in enumerate(rects) if first[t][0] == third[t][0] < r[2] and first[t][1] != third[t][1]]
    same_h = [t for t, r in enumerate(rects) if first[t][1] == third[t][1] < r[3] and first[t][0] != third[t][0]]
    assert same_w and same_h, "no tile repeats a stored width / height across two sets that are not clones"  # a condition
    slots = np.stack([np.stack([random_slots(rng, tw[k, f], th[k, f], bw * bh, c, "alpha") for f in range(n)]) for k in range(3)])
    for f in range(n):
        fill_clones(slots[1, f], imgs[f], rects, tw[1, f], th[1, f])
    frames = device_frames(imgs, 3, 1)
    dev = [torch.from_numpy(a).cuda() for a in (tw.astype(np.int32), th.astype(np.int32), slots)]
    for filt in FILTERS:
        tiles, totals, status = run_frames(gpu, frames, bw, bh, filt, *dev)
        assert status == 0 and (tiles[1] == 0).all()
        for k in range(3):
            for f in range(n):
                exp = expected_tiles(oracle, imgs[f], bw, bh, filt, tw[k, f], th[k, f], slots[k, f])
                assert (tiles[k, f] == exp).all(), f"filter {filt} set {k} frame {f}: tiles {np.argwhere((tiles[k, f] != exp).any(axis=1)).ravel().tolist()}"
                assert (totals[k, f] == exp.sum(axis=0)).all()


# ---- varied -------------------------------------------------------------------------------------------------------------

VARIED_SIZES = [(1, 1), (31, 33), (97, 61), (33, 2), (64, 32)]


def odd_layout(sizes, c):
    """descriptors of images at odd offsets with padded rows in one buffer -> (descs, bytes)"""
    descs, at = [], 1
    for k, (w, h) in enumerate(sizes):
        pitch = w * c + 3 * (k % 3)
        descs.append((w, h, pitch, at))
        at += pitch * h + 1 + 2 * (k % 2)
    return descs, at


def varied_batch(rng, sizes, bw, bh, c, kind):
    """images at odd offsets with padded rows in one buffer, hand-made stored sizes, random stored bytes"""
    import torch
    descs, at = odd_layout(sizes, c)
    buf = np.full(at, POISON, np.uint8)
    imgs, tws, ths, slots = [], [], [], []
    for (w, h, pitch, off) in descs:
        img = random_pixels(rng, (h, w, c), kind)
        np.lib.stride_tricks.as_strided(buf[off:], (h, w, c), (pitch, c, 1))[...] = img
        tw, th = hand_sizes(tile_rects(w, h, bw, bh), 1)
        sl = random_slots(rng, tw, th, bw * bh, c, kind)
        fill_clones(sl, img, tile_rects(w, h, bw, bh), tw, th)
        imgs.append(img), tws.append(tw), ths.append(th), slots.append(sl)
    dev = (torch.from_numpy(buf).cuda(), torch.from_numpy(np.concatenate(tws).astype(np.int32)).cuda(),
           torch.from_numpy(np.concatenate(ths).astype(np.int32)).cuda(), torch.from_numpy(np.concatenate(slots)).cuda())
    return descs, imgs, tws, ths, slots, dev


def run_varied(gpu, descs, c, bw, bh, filt, dev, want_tiles=True):
    import torch
    buf, ow, oh, slots = dev
    tiles, totals = poisoned_out((ow.numel(), c), (len(descs), c))
    flags = torch.full((len(descs),), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    gpu.distortion_varied_frames_device(buf, bw, bh, filt, ow, oh, slots, descs=descs, channels=c,
                                        out=(tiles if want_tiles else None, totals), image_flags=flags)
    status = gpu.decode_status()
    torch.cuda.synchronize()
    return (tiles.cpu().numpy() if want_tiles else None), totals.cpu().numpy(), flags.cpu().numpy(), status


@pytest.mark.parametrize("c,kind", [(4, "alpha"), (3, "rgb")])
def test_five_images_in_one_call_equal_the_frames_call_and_the_oracle(gpu, product, oracle, c, kind):
    import torch
    bw = bh = 32
    rng = np.random.default_rng(40 + c)
    descs, imgs, tws, ths, slots, dev = varied_batch(rng, VARIED_SIZES, bw, bh, c, kind)
    assert (1, 1) in VARIED_SIZES and (97, 61) in VARIED_SIZES
    to = product.varied_layout(descs, bw, bh)
    for filt in FILTERS:
        tiles, totals, flags, status = run_varied(gpu, descs, c, bw, bh, filt, dev)
        assert status == 0 and (flags == 0).all()
        for i, img in enumerate(imgs):
            a, b = int(to[i]), int(to[i + 1])
            exp = expected_tiles(oracle, img, bw, bh, filt, tws[i], ths[i], slots[i])
            assert (tiles[a:b] == exp).all(), f"C{c} filter {filt} image {i} {VARIED_SIZES[i]} vs oracle"
            assert (totals[i] == exp.sum(axis=0)).all()
            if filt in (0, 4):
                one, one_totals, st = run_frames(gpu, torch.from_numpy(img[None]).cuda(), bw, bh, filt, dev[1][a:b][None].contiguous(),
                                                 dev[2][a:b][None].contiguous(), dev[3][a:b][None].contiguous())
                assert st == 0 and (one[0, 0] == tiles[a:b]).all() and (one_totals[0, 0] == totals[i]).all(), f"image {i} vs the frames call"
    _, alone, _, _ = run_varied(gpu, descs, c, bw, bh, 4, dev, want_tiles=False)
    assert (alone == totals).all()


@pytest.mark.parametrize("c", [3, 4])
def test_2049_images_equal_the_oracle(gpu, product, oracle, c):
    """the batch of tests/test_gpu_varied_decode.py that has more images than a block keeps first tiles of in LDS: per tile and per
    image against the oracle's expand of every image"""
    import torch
    from test_gpu_varied_decode import MANY, many_images
    m = many_images(oracle, c)
    descs, at = odd_layout(m.sizes, c)
    buf = np.full(at, POISON, np.uint8)
    for (w, h, pitch, off), img in zip(descs, m.images):
        np.lib.stride_tricks.as_strided(buf[off:], (h, w, c), (pitch, c, 1))[...] = img
    dev = (torch.from_numpy(buf).cuda(), torch.from_numpy(m.flat[1].astype(np.int32)).cuda(), torch.from_numpy(m.flat[2].astype(np.int32)).cuda(),
           torch.from_numpy(m.flat[3]).cuda())
    to = product.varied_layout(descs, 4, 4)
    assert int(to[-1]) == m.flat[1].size
    for filt in (0, 4):
        tiles, totals, flags, status = run_varied(gpu, descs, c, 4, 4, filt, dev)
        assert status == 0 and (flags == 0).all()
        exp_tiles, exp_totals = [], []
        for img, exp in zip(m.images, m.expected(filt)):
            d = (img.astype(np.int64) - exp.astype(np.int64)) ** 2
            per_tile = np.array([d[y:y + fh, x:x + fw].sum(axis=(0, 1)) for (x, y, fw, fh) in tile_rects(img.shape[1], img.shape[0], 4, 4)], np.int64)
            exp_tiles.append(per_tile.reshape(-1, c)), exp_totals.append(per_tile.reshape(-1, c).sum(axis=0))
        exp_tiles, exp_totals = np.concatenate(exp_tiles), np.stack(exp_totals)
        print(f"C{c} filter {filt}: {int((tiles != exp_tiles).any(axis=1).sum())} of {exp_tiles.shape[0]} tiles, "
              f"{int((totals != exp_totals).any(axis=1).sum())} of {MANY} images differ")
        assert exp_tiles.any() and not exp_tiles.all(axis=1).all()  # (clones and stored tiles both)
        assert (tiles == exp_tiles).all(), f"C{c} filter {filt}: tiles {np.flatnonzero((tiles != exp_tiles).any(axis=1))[:10].tolist()}"
        assert (totals == exp_totals).all(), f"C{c} filter {filt}: images {np.flatnonzero((totals != exp_totals).any(axis=1))[:10].tolist()}"


# ---- invalid stored sizes -------------------------------------------------------------------------------------------------

def test_invalid_stored_sizes_are_marked_and_left_out(gpu, product, oracle):
    """one tile with stored width 0, one with a stored height above its place: all-ones entries, status bit 0, the image's flag in
    the varied form, totals of the remaining tiles, every other tile exact"""
    import torch
    case = case_of(oracle, GEOMS[0], "alpha")
    T, c = case.T, case.c
    zero_w, tall = 1, T + T - 1  # frame 0's second tile; frame 1's corner tile (4x6)
    ow, oh = case.d_tw.clone(), case.d_th.clone()
    ow.view(-1)[zero_w] = 0
    oh.view(-1)[tall] = case.rects[T - 1][3] + 1
    tiles, totals, status = run_frames(gpu, case.frames, case.bw, case.bh, 4, ow, oh, case.d_slots)
    exp = case.expected(4).reshape(-1, c).copy()
    bad = np.zeros(2 * T, bool)
    bad[[zero_w, tall]] = True
    flat = tiles[0].reshape(-1, c)
    assert status & 1
    assert (flat[bad] == -1).all()  # UINT64_MAX
    assert (flat[~bad] == exp[~bad]).all()
    exp[bad] = 0
    assert (totals[0] == exp.reshape(2, T, c).sum(axis=1)).all()
    # a clean call afterwards clears the status
    assert run_frames(gpu, case.frames, case.bw, case.bh, 4, case.d_tw, case.d_th, case.d_slots)[2] == 0

    bw = bh = 32
    rng = np.random.default_rng(41)
    descs, imgs, tws, ths, slots, dev = varied_batch(rng, VARIED_SIZES, bw, bh, 4, "opaque")
    to = product.varied_layout(descs, bw, bh)
    k = VARIED_SIZES.index((97, 61))
    ow, oh = dev[1].clone(), dev[2].clone()
    ow[int(to[k]) + 2] = 0
    oh[int(to[k + 1]) - 1] = 61 - 32 + 1
    tiles, totals, flags, status = run_varied(gpu, descs, 4, bw, bh, 2, (dev[0], ow, oh, dev[3]))
    assert status & 1 and flags.tolist() == [1 if i == k else 0 for i in range(len(descs))]
    for i, img in enumerate(imgs):
        a, b = int(to[i]), int(to[i + 1])
        exp = expected_tiles(oracle, img, bw, bh, 2, tws[i], ths[i], slots[i])
        if i == k:
            bad = np.zeros(b - a, bool)
            bad[[2, b - a - 1]] = True
            assert (tiles[a:b][bad] == -1).all() and (tiles[a:b][~bad] == exp[~bad]).all()
            exp[bad] = 0
        else:
            assert (tiles[a:b] == exp).all()
        assert (totals[i] == exp.sum(axis=0)).all()


# ---- errors ---------------------------------------------------------------------------------------------------------------

def test_errors_write_nothing(gpu, product, oracle):
    import torch
    L = product.binding.load_library()
    F, P, descs_of = product.binding.Frames, product.binding.Params, product.binding.image_descs
    case = case_of(oracle, GEOMS[0], "alpha")
    n, T, c, w, h = case.n, case.T, case.c, case.w, case.h
    fr = case.frames
    good_f = F(w, h, c, fr.stride(1), n, 0, fr.stride(0))
    good_p = P(case.bw, case.bh, 0, 4, 0.0, 0)
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    def call_frames(f, p, n_sets, pixels=True, tw=True, th=True, slots=True, totals=True):
        tiles, tot = poisoned_out((1, n, T, c), (1, n, c))
        rc = L.pxz_distortion_frames_device(gpu._h, C.byref(f) if f is not None else None, C.byref(p) if p is not None else None, n_sets,
                                            ptr(fr) if pixels else None, ptr(case.d_tw) if tw else None, ptr(case.d_th) if th else None,
                                            ptr(case.d_slots) if slots else None, ptr(tiles), ptr(tot) if totals else None)
        torch.cuda.synchronize()
        assert (tiles == POISON64).all() and (tot == POISON64).all(), "an error case wrote its outputs"
        return rc

    assert call_frames(None, good_p, 1) == INVALID_ARG
    assert call_frames(good_f, None, 1) == INVALID_ARG
    assert call_frames(good_f, good_p, 0) == INVALID_ARG
    for missing in ("pixels", "tw", "th", "slots", "totals"):
        assert call_frames(good_f, good_p, 1, **{missing: False}) == INVALID_ARG, missing
    assert call_frames(good_f, P(case.bw, case.bh, 0, 5, 0.0, 0), 1) == INVALID_ARG            # a bad filter
    assert call_frames(F(w, h, c, w * c - 1, n, 0, fr.stride(0)), good_p, 1) == INVALID_ARG   # a pitch below one row
    assert call_frames(F(w, h, 5, fr.stride(1), n, 0, fr.stride(0)), good_p, 1) == INVALID_ARG
    assert call_frames(good_f, P(0, case.bh, 0, 4, 0.0, 0), 1) == INVALID_ARG
    assert call_frames(good_f, P(200, 200, 0, 4, 0.0, 0), 1) == UNSUPPORTED                    # a 200x200 RGBA block
    assert call_frames(F(w, h, 3, fr.stride(1), n, 0, fr.stride(0)), P(144, 144, 0, 4, 0.0, 0), 1) == UNSUPPORTED  # RGB: slot fits, LDS not

    bw = bh = 32
    descs, imgs, tws, ths, slots, dev = varied_batch(np.random.default_rng(42), VARIED_SIZES, bw, bh, 4, "opaque")
    ok = P(bw, bh, 0, 4, 0.0, 0)

    def call_varied(geoms, count, channels, p, base=True, slots_given=True, totals=True):
        tiles, tot = poisoned_out((dev[1].numel(), 4), (len(descs), 4))
        flags = torch.full((len(descs),), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        rc = L.pxz_distortion_varied_frames_device(gpu._h, C.cast(descs_of(geoms), C.c_void_p) if geoms is not None else None, count, channels,
                                                   C.byref(p) if p is not None else None, ptr(dev[0]) if base else None, ptr(dev[1]), ptr(dev[2]),
                                                   ptr(dev[3]) if slots_given else None, ptr(tiles), ptr(tot) if totals else None, ptr(flags))
        torch.cuda.synchronize()
        assert (tiles == POISON64).all() and (tot == POISON64).all() and (flags == 0x5A5A5A5A).all(), "an error case wrote its outputs"
        return rc

    assert call_varied(descs, 5, 4, None) == INVALID_ARG
    assert call_varied(None, 5, 4, ok) == INVALID_ARG
    assert call_varied(descs, 0, 4, ok) == INVALID_ARG
    assert call_varied(descs, 5, 2, ok) == INVALID_ARG
    assert call_varied(descs, 5, 4, ok, base=False) == INVALID_ARG
    assert call_varied(descs, 5, 4, ok, slots_given=False) == INVALID_ARG
    assert call_varied(descs, 5, 4, ok, totals=False) == INVALID_ARG
    assert call_varied(descs, 5, 4, P(bw, bh, 0, 7, 0.0, 0)) == INVALID_ARG
    short = list(descs)
    short[2] = (descs[2][0], descs[2][1], descs[2][0] * 4 - 1, descs[2][3])
    assert call_varied(short, 5, 4, ok) == INVALID_ARG and "image 2" in L.pxz_last_error(gpu._h).decode()
    assert call_varied(descs, 5, 4, P(200, 200, 0, 4, 0.0, 0)) == UNSUPPORTED


# ---- the host call ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,block,crop", [("image.png", 64, None), ("base.png", 32, (200, 150))])
@pytest.mark.parametrize("mode,factors", [(1, [64.0, 16.0, 4.0, 1.0]), (0, [2.0, 0.5, 0.125, 0.03])], ids=["directional", "shrink_by"])
def test_rate_distortion_image_equals_the_oracle(gpu, product, oracle, golden_dir, name, block, crop, mode, factors):
    img = np.asarray(Image.open(os.path.join(golden_dir, name)))
    if crop:
        img = img[:crop[1], :crop[0]]
    img = np.ascontiguousarray(img)
    h, w, c = img.shape
    down, up = 4, 2
    file_bytes, sse = gpu.rate_distortion_image(img, block, block, mode, down, up, factors)
    assert file_bytes.shape == (4,) and sse.shape == (4, c)
    for r, k in enumerate(factors):
        ev, ew, eh, es = oracle.shrink_image(img, block, block, mode, down, k, nthreads=8)
        raw = oracle.encode_container(w, h, block, block, c, 0, ev, None, ew, eh, es)
        exp = expected_tiles(oracle, img, block, block, up, ew, eh, es).sum(axis=0)
        print(f"{name} mode {mode} k={k}: {int(file_bytes[r])} bytes (oracle {len(raw)}), sse {sse[r].tolist()} (oracle {exp.tolist()}), "
              f"PSNR {product.psnr(int(sse[r].sum()), h * w * c):.2f} dB")
        assert int(file_bytes[r]) == len(raw), f"factor {k}: file length"
        assert (sse[r].astype(np.int64) == exp).all(), f"factor {k}: squared error"
    assert len(set(file_bytes.tolist())) >= 2  # the factors spread the files
