"""Distortion of re-shrunk tiles against the archive's own (pxz_reshrink_distortion_varied_device, pxz_rate_distortion_varied_files,
pxz_transcode_varied_files_fit).  Every comparison is exact integer equality.  The expected value always comes from the oracle on
the CPU: oracle.expand_image of the reference tiles with expand_filter, oracle.expand_image of each set with filter_up, and the
squared differences summed per tile in numpy int64 -- never anything the library computed.  A set tile stored at its full size
is the reference by definition (sums 0, its slot is not read), so such slots hold garbage here.  The stored sizes of the first
tests are made by hand and the stored bytes are random, so the kernel is exercised independently of any detector.  Outputs are
poisoned before every call."""
import ctypes as C
import os

import numpy as np
import pytest
from PIL import Image

from test_fit_host import FIT_BYTES, FIT_SSE, U64, select
from test_gpu_distortion import BOTH, FULL, LOWER, NARROWER, ONE, POISON, POISON64, class_of, random_pixels, random_slots, shape_of, tile_rects

pytestmark = pytest.mark.gpu

INVALID_ARG, UNSUPPORTED, BUFFER_TOO_SMALL = -1, -5, -7
POISON32 = 0x5A5A5A5A
LDS_PER_CU = 160 * 1024


@pytest.fixture(scope="module")
def gpu(product):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    h = product.Handle(0)
    yield h
    h.close()


def last_error(gpu):
    return (gpu._L.pxz_last_error(gpu._h) or b"").decode()


# ---- inputs and the expected sums ---------------------------------------------------------------------------------------

def dealt_sizes(rects, shift):
    """the five shapes of tests/test_gpu_distortion.py dealt in turn over the tiles, largest tiles first, starting at `shift`"""
    order = sorted(range(len(rects)), key=lambda t: (-rects[t][2] * rects[t][3], t))
    tw, th = np.zeros(len(rects), np.uint32), np.zeros(len(rects), np.uint32)
    for rank, t in enumerate(order):
        k = rank + shift
        tw[t], th[t] = shape_of(rects[t][2], rects[t][3], k % 5, third=(k // 5) % 2 == 1)
    return tw, th


def tile_sums(d, w, h, bw, bh):
    """d [h, w, c] -> per tile and channel its sum, int64 [tiles, c]"""
    return np.array([d[y:y + fh, x:x + fw].sum(axis=(0, 1)) for (x, y, fw, fh) in tile_rects(w, h, bw, bh)], np.int64).reshape(-1, d.shape[2])


class Batch:
    """images of the given sizes (no pixels: the archive is all there is), the archive's stored tiles and n_sets stored versions of
    them: sizes by hand, bytes random.  shifts: where each set starts dealing its shapes (the reference starts at 1)."""

    def __init__(self, oracle, sizes, bw, bh, kind, shifts, seed=0, sets=None, ref=None):
        import torch
        self.oracle, self.sizes, self.bw, self.bh, self.kind = oracle, sizes, bw, bh, kind
        self.c = c = 3 if kind == "rgb" else 4
        rng = np.random.default_rng(seed + bw * 1000 + bh * 10 + c)
        self.per_image = [tile_rects(w, h, bw, bh) for (w, h) in sizes]
        self.rects = [r for rects in self.per_image for r in rects]
        self.to = np.concatenate([[0], np.cumsum([len(r) for r in self.per_image])])
        self.T, self.n, slot_px = len(self.rects), len(sizes), bw * bh
        self.fw = np.array([r[2] for r in self.rects], np.uint32)
        self.fh = np.array([r[3] for r in self.rects], np.uint32)
        self.rtw, self.rth = ref if ref is not None else dealt_sizes(self.rects, 1)
        self.rslots = random_slots(rng, self.rtw, self.rth, slot_px, c, kind)
        sets = sets if sets is not None else [dealt_sizes(self.rects, s) for s in shifts]
        self.K = len(sets)
        self.tw = np.stack([s[0] for s in sets]).astype(np.uint32)
        self.th = np.stack([s[1] for s in sets]).astype(np.uint32)
        self.slots = np.stack([random_slots(rng, self.tw[k], self.th[k], slot_px, c, kind) for k in range(self.K)])
        self.clone = (self.tw == self.fw[None]) & (self.th == self.fh[None])
        # a clone's slot is not read: bytes that would show
        self.slots[self.clone] = rng.integers(0, 256, (int(self.clone.sum()), slot_px * c), dtype=np.uint8)
        i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a).astype(np.int32)).cuda()  # noqa: E731
        self.dev_ref = (i32(self.rtw), i32(self.rth), torch.from_numpy(self.rslots).cuda())
        self.dev_sets = (i32(self.tw), i32(self.th), torch.from_numpy(self.slots).cuda())
        self._ref, self._expected = {}, {}

    def ref_images(self, xf):
        if xf not in self._ref:
            self._ref[xf] = [self.oracle.expand_image(w, h, self.bw, self.bh, self.c, xf, self.rtw[a:b], self.rth[a:b], self.rslots[a:b])
                             for (w, h), a, b in zip(self.sizes, self.to[:-1], self.to[1:])]
        return self._ref[xf]

    def expected(self, xf, uf):
        """int64 [K, T, c]: computed once per pair of filters and left unchanged"""
        if (xf, uf) not in self._expected:
            out = np.zeros((self.K, self.T, self.c), np.int64)
            for k in range(self.K):
                for (w, h), a, b, ref in zip(self.sizes, self.to[:-1], self.to[1:], self.ref_images(xf)):
                    img = self.oracle.expand_image(w, h, self.bw, self.bh, self.c, uf, self.tw[k, a:b], self.th[k, a:b], self.slots[k, a:b])
                    out[k, a:b] = tile_sums((ref.astype(np.int64) - img.astype(np.int64)) ** 2, w, h, self.bw, self.bh)
            out[self.clone] = 0
            self._expected[(xf, uf)] = out
        return self._expected[(xf, uf)]

    def totals(self, tiles):
        """[K, T, c] -> [K, n, c]"""
        return np.stack([tiles[:, a:b].sum(axis=1) for a, b in zip(self.to[:-1], self.to[1:])], axis=1)


def run(gpu, b, xf, uf, want_tiles=True, ref=None, sets=None, sizes=None):
    """one call into poisoned outputs -> (tile sums | None, totals, flags, pxz_decode_status) on the host"""
    import torch
    ref, sets = ref or b.dev_ref, sets or b.dev_sets
    K = sets[0].shape[0]
    tiles = torch.full((K, b.T, b.c), POISON64, dtype=torch.int64, device="cuda")
    totals = torch.full((K, b.n, b.c), POISON64, dtype=torch.int64, device="cuda")
    flags = torch.full((b.n,), POISON32, dtype=torch.int32, device="cuda")
    gpu.reshrink_distortion_varied_device(sizes or b.sizes, b.c, b.bw, b.bh, xf, uf, *ref, *sets, out=(tiles if want_tiles else None, totals),
                                          image_flags=flags)
    status = gpu.decode_status()
    torch.cuda.synchronize()
    if not want_tiles:
        assert bool((tiles == POISON64).all()), "tile sums were written by a call that was given none"
    return (tiles.cpu().numpy() if want_tiles else None), totals.cpu().numpy(), flags.cpu().numpy(), status


def check(gpu, b, xf, uf, what):
    tiles, totals, flags, status = run(gpu, b, xf, uf)
    exp = b.expected(xf, uf)
    print(f"{what} filters {xf}/{uf}: {int((tiles != exp).any(axis=2).sum())} of {exp.shape[0] * exp.shape[1]} entries differ")
    assert status == 0 and (flags == 0).all(), (what, status, flags)
    assert (tiles == exp).all(), f"{what} filters {xf}/{uf}: entries {np.argwhere((tiles != exp).any(axis=2))[:10].tolist()} differ"
    assert (totals == b.totals(exp)).all(), f"{what} filters {xf}/{uf}: totals"
    return tiles, totals


# ---- 1. hand-made stored sizes of every class ---------------------------------------------------------------------------

# block, image sizes, pixel kinds, whether the geometry has room for every class of stored size
HAND = [((32, 32), [(100, 70)], ("opaque", "alpha", "rgb"), True),                # edge tiles 4x6
        ((16, 16), [(50, 33), (9, 5), (83, 61)], ("alpha", "rgb"), True),         # ragged sizes, an image below a block
        ((64, 64), [(130, 65), (70, 131)], ("opaque", "alpha", "rgb"), True),     # edge tiles 2x1 and 6x3
        ((37, 61), [(100, 70), (20, 40), (113, 125)], ("rgb",), True),
        ((5, 3), [(23, 11), (7, 5), (4, 2), (18, 14)], ("rgb",), False),          # 45-byte slots: the sets on every alignment
        ((32, 32), [(1, 1), (1, 40)], ("alpha", "rgb"), False)]                   # a 1x1 image and a 1-px-wide image
HAND_CASES = [(block, sizes, kind, room) for (block, sizes, kinds, room) in HAND for kind in kinds]
_batches = {}


def hand_batch(oracle, block, sizes, kind):
    key = (block, tuple(sizes), kind)
    if key not in _batches:
        _batches[key] = Batch(oracle, sizes, block[0], block[1], kind, shifts=(0, 2, 3))
    return _batches[key]


@pytest.mark.parametrize("block,sizes,kind,room", HAND_CASES, ids=[f"{b[0]}x{b[1]}-{s[0][0]}x{s[0][1]}-{k}" for (b, s, k, _) in HAND_CASES])
def test_hand_made_sizes_equal_the_oracle(gpu, oracle, block, sizes, kind, room):
    """three sets whose classes are dealt independently of the reference's; Lanczos3 / CatmullRom, and Nearest against Lanczos3"""
    b = hand_batch(oracle, block, sizes, kind)
    if room:
        every = {FULL, LOWER, NARROWER, BOTH, ONE}
        ref_classes = {class_of(int(fw), int(fh), int(a), int(c)) for fw, fh, a, c in zip(b.fw, b.fh, b.rtw, b.rth)}
        assert every <= ref_classes, f"reference classes met: {sorted(ref_classes)}"  # a condition, not a measurement
        pairs = {(class_of(int(fw), int(fh), int(ra), int(rb)), class_of(int(fw), int(fh), int(sa), int(sb)))
                 for k in range(b.K) for fw, fh, ra, rb, sa, sb in zip(b.fw, b.fh, b.rtw, b.rth, b.tw[k], b.th[k])}
        assert every <= {p[1] for p in pairs} and len(pairs) >= 12, f"(reference, set) classes met: {sorted(pairs)}"
    if block == (5, 3):
        assert b.slots.shape[2] == 45 and b.T >= 16  # set s of tile t starts at byte 45 * (s * T + t): every residue mod 16
    for (xf, uf) in [(4, 2), (0, 4)]:
        check(gpu, b, xf, uf, f"{block} {sizes} {kind}")


def test_all_25_filter_pairs(gpu, oracle):
    b = hand_batch(oracle, (16, 16), [(50, 33), (9, 5), (83, 61)], "alpha")
    for xf in range(5):
        for uf in range(5):
            check(gpu, b, xf, uf, "16x16 alpha")


@pytest.mark.parametrize("kind", ["alpha", "rgb"])
def test_the_call_is_expand_then_distortion_bit_for_bit(gpu, oracle, kind):
    """the device composition that defines the call: pxz_expand_varied_frames_device of the archive into a packed image, then
    pxz_distortion_varied_frames_device of every set against it"""
    import torch
    b = hand_batch(oracle, (32, 32), [(100, 70)], kind)
    descs, at = [], 0
    for (w, h) in b.sizes:
        descs.append((w, h, w * b.c, at))
        at += w * h * b.c
    for (xf, uf) in [(4, 2), (1, 0), (3, 3)]:
        image = torch.zeros(at, dtype=torch.uint8, device="cuda")
        gpu.expand_varied_frames_device(descs, b.c, b.bw, b.bh, xf, *b.dev_ref, image)
        tiles, totals, _, status = run(gpu, b, xf, uf)
        assert status == 0
        for k in range(b.K):
            t, tot = gpu.distortion_varied_frames_device(image, b.bw, b.bh, uf, b.dev_sets[0][k], b.dev_sets[1][k], b.dev_sets[2][k], descs=descs,
                                                         channels=b.c)
            torch.cuda.synchronize()
            assert (t.cpu().numpy() == tiles[k]).all() and (tot.cpu().numpy() == totals[k]).all(), f"{kind} filters {xf}/{uf} set {k}"
        assert (tiles == b.expected(xf, uf)).all()


# ---- 2. set counts ------------------------------------------------------------------------------------------------------

def repeating_sets(rects, count):
    """`count` sets over the tiles: every tile smaller on both axes, then at full size (a clone set in between), then with the first
    set's width and another height (even tiles) or the first set's height and another width (odd tiles), and so on in turn: the
    axis whose stored size repeats reuses the windows staged two sets earlier, the other is staged again"""
    first = [shape_of(r[2], r[3], BOTH, third=t % 2 == 1) for t, r in enumerate(rects)]
    third = [(a, max(c // 2, 1)) if t % 2 == 0 else (max(a // 2, 1), c) for t, (a, c) in enumerate(first)]
    kinds = [first, [(r[2], r[3]) for r in rects], third]
    return [(np.array([s[0] for s in kinds[k % 3]], np.uint32), np.array([s[1] for s in kinds[k % 3]], np.uint32)) for k in range(count)]


@pytest.mark.parametrize("count", [1, 3, 32])
def test_set_counts_kept_windows_and_totals(gpu, oracle, count):
    sizes = [(100, 70), (45, 40)] if count < 32 else [(70, 40)]
    bw, bh = (48, 20) if count == 3 else (32, 32)
    rects = [r for (w, h) in sizes for r in tile_rects(w, h, bw, bh)]
    b = Batch(oracle, sizes, bw, bh, "alpha", None, seed=count, sets=repeating_sets(rects, count))
    assert b.K == count
    if count >= 3:
        same_w = [t for t in range(b.T) if b.tw[0, t] == b.tw[2, t] < b.fw[t] and b.th[0, t] != b.th[2, t]]
        same_h = [t for t in range(b.T) if b.th[0, t] == b.th[2, t] < b.fh[t] and b.tw[0, t] != b.tw[2, t]]
        assert same_w and same_h, "no tile repeats a stored width / height across two sets that are not clones"  # a condition
    for (xf, uf) in [(4, 4), (2, 0)]:
        tiles, totals = check(gpu, b, xf, uf, f"{count} sets")
        if count >= 2:
            assert (tiles[1] == 0).all()
        _, alone, flags, status = run(gpu, b, xf, uf, want_tiles=False)
        assert status == 0 and (flags == 0).all()
        assert (alone == totals).all() and (alone == b.totals(tiles)).all(), "the totals are not the sums of the tiles"


# ---- 3. clones ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["alpha", "rgb"])
def test_clones_on_either_side(gpu, oracle, kind):
    """set 0: every tile at full size (zeros, garbage slots); sets 1 and 2 by hand, against a reference that is stored at full size
    throughout: its bytes are the reference"""
    rects = [r for (w, h) in [(100, 70), (33, 20)] for r in tile_rects(w, h, 32, 32)]
    full = (np.array([r[2] for r in rects], np.uint32), np.array([r[3] for r in rects], np.uint32))
    b = Batch(oracle, [(100, 70), (33, 20)], 32, 32, kind, None, seed=9, ref=full, sets=[full, dealt_sizes(rects, 1), dealt_sizes(rects, 3)])
    assert b.clone[0].all() and not b.clone[1].all()
    for (xf, uf) in [(4, 4), (0, 2)]:
        tiles, totals = check(gpu, b, xf, uf, f"clones {kind}")
        assert (tiles[0] == 0).all() and (totals[0] == 0).all() and tiles[1].any()
        # a reference at full size does not depend on its filter
        assert (tiles == b.expected(1, uf)).all()


# ---- 4. flags -----------------------------------------------------------------------------------------------------------

def test_bad_stored_sizes_are_marked_and_left_out(gpu, oracle):
    b = hand_batch(oracle, (16, 16), [(50, 33), (9, 5), (83, 61)], "alpha")
    exp = b.expected(4, 2)
    a2 = int(b.to[2])
    bad_ref, bad_set_zero, bad_set_wide = a2 + 1, a2 + 7, 2  # image 2 (a reference tile, and set 1's entry of another); image 0 (set 2)
    rtw, rth, rslots = (x.clone() for x in b.dev_ref)
    tw, th, slots = (x.clone() for x in b.dev_sets)
    rth[bad_ref] = int(b.fh[bad_ref]) + 1
    tw[1, bad_set_zero] = 0
    tw[2, bad_set_wide] = int(b.fw[bad_set_wide]) + 1
    rslots[bad_ref] = 0xEE  # (nothing of a bad reference tile is read)
    tiles, totals, flags, status = run(gpu, b, 4, 2, ref=(rtw, rth, rslots), sets=(tw, th, slots))
    assert status & 1
    assert flags.tolist() == [1, 0, 1], flags
    bad = np.zeros((b.K, b.T), bool)
    bad[:, bad_ref] = True
    bad[1, bad_set_zero] = True
    bad[2, bad_set_wide] = True
    assert (tiles[bad] == -1).all(), "UINT64_MAX at every set of a bad reference tile and at a bad set entry"
    assert (tiles[~bad] == exp[~bad]).all(), "an entry beside the bad ones"
    left = exp.copy()
    left[bad] = 0
    assert (totals == b.totals(left)).all(), "the totals leave the bad entries out, and only those"
    # a clean call afterwards clears the status and the flags
    check(gpu, b, 4, 2, "the clean call after a flagged one")


# ---- 5. the worst case of the per-tile sums ---------------------------------------------------------------------------------

@pytest.mark.parametrize("c", [4, 3])
def test_worst_case_sums_at_the_largest_block(gpu, product, c):
    """the largest block the size query admits, the reference all 255 (stored at full size), the set a 1x1 tile of zeros: every
    channel's sum is exactly fw * fh * 255^2 -- what the uint32 accumulation must hold"""
    import torch
    n = 1
    while product.reshrink_distortion_lds_bytes(n + 1, n + 1, c, 4, 4) <= LDS_PER_CU:
        n += 1
    assert n >= 96 and n * n * 65025 < 2 ** 32
    sizes = [(n, n), (n + 5, 7)]
    rects = [r for (w, h) in sizes for r in tile_rects(w, h, n, n)]
    T = len(rects)
    assert [(r[2], r[3]) for r in rects] == [(n, n), (n, 7), (5, 7)]
    i32 = lambda a: torch.tensor(a, dtype=torch.int32, device="cuda")  # noqa: E731
    ref = (i32([r[2] for r in rects]), i32([r[3] for r in rects]), torch.full((T, n * n * c), 255, dtype=torch.uint8, device="cuda"))
    sets = (i32([[1] * T]), i32([[1] * T]), torch.zeros((1, T, n * n * c), dtype=torch.uint8, device="cuda"))
    tiles = torch.full((1, T, c), POISON64, dtype=torch.int64, device="cuda")
    totals = torch.full((1, 2, c), POISON64, dtype=torch.int64, device="cuda")
    for (xf, uf) in [(4, 4), (0, 0)]:
        gpu.reshrink_distortion_varied_device(sizes, c, n, n, xf, uf, *ref, *sets, out=(tiles, totals))
        torch.cuda.synchronize()
        exp = np.array([[r[2] * r[3] * 65025] * c for r in rects], np.int64)
        assert (tiles[0].cpu().numpy() == exp).all(), (n, tiles[0].cpu().numpy().tolist(), exp.tolist())
        assert (totals[0].cpu().numpy() == np.stack([exp[0], exp[1] + exp[2]])).all()
    # one step beyond is refused, and nothing is written
    tiles.fill_(POISON64)
    with pytest.raises(product.PxzError) as e:
        gpu.reshrink_distortion_varied_device(sizes, c, n + 1, n + 1, 4, 4, *ref, *sets, out=(tiles, totals))
    assert e.value.code == UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((tiles == POISON64).all())


# ---- 6. many tiles, many images -------------------------------------------------------------------------------------------

def test_more_tiles_than_the_grid_has_waves(gpu, oracle):
    """35328 tiles of 8x8 in one image: eight waves to a block and at most 4096 blocks leave the grid 32768 waves, so waves walk
    the grid-stride loop; set 1's entries start 35328 tiles behind set 0's"""
    import torch
    bw = bh = 8
    w, h, c, K = 2048, 1100, 3, 2
    cols, rows = w // bw, -(-h // bh)
    T = cols * rows
    assert T == 35328 > 32768 and h % bh == 4
    rng = np.random.default_rng(35328)
    fh = np.where(np.arange(T) // cols == rows - 1, 4, 8).astype(np.uint32)
    shapes = np.array([(8, 8), (4, 8), (8, 4), (3, 5), (1, 1), (6, 7), (5, 2)], np.uint32)

    def draw(count):
        pick = shapes[rng.integers(0, len(shapes), count * T)]
        return pick[:, 0].reshape(count, T), np.minimum(pick[:, 1].reshape(count, T), fh[None])
    (rtw, rth), (tw, th) = draw(1), draw(K)
    rslots = rng.integers(0, 256, (T, bw * bh * c), dtype=np.uint8)
    slots = rng.integers(0, 256, (K, T, bw * bh * c), dtype=np.uint8)
    ref = oracle.expand_image(w, h, bw, bh, c, 4, rtw[0], rth[0], rslots).astype(np.int64)
    exp = np.zeros((K, T, c), np.int64)
    for k in range(K):
        d = np.zeros((rows * bh, w, c), np.int64)
        d[:h] = (ref - oracle.expand_image(w, h, bw, bh, c, 2, tw[k], th[k], slots[k]).astype(np.int64)) ** 2
        exp[k] = d.reshape(rows, bh, cols, bw, c).sum(axis=(1, 3)).reshape(T, c)
    exp[(tw == 8) & (th == fh[None])] = 0  # clones: the reference by definition
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a).astype(np.int32)).cuda()  # noqa: E731
    tiles = torch.full((K, T, c), POISON64, dtype=torch.int64, device="cuda")
    totals = torch.full((K, 1, c), POISON64, dtype=torch.int64, device="cuda")
    gpu.reshrink_distortion_varied_device([(w, h)], c, bw, bh, 4, 2, i32(rtw[0]), i32(rth[0]), torch.from_numpy(rslots).cuda(), i32(tw), i32(th),
                                          torch.from_numpy(slots).cuda(), out=(tiles, totals))
    torch.cuda.synchronize()
    tiles = tiles.cpu().numpy()
    assert exp.any(axis=2).sum() > T and (tiles == exp).all(), np.argwhere((tiles != exp).any(axis=2))[:10].tolist()
    assert (totals.cpu().numpy()[:, 0] == exp.sum(axis=1)).all()


@pytest.mark.parametrize("kind", ["alpha", "rgb"])
def test_2049_one_tile_images(gpu, oracle, kind):
    """one image more than a block keeps first tiles of in LDS: the owner search reads the table itself, and every tile belongs to
    another image"""
    sizes = [(1 + (7 * i) % 8, 1 + (5 * i) % 8) for i in range(2049)]
    b = Batch(oracle, sizes, 8, 8, kind, shifts=(0, 3), seed=2049)
    assert b.T == b.n == 2049
    tiles, totals = check(gpu, b, 4, 1, f"2049 images {kind}")
    assert (totals == tiles).all() and tiles.any()


def test_two_table_sets_survive_a_full_cache(product, oracle):
    """The call needs the tables of both filters at once, and the handle keeps at most 16 sets, emptying the cache before the 17th
    is built.  On a fresh handle, fifteen geometries with one filter leave room for exactly one more set: the next call, with two
    different filters and new tile sides, builds the reference's set into the last place and the sets' into an emptied cache"""
    import torch
    h = product.Handle(0)
    try:
        for k in range(17):
            b = Batch(oracle, [(8 + k, 8), (5, 3 + k)], 8, 24, "alpha", shifts=(0, 3), seed=k)  # edge sides k and 3 + k: new sides every time
            xf, uf = (4, 2) if k >= 15 else (4, 4)
            tiles, totals, flags, status = run(h, b, xf, uf)
            assert status == 0 and (flags == 0).all()
            assert (tiles == b.expected(xf, uf)).all() and (totals == b.totals(b.expected(xf, uf))).all(), f"geometry {k}"
        torch.cuda.synchronize()
    finally:
        h.close()


# ---- 7. slots beyond 4 GiB ----------------------------------------------------------------------------------------------------

def test_sets_beyond_4_gib_are_addressed_with_64_bits(gpu, product):
    """96x96 RGBA slots are 36864 bytes; with 32 sets of 3782 tiles every slot of set 31 starts beyond byte 2^32.  Stored tiles are
    1x1 and opaque, the filters Nearest, so tile t of set s expands to one colour and the expected sum is fw * fh * (reference -
    set)^2 per channel.  The whole buffer is filled with a decoy byte first: a 32-bit offset would read (offset mod 2^32), which
    holds the decoy or another tile's pixel"""
    import torch
    bw = bh = 96
    K, c, slot = 32, 4, 96 * 96 * 4
    assert product.reshrink_distortion_lds_bytes(bw, bh, c, 0, 0) <= LDS_PER_CU
    sizes = [(63 * bw, 60 * bh), (100, 50)]
    rects = [r for (w, h) in sizes for r in tile_rects(w, h, bw, bh)]
    T = len(rects)
    assert T == 3782 and (K - 1) * T * slot >= 2 ** 32
    try:
        slots = torch.full((K * T, slot), 0x77, dtype=torch.uint8, device="cuda")
    except (torch.cuda.OutOfMemoryError, RuntimeError) as e:
        pytest.skip(f"the device refused the {K * T * slot / 2 ** 30:.1f} GiB of slots this test addresses: {e}")
    rng = np.random.default_rng(4)
    px = rng.integers(0, 256, (K * T, 4), dtype=np.uint8)
    px[:, 3] = 255
    ref_px = rng.integers(0, 256, (T, 4), dtype=np.uint8)
    ref_px[:, 3] = 255
    slots[:, :4] = torch.from_numpy(px).cuda()
    beyond = np.arange(K * T, dtype=np.int64) * slot >= 2 ** 32
    assert beyond[(K - 1) * T:].all() and beyond.sum() > T
    # what a 32-bit offset would reach differs from what must be read, for every slot beyond 4 GiB
    wrapped = (np.arange(K * T, dtype=np.int64)[beyond] * slot) % 2 ** 32
    at_wrapped = np.where(wrapped % slot == 0, px[wrapped // slot, 0], 0x77)
    assert (at_wrapped != px[beyond, 0]).mean() > 0.99
    rslots = torch.zeros((T, slot), dtype=torch.uint8, device="cuda")
    rslots[:, :4] = torch.from_numpy(ref_px).cuda()
    ones = torch.ones(K * T, dtype=torch.int32, device="cuda")
    tiles = torch.full((K, T, c), POISON64, dtype=torch.int64, device="cuda")
    totals = torch.full((K, 2, c), POISON64, dtype=torch.int64, device="cuda")
    gpu.reshrink_distortion_varied_device(sizes, c, bw, bh, 0, 0, ones[:T], ones[:T], rslots, ones.view(K, T), ones.view(K, T), slots.view(K, T, slot),
                                          out=(tiles, totals))
    torch.cuda.synchronize()
    area = np.array([r[2] * r[3] for r in rects], np.int64)
    exp = area[None, :, None] * (ref_px.astype(np.int64)[None] - px.astype(np.int64).reshape(K, T, 4)) ** 2
    got = tiles.cpu().numpy()
    assert (got[K - 1] == exp[K - 1]).all(), "the slots of the last set, beyond 4 GiB, were not the ones read"
    assert (got == exp).all()
    assert (totals.cpu().numpy() == np.stack([exp[:, :T - 2].sum(axis=1), exp[:, T - 2:].sum(axis=1)], axis=1)).all()


# ---- 8. a real ladder ---------------------------------------------------------------------------------------------------------

def golden_image(golden_dir, name, crop):
    img = np.asarray(Image.open(os.path.join(golden_dir, name)))
    if crop:
        img = img[:crop[1], :crop[0]]
    return np.ascontiguousarray(img)


@pytest.mark.parametrize("name,block,crop", [("image.png", 64, None), ("base.png", 32, (200, 150))])
@pytest.mark.parametrize("mode,first,factors", [(1, 1024.0, [512.0, 128.0, 32.0, 4.0]), (0, 2.0, [1.0, 0.5, 0.125, 0.03])], ids=["directional", "shrink_by"])
def test_end_to_end_on_a_real_ladder(gpu, product, oracle, golden_dir, name, block, crop, mode, first, factors):
    """the image shrunk once (the archive), the re-shrink ladder out of place at four factors, and the sums against the oracle's
    expansion of the archive and of every rung the device wrote"""
    import torch
    img = golden_image(golden_dir, name, crop)
    h, w, c = img.shape
    down, xf, uf = 4, 2, 4
    _, atw, ath, aslots = oracle.shrink_image(img, block, block, mode, down, first, nthreads=8)
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a).astype(np.int32)).cuda()  # noqa: E731
    ref = (i32(atw), i32(ath), torch.from_numpy(np.ascontiguousarray(aslots)).cuda())
    _, vals, ow, oh, slots = gpu.reshrink_varied_ladder_frames_device([(w, h)], c, block, block, mode, down, factors, xf, *ref)
    tiles, totals = gpu.reshrink_distortion_varied_device([(w, h)], c, block, block, xf, uf, *ref, ow, oh, slots)
    torch.cuda.synchronize()
    assert bool((ref[0] == i32(atw)).all()) and bool((ref[2] == torch.from_numpy(np.ascontiguousarray(aslots)).cuda()).all())  # the archive is kept
    hw, hh, hs = ow.cpu().numpy().astype(np.uint32), oh.cpu().numpy().astype(np.uint32), slots.cpu().numpy()
    ref_img = oracle.expand_image(w, h, block, block, c, xf, atw, ath, np.ascontiguousarray(aslots)).astype(np.int64)
    tiles, totals = tiles.cpu().numpy(), totals.cpu().numpy()
    for r, k in enumerate(factors):
        rung = oracle.expand_image(w, h, block, block, c, uf, hw[r], hh[r], hs[r]).astype(np.int64)
        exp = tile_sums((ref_img - rung) ** 2, w, h, block, block)
        print(f"{name} mode {mode} k={k}: sse {totals[r, 0].tolist()} (oracle {exp.sum(axis=0).tolist()}), "
              f"PSNR against the archive {product.psnr(int(totals[r, 0].sum()), h * w * c):.2f} dB")
        assert (tiles[r] == exp).all(), f"factor {k}: tiles {np.argwhere((tiles[r] != exp).any(axis=1)).ravel()[:10].tolist()}"
        assert (totals[r, 0] == exp.sum(axis=0)).all(), f"factor {k}: totals"
    assert len({tuple(t) for t in totals[:, 0].tolist()}) >= 2 and totals.any()  # the factors spread the errors


# ---- 9. the host forms ----------------------------------------------------------------------------------------------------------

ARCHIVE_SIZES = [(150, 100), (9, 9), (70, 131), (100, 38), (66, 35)]  # five files of different sizes
# unsorted; rungs 1 and 5 are one factor and rungs 2 and 6 another: where a target falls on such a pair, the lower index decides
ARCHIVE_FACTORS = {0: [.25, .125, .5, 2, .05, .125, .5, .02], 1: [4, 2, 8, 32, .8, 2, 8, .32]}
DOWN, XF, UF, FILTER_BYTE = 4, 2, 3, 3
_archives = {}


class Archive:
    """five .pixlzr files written by the oracle (file 0 with every tile at full size, so that it decodes to an image no rung of
    which is free of error; the others at a middling factor, with reduced tiles) and, computed once on the CPU, what the oracle
    composition decode -> expand(XF) -> shrink(factors[r]) -> encode / expand(UF) makes of them: the table and every rung's files"""

    def __init__(self, oracle, block, c, mode):
        from test_gpu_fit import host_images
        self.block, self.c, self.mode, self.factors = block, c, mode, ARCHIVE_FACTORS[mode]
        images = host_images(block, c, mode)[:len(ARCHIVE_SIZES)]
        assert [(i.shape[1], i.shape[0]) for i in images] == ARCHIVE_SIZES
        wrote = [1e6] + [[1.0, 16.0][mode]] * (len(images) - 1)
        self.files, self.decoded = [], []
        K, n = len(self.factors), len(images)
        self.bytes, self.sse = np.zeros((K, n), np.uint64), np.zeros((K, n, c), np.uint64)
        self.rungs = [[None] * n for _ in range(K)]
        for i, (img, f) in enumerate(zip(images, wrote)):
            h, w = img.shape[:2]
            vals, tw, th, slots = oracle.shrink_image(img, block, block, mode, DOWN, f, nthreads=8)
            self.files.append(oracle.encode_container(w, h, block, block, c, 0, vals, None, tw, th, slots))
            d = oracle.decode_container(self.files[-1])
            ref = oracle.expand_image(w, h, block, block, c, XF, d["tw"], d["th"], np.ascontiguousarray(d["slots"][:, :block * block * c]))
            self.decoded.append(ref)
            for r, k in enumerate(self.factors):
                rv, rw, rh, rs = oracle.shrink_image(ref, block, block, mode, DOWN, k, nthreads=8)
                self.rungs[r][i] = oracle.encode_container(w, h, block, block, c, FILTER_BYTE, rv, None, rw, rh, rs)
                self.bytes[r, i] = len(oracle.encode_container(w, h, block, block, c, 0, rv, None, rw, rh, rs))
                back = oracle.expand_image(w, h, block, block, c, UF, rw, rh, rs)
                self.sse[r, i] = ((ref.astype(np.int64) - back.astype(np.int64)) ** 2).sum(axis=(0, 1))
        assert (self.decoded[0] == images[0]).all()


def archive(oracle, block, c, mode):
    if (block, c, mode) not in _archives:
        _archives[(block, c, mode)] = Archive(oracle, block, c, mode)
    return _archives[(block, c, mode)]


def targets_from(file_bytes, sse, criterion):
    """per file its third-smallest length (FIT_BYTES) or error (FIT_SSE); file 0 gets 0, file 1 2^64-1"""
    q = file_bytes if criterion == FIT_BYTES else sse.sum(axis=2)
    t = [int(np.sort(q[:, i])[2]) for i in range(q.shape[1])]
    t[0], t[1] = 0, U64
    return t


@pytest.mark.parametrize("mode", [0, 1], ids=["shrink_by", "directional"])
@pytest.mark.parametrize("block,c", [(32, 4), (64, 3)])
def test_the_table_equals_the_ladder_files_size_query_and_the_oracle(gpu, oracle, block, c, mode):
    a = archive(oracle, block, c, mode)
    file_bytes, sse = gpu.rate_distortion_varied_files(a.files, block, block, mode, DOWN, XF, UF, a.factors)
    query = gpu.transcode_varied_ladder_files(a.files, block, block, mode, DOWN, a.factors, XF, filter_byte=0, sizes_only=True)
    assert file_bytes.shape == (len(a.factors), len(a.files)) and sse.shape == file_bytes.shape + (c,)
    assert (file_bytes.astype(np.int64) == query).all(), "the bytes column differs from pxz_transcode_varied_ladder_files' size query"
    print(f"block {block} c{c} mode {mode}: bytes\n{file_bytes}\nsse\n{sse.sum(axis=2)}")
    assert (file_bytes == a.bytes).all(), "the bytes column differs from the oracle's files"
    assert (sse == a.sse).all(), "the sse column differs from the oracle's"
    assert sse.any() and max(len(set(file_bytes[:, i].tolist())) for i in range(len(a.files))) >= 3  # the factors spread the files


@pytest.mark.parametrize("criterion", [FIT_BYTES, FIT_SSE], ids=["bytes", "sse"])
@pytest.mark.parametrize("mode", [0, 1], ids=["shrink_by", "directional"])
@pytest.mark.parametrize("block,c", [(32, 4), (64, 3)])
def test_fit_files_equal_the_one_factor_transcode_and_todays_detour(gpu, product, oracle, block, c, mode, criterion):
    a = archive(oracle, block, c, mode)
    Kf, n = len(a.factors), len(a.files)
    targets = targets_from(a.bytes, a.sse, criterion)
    exp_choice, exp_flags = select(a.bytes.tolist(), a.sse.tolist(), criterion, targets)
    # what the table must hold for the comparison below to say anything
    total = a.sse.sum(axis=2)
    assert any(0 < r < Kf - 1 for r in exp_choice), "every expected choice is the first or the last rung"
    assert any(any(q != r and a.bytes[q, i] == a.bytes[r, i] and total[q, i] == total[r, i] for q in range(Kf))
               for i, r in enumerate(exp_choice)), "no choice is decided by the lowest index among equal rungs"
    assert any(exp_flags), "no file misses its target"

    files, choice, flags, t_bytes, t_sse = gpu.transcode_varied_files_fit(a.files, block, block, mode, DOWN, XF, UF, a.factors, criterion, targets,
                                                                          filter_byte=FILTER_BYTE, want_table=True)
    assert (t_bytes == a.bytes).all() and (t_sse == a.sse).all(), "the table differs from the oracle's"
    h_choice, h_flags = product.fit_select(t_bytes, t_sse, criterion, targets)
    assert choice.tolist() == h_choice.tolist() == exp_choice and flags.tolist() == h_flags.tolist() == exp_flags
    for i in range(n):
        k = a.factors[exp_choice[i]]
        alone = gpu.transcode_varied_files([a.files[i]], block, block, mode, DOWN, k, XF, filter_byte=FILTER_BYTE)[0]
        assert files[i] == alone, f"file {i} at factor {k}: differs from pxz_transcode_varied_files of the file alone"
        assert files[i] == a.rungs[exp_choice[i]][i], f"file {i} at factor {k}: differs from the oracle's file"
    # today's detour: decode to pixels, download, upload, fit from the image
    images, dflags = gpu.decode_varied_files(a.files, c, block, block, XF)
    assert (dflags == 0).all() and all((x == y).all() for x, y in zip(images, a.decoded))
    d_files, d_choice, d_fl, d_bytes, d_sse = gpu.encode_varied_images_fit(images, block, block, mode, DOWN, UF, a.factors, criterion, targets,
                                                                           filter_byte=FILTER_BYTE, want_table=True)
    assert d_files == files and d_choice.tolist() == choice.tolist() and d_fl.tolist() == flags.tolist()
    assert (d_bytes == t_bytes).all() and (d_sse == t_sse).all()


# ---- 10. size query and errors ----------------------------------------------------------------------------------------------------

def test_size_query_then_exact_capacity(gpu, product, oracle):
    a = archive(oracle, 32, 4, 0)
    targets = targets_from(a.bytes, a.sse, FIT_BYTES)
    files, choice, flags = gpu.transcode_varied_files_fit(a.files, 32, 32, 0, DOWN, XF, UF, a.factors, FIT_BYTES, targets, filter_byte=FILTER_BYTE)
    total = sum(len(f) for f in files)
    for out in (np.zeros(0, np.uint8), np.full(total - 1, POISON, np.uint8)):
        with pytest.raises(product.PxzError) as e:
            gpu.transcode_varied_files_fit(a.files, 32, 32, 0, DOWN, XF, UF, a.factors, FIT_BYTES, targets, filter_byte=FILTER_BYTE, out=out)
        assert e.value.code == BUFFER_TOO_SMALL and e.value.needed == total
        assert (e.value.choice == choice).all() and (e.value.fit_flags == flags).all()
        assert (e.value.table[0] == a.bytes).all() and (e.value.table[1] == a.sse).all()
        assert (out == POISON).all(), "a call that was short of room wrote to out"
    exact = np.full(total + 16, POISON, np.uint8)
    got, _, _ = gpu.transcode_varied_files_fit(a.files, 32, 32, 0, DOWN, XF, UF, a.factors, FIT_BYTES, targets, filter_byte=FILTER_BYTE,
                                               out=exact[:total])
    assert got == files and (exact[total:] == POISON).all()


class RawFit:
    """pxz_transcode_varied_files_fit and pxz_rate_distortion_varied_files through ctypes, every output poisoned"""

    def __init__(self, gpu, product, files, block, mode, factors, criterion=FIT_BYTES, targets=None):
        self.gpu, self.n = gpu, len(files)
        self.bufs = [np.frombuffer(bytes(f), np.uint8) for f in files]
        self.pd = product.binding.Params(block[0], block[1], mode, DOWN, 0.0, 0)
        self.fac = np.ascontiguousarray(factors, np.float32)
        self.n_factors, self.criterion, self.xf, self.uf = self.fac.size, criterion, XF, UF
        self.targets = np.array([int(t) for t in (targets if targets is not None else [100] * self.n)], np.uint64)
        kn = max(self.n_factors, 1) * self.n
        self.offs = np.full(self.n + 1, U64, np.uint64)
        self.choice, self.flags = np.full(self.n, POISON32, np.uint32), np.full(self.n, POISON32, np.uint32)
        self.t_bytes, self.t_sse = np.full(kn, U64, np.uint64), np.full(kn * 4, U64, np.uint64)
        self.out = np.full(1 << 20, POISON, np.uint8)

    def head(self, null_factors):
        ptr = lambda a: None if a is None else C.c_void_p(a.ctypes.data)  # noqa: E731
        ptrs = (C.c_void_p * self.n)(*[b.ctypes.data for b in self.bufs])
        lens = (C.c_size_t * self.n)(*[b.size for b in self.bufs])
        self._keep = (ptrs, lens)
        return [self.gpu._h, C.cast(ptrs, C.c_void_p), C.cast(lens, C.c_void_p), self.n, C.byref(self.pd), self.xf, self.uf,
                None if null_factors else ptr(self.fac), self.n_factors], ptr

    def fit(self, null_targets=False, null_factors=False):
        head, ptr = self.head(null_factors)
        return self.gpu._L.pxz_transcode_varied_files_fit(*head, self.criterion, None if null_targets else ptr(self.targets), FILTER_BYTE,
                                                          ptr(self.out), self.out.size, ptr(self.offs), ptr(self.choice), ptr(self.flags),
                                                          ptr(self.t_bytes), ptr(self.t_sse))

    def table(self, null_factors=False):
        head, ptr = self.head(null_factors)
        return self.gpu._L.pxz_rate_distortion_varied_files(*head, ptr(self.t_bytes), ptr(self.t_sse))

    def untouched(self):
        return bool((self.offs == U64).all() and (self.choice == POISON32).all() and (self.flags == POISON32).all() and
                    (self.t_bytes == U64).all() and (self.t_sse == U64).all() and (self.out == POISON).all())


def test_host_form_errors_write_nothing(gpu, product, oracle):
    a = archive(oracle, 32, 4, 0)

    def refused(code, text=None, files=a.files, block=(32, 32), factors=a.factors, both=True, **kw):
        for form in (("fit", "table") if both else ("fit",)):
            raw = RawFit(gpu, product, files, block, 0, factors)
            call_kw = {}
            for key, v in kw.items():
                if key in ("null_targets", "null_factors"):
                    call_kw[key] = v
                else:
                    setattr(raw, key, v)
            assert getattr(raw, form)(**call_kw) == code, (form, kw, last_error(gpu))
            assert raw.untouched(), (form, kw, "an error case wrote its outputs")
            assert text is None or text in last_error(gpu), last_error(gpu)

    refused(INVALID_ARG, criterion=2, both=False)
    refused(INVALID_ARG, null_targets=True, both=False)
    refused(INVALID_ARG, null_factors=True)
    refused(INVALID_ARG, n_factors=0)
    refused(INVALID_ARG, factors=[1.0] * 33)
    refused(INVALID_ARG, factors=[0.5, float("nan")])
    refused(INVALID_ARG, xf=5)
    refused(INVALID_ARG, uf=5)
    # a malformed file: all or nothing, and the image is named
    cut = list(a.files)
    cut[3] = cut[3][:len(cut[3]) - 9]
    refused(INVALID_ARG, "image 3", files=cut)
    refused(INVALID_ARG, "image 2", files=a.files[:2] + [a.files[2][:10]] + a.files[3:])
    # files of another channel count among them; files of another block size than the call's
    other = archive(oracle, 64, 3, 0)
    refused(INVALID_ARG, "image 1", files=[a.files[0], other.files[1]])
    refused(UNSUPPORTED, "block", block=(64, 64))
    refused(UNSUPPORTED, "block", block=(32, 16))
    # and the handle still works
    file_bytes, sse = gpu.rate_distortion_varied_files(a.files, 32, 32, 0, DOWN, XF, UF, a.factors)
    assert (file_bytes == a.bytes).all() and (sse == a.sse).all()


def test_device_form_errors_write_nothing(gpu, product, oracle):
    import torch
    b = hand_batch(oracle, (16, 16), [(50, 33), (9, 5), (83, 61)], "alpha")
    L, P, descs_of = gpu._L, product.binding.Params, product.binding.image_descs
    geoms = [(w, h, w * 4, 0) for (w, h) in b.sizes]
    ok = P(16, 16, 0, 2, 0.0, 0)
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    def call(code, text=None, geoms=geoms, count=3, channels=4, p=ok, xf=4, n_sets=3, missing=()):
        tiles = torch.full((b.K, b.T, 4), POISON64, dtype=torch.int64, device="cuda")
        totals = torch.full((b.K, b.n, 4), POISON64, dtype=torch.int64, device="cuda")
        flags = torch.full((b.n,), POISON32, dtype=torch.int32, device="cuda")
        dev = dict(zip(("rw", "rh", "rs", "w", "h", "s"), b.dev_ref + b.dev_sets))
        args = [None if k in missing else ptr(v) for k, v in dev.items()]
        rc = L.pxz_reshrink_distortion_varied_device(gpu._h, C.cast(descs_of(geoms), C.c_void_p) if geoms is not None else None, count, channels,
                                                     C.byref(p) if p is not None else None, xf, n_sets, *args, ptr(tiles),
                                                     None if "totals" in missing else ptr(totals), ptr(flags))
        torch.cuda.synchronize()
        assert rc == code, (rc, last_error(gpu))
        assert bool((tiles == POISON64).all() and (totals == POISON64).all() and (flags == POISON32).all()), "an error case wrote its outputs"
        assert text is None or text in last_error(gpu), last_error(gpu)

    call(INVALID_ARG, p=None)
    call(INVALID_ARG, geoms=None)
    call(INVALID_ARG, count=0)
    call(INVALID_ARG, channels=2)
    call(INVALID_ARG, channels=5)
    call(INVALID_ARG, n_sets=0)
    call(INVALID_ARG, xf=5)
    call(INVALID_ARG, p=P(16, 16, 0, 5, 0.0, 0))
    call(INVALID_ARG, p=P(0, 16, 0, 2, 0.0, 0))
    for k in ("rw", "rh", "rs", "w", "h", "s", "totals"):
        call(INVALID_ARG, missing=(k,))
    call(INVALID_ARG, "image 1", geoms=[geoms[0], geoms[1] + (1,), geoms[2]])          # reserved
    call(INVALID_ARG, "image 2", geoms=[geoms[0], geoms[1], (0, 61, 0, 0)])            # an empty image
    call(UNSUPPORTED, "image 0", geoms=[(2 ** 24 + 1, 4, 0, 0), geoms[1], geoms[2]])   # a side above 2^24
    call(UNSUPPORTED, p=P(128, 128, 0, 2, 0.0, 0))                                     # three planes of 64 KB
    call(UNSUPPORTED, p=P(200, 200, 0, 2, 0.0, 0))
    call(UNSUPPORTED, "sets", geoms=[(2 ** 14, 2 ** 14, 0, 0)], count=1, n_sets=2 ** 13)  # 2^20 tiles in 2^13 sets: above 2^32-1
    check(gpu, b, 4, 2, "the clean call after the refused ones")


# ---- 11. the handle is left alone -----------------------------------------------------------------------------------------------

def test_the_handle_is_left_alone(gpu, product, oracle):
    import torch
    from test_gpu_parity import assert_same_tiles
    frames = gpu.synth_frames_device(2, 200, 328, 4, dist=product.DIST_ALPHA)
    a = archive(oracle, 32, 4, 0)
    b = hand_batch(oracle, (32, 32), [(100, 70)], "alpha")
    targets = targets_from(a.bytes, a.sse, FIT_SSE)

    def single():
        vals, ow, oh, slots = (x.cpu().numpy() for x in gpu.shrink_frames_device(frames, 32, 32, 0, 4, 1.0))
        return vals.reshape(-1), ow.reshape(-1), oh.reshape(-1), slots.reshape(-1, slots.shape[-1])

    def three_calls():
        tiles, totals, _, _ = run(gpu, b, 4, 2)
        file_bytes, sse = gpu.rate_distortion_varied_files(a.files, 32, 32, 0, DOWN, XF, UF, a.factors)
        files, choice, flags = gpu.transcode_varied_files_fit(a.files, 32, 32, 0, DOWN, XF, UF, a.factors, FIT_SSE, targets)
        return [tiles, totals, file_bytes, sse, np.frombuffer(b"".join(files), np.uint8), choice, flags]

    single()  # (the first launch on a handle has no statistics of a launch before it)
    before, state = single(), gpu.state()
    first = three_calls()
    torch.cuda.synchronize()
    assert gpu.state() == state, "a call of the archive fit changed what pxz_handle_state reports"
    assert_same_tiles(single(), before, 4, "the single-geometry call after the archive fit")
    gpu.trim()
    again = three_calls()
    assert gpu.state() == state
    for k, (x, y) in enumerate(zip(first, again)):
        assert x.tobytes() == y.tobytes(), f"result {k} differs after a trim"
    assert (first[0] == b.expected(4, 2)).all() and (first[2] == a.bytes).all() and (first[3] == a.sse).all()
