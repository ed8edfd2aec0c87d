"""Distortion of re-tiled tiles against the archive they came from (pxz_retile_distortion_varied_device,
pxz_rate_distortion_retile_files, pxz_retile_varied_files_fit, pxz_retile_varied_files_fit_tiles).  Every comparison is exact
integer or byte equality.  The expected value always comes from the oracle on the CPU: oracle.expand_image of the archive's tiles
at the SOURCE block with expand_filter, oracle.expand_image of each set at the NEW block with filter_up, the squared differences
summed per tile of the new grid in numpy int64; for the host forms oracle.decode_container, oracle.shrink_image at the new block
and oracle.encode_container besides -- never anything the library computed.  A set tile stored at its full size is the
reference by definition (sums 0, its slot is not read), so such slots hold garbage here.  The stored sizes of the first tests are
made by hand and the stored bytes are random, so the kernel is exercised independently of any detector.  Outputs are poisoned
before every call."""
import ctypes as C
import os

import numpy as np
import pytest
from PIL import Image

from test_fit_host import FIT_BYTES, FIT_SSE, U64, select
from test_gpu_distortion import BOTH, FULL, LOWER, NARROWER, ONE, POISON, POISON64, class_of, random_slots, tile_rects
from test_gpu_reshrink_distortion import (ARCHIVE_SIZES, BUFFER_TOO_SMALL, DOWN, FILTER_BYTE, INVALID_ARG, POISON32, UF, UNSUPPORTED, XF, archive,
                                          dealt_sizes, last_error, targets_from, tile_sums)
from test_gpu_reshrink_distortion import run as reshrink_run

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu(product):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    h = product.Handle(0)
    yield h
    h.close()


# ---- inputs and the expected sums ---------------------------------------------------------------------------------------

class Batch:
    """images of the given sizes (no pixels: the archive is all there is), the archive's stored tiles in the layout of `src` blocks
    and n_sets stored versions of the tiles of the `dst` grid: sizes by hand, bytes random.  shifts: where each set starts dealing
    its shapes (the reference starts at 1)."""

    def __init__(self, oracle, sizes, src, dst, kind, shifts=(0, 2, 3), seed=0, sets=None):
        import torch
        self.oracle, self.sizes, self.src, self.dst, self.kind = oracle, sizes, src, dst, kind
        self.c = c = 3 if kind == "rgb" else 4
        rng = np.random.default_rng(seed + src[0] * 100000 + dst[0] * 1000 + dst[1] * 10 + c)
        self.src_per_image = [tile_rects(w, h, *src) for (w, h) in sizes]
        self.src_rects = [r for rects in self.src_per_image for r in rects]
        self.sto = np.concatenate([[0], np.cumsum([len(r) for r in self.src_per_image])])
        self.per_image = [tile_rects(w, h, *dst) for (w, h) in sizes]
        self.rects = [r for rects in self.per_image for r in rects]
        self.to = np.concatenate([[0], np.cumsum([len(r) for r in self.per_image])])
        self.T, self.Ts, self.n = len(self.rects), len(self.src_rects), len(sizes)
        self.fw = np.array([r[2] for r in self.rects], np.uint32)
        self.fh = np.array([r[3] for r in self.rects], np.uint32)
        self.sfw = np.array([r[2] for r in self.src_rects], np.uint32)
        self.sfh = np.array([r[3] for r in self.src_rects], np.uint32)
        self.rtw, self.rth = dealt_sizes(self.src_rects, 1)
        self.rslots = random_slots(rng, self.rtw, self.rth, src[0] * src[1], c, kind)
        sets = sets if sets is not None else [dealt_sizes(self.rects, s) for s in shifts]
        self.K = len(sets)
        self.tw = np.stack([s[0] for s in sets]).astype(np.uint32)
        self.th = np.stack([s[1] for s in sets]).astype(np.uint32)
        slot_px = dst[0] * dst[1]
        self.slots = np.stack([random_slots(rng, self.tw[k], self.th[k], slot_px, c, kind) for k in range(self.K)])
        self.clone = (self.tw == self.fw[None]) & (self.th == self.fh[None])
        # a clone's slot is not read: bytes that would show
        self.slots[self.clone] = rng.integers(0, 256, (int(self.clone.sum()), slot_px * c), dtype=np.uint8)
        i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a).astype(np.int32)).cuda()  # noqa: E731
        self.dev_ref = (i32(self.rtw), i32(self.rth), torch.from_numpy(self.rslots).cuda())
        self.dev_sets = (i32(self.tw), i32(self.th), torch.from_numpy(self.slots).cuda())
        self._ref, self._expected = {}, {}

    def ref_images(self, xf):
        """what the archive decodes to: the oracle's expand at the SOURCE block"""
        if xf not in self._ref:
            self._ref[xf] = [self.oracle.expand_image(w, h, *self.src, self.c, xf, self.rtw[a:b], self.rth[a:b], self.rslots[a:b])
                             for (w, h), a, b in zip(self.sizes, self.sto[:-1], self.sto[1:])]
        return self._ref[xf]

    def expected(self, xf, uf):
        """int64 [K, T, c] over the tiles of the NEW grid: computed once per pair of filters and left unchanged"""
        if (xf, uf) not in self._expected:
            out = np.zeros((self.K, self.T, self.c), np.int64)
            for k in range(self.K):
                for (w, h), a, b, ref in zip(self.sizes, self.to[:-1], self.to[1:], self.ref_images(xf)):
                    img = self.oracle.expand_image(w, h, *self.dst, self.c, uf, self.tw[k, a:b], self.th[k, a:b], self.slots[k, a:b])
                    out[k, a:b] = tile_sums((ref.astype(np.int64) - img.astype(np.int64)) ** 2, w, h, *self.dst)
            out[self.clone] = 0
            self._expected[(xf, uf)] = out
        return self._expected[(xf, uf)]

    def totals(self, tiles):
        """[K, T, c] -> [K, n, c]"""
        return np.stack([tiles[:, a:b].sum(axis=1) for a, b in zip(self.to[:-1], self.to[1:])], axis=1)

    def covered_by(self, image, src_tile):
        """the flat tiles of the new grid that overlap tile `src_tile` (flat, source layout) of image `image`"""
        x, y, fw, fh = self.src_rects[src_tile]
        return [int(self.to[image]) + t for t, (dx, dy, dw, dh) in enumerate(self.per_image[image])
                if dx < x + fw and x < dx + dw and dy < y + fh and y < dy + dh]


def run(gpu, b, xf, uf, want_tiles=True, ref=None, sets=None):
    """one call into poisoned outputs -> (tile sums | None, totals, flags, pxz_decode_status) on the host"""
    import torch
    ref, sets = ref or b.dev_ref, sets or b.dev_sets
    K = sets[0].shape[0]
    tiles = torch.full((K, b.T, b.c), POISON64, dtype=torch.int64, device="cuda")
    totals = torch.full((K, b.n, b.c), POISON64, dtype=torch.int64, device="cuda")
    flags = torch.full((b.n,), POISON32, dtype=torch.int32, device="cuda")
    gpu.retile_distortion_varied_device(b.sizes, b.c, *b.src, *b.dst, xf, uf, *ref, *sets, out=(tiles if want_tiles else None, totals),
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

PAIRS = [((64, 64), (32, 32)),   # new tiles split stored tiles
         ((32, 32), (64, 64)),   # new tiles merge stored tiles
         ((32, 32), (48, 20)),   # new tiles straddle stored tiles
         ((16, 16), (16, 16))]   # equal blocks
IMAGE_SETS = [[(100, 70)],
              [(50, 33), (9, 5), (83, 61)],    # an image below either block, ragged edges
              [(130, 65), (70, 131)]]          # edge tiles 2x1 and 6x3 (at 64x64)
KINDS = ("opaque", "alpha", "rgb")
HAND_CASES = [(src, dst, sizes, kind) for (src, dst) in PAIRS for sizes in IMAGE_SETS for kind in KINDS]
_batches = {}


def hand_batch(oracle, src, dst, sizes, kind):
    key = (src, dst, tuple(sizes), kind)
    if key not in _batches:
        _batches[key] = Batch(oracle, sizes, src, dst, kind)
    return _batches[key]


def pair_id(src, dst):
    return f"{src[0]}x{src[1]}to{dst[0]}x{dst[1]}"


@pytest.mark.parametrize("src,dst,sizes,kind", HAND_CASES, ids=[f"{pair_id(s, d)}-{z[0][0]}x{z[0][1]}-{k}" for (s, d, z, k) in HAND_CASES])
def test_hand_made_sizes_equal_the_oracle(gpu, oracle, src, dst, sizes, kind):
    """the reference and three sets with the five classes dealt independently; Bilinear / CatmullRom, and Lanczos3 / Nearest"""
    b = hand_batch(oracle, src, dst, sizes, kind)
    if sizes == IMAGE_SETS[2]:  # (the image set with tiles enough on either side of every pair)
        every = {FULL, LOWER, NARROWER, BOTH, ONE}
        ref_classes = {class_of(int(fw), int(fh), int(a), int(c)) for fw, fh, a, c in zip(b.sfw, b.sfh, b.rtw, b.rth)}
        set_classes = {class_of(int(fw), int(fh), int(a), int(c)) for k in range(b.K) for fw, fh, a, c in zip(b.fw, b.fh, b.tw[k], b.th[k])}
        assert every <= ref_classes and every <= set_classes, (sorted(ref_classes), sorted(set_classes))  # a condition, not a measurement
    for (xf, uf) in [(2, 3), (4, 0)]:
        tiles, totals = check(gpu, b, xf, uf, f"{pair_id(src, dst)} {sizes} {kind}")
        if src == dst:  # equal blocks: also what the re-shrink's distortion gives on the same inputs
            class Same:
                pass
            s = Same()
            s.sizes, s.c, s.bw, s.bh, s.T, s.n, s.dev_ref, s.dev_sets = b.sizes, b.c, dst[0], dst[1], b.T, b.n, b.dev_ref, b.dev_sets
            r_tiles, r_totals, r_flags, r_status = reshrink_run(gpu, s, xf, uf)
            assert r_status == 0 and (r_flags == 0).all()
            assert (r_tiles == tiles).all() and (r_totals == totals).all(), "differs from pxz_reshrink_distortion_varied_device"


def test_all_25_filter_pairs(gpu, oracle):
    b = hand_batch(oracle, (64, 64), (32, 32), [(100, 70)], "alpha")
    for xf in range(5):
        for uf in range(5):
            check(gpu, b, xf, uf, "64x64 -> 32x32 alpha")


# ---- 2. targeted cases ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("src,dst", PAIRS[:3], ids=[pair_id(*p) for p in PAIRS[:3]])
def test_clone_slots_are_not_read(gpu, oracle, src, dst):
    import torch
    b = hand_batch(oracle, src, dst, [(100, 70)], "alpha")
    assert b.clone.any() and not b.clone.all()
    first, first_totals = check(gpu, b, 2, 3, "clones")
    slots = b.dev_sets[2].clone()
    slots[torch.from_numpy(b.clone).cuda()] = 0x3C  # other garbage
    tiles, totals, flags, status = run(gpu, b, 2, 3, sets=(b.dev_sets[0], b.dev_sets[1], slots))
    assert status == 0 and (flags == 0).all()
    assert (tiles == first).all() and (totals == first_totals).all() and (tiles[b.clone] == 0).all()


@pytest.mark.parametrize("src,dst", PAIRS, ids=[pair_id(*p) for p in PAIRS])
def test_without_the_tile_array_the_totals_are_still_exact(gpu, oracle, src, dst):
    b = hand_batch(oracle, src, dst, [(50, 33), (9, 5), (83, 61)], "rgb")
    _, totals, flags, status = run(gpu, b, 4, 0, want_tiles=False)  # (run asserts that the tile array keeps its poison)
    assert status == 0 and (flags == 0).all()
    assert (totals == b.totals(b.expected(4, 0))).all()


def test_32_sets(gpu, oracle):
    rects = tile_rects(50, 33, 32, 32)
    b = Batch(oracle, [(50, 33)], (64, 64), (32, 32), "alpha", seed=32, sets=[dealt_sizes(rects, s) for s in range(32)])
    assert b.K == 32
    for (xf, uf) in [(2, 3), (4, 0)]:
        check(gpu, b, xf, uf, "32 sets")


def test_a_bad_set_entry_is_marked_and_left_out(gpu, oracle):
    b = hand_batch(oracle, (64, 64), (32, 32), [(50, 33), (9, 5), (83, 61)], "alpha")
    exp = b.expected(2, 3)
    zero, wide = int(b.to[2]) + 4, 1  # image 2 (set 1: a stored width of 0); image 0 (set 2: wider than its place)
    tw, th, slots = (x.clone() for x in b.dev_sets)
    tw[1, zero] = 0
    tw[2, wide] = int(b.fw[wide]) + 1
    tiles, totals, flags, status = run(gpu, b, 2, 3, sets=(tw, th, slots))
    assert status & 1 and flags.tolist() == [1, 0, 1], (status, flags)
    bad = np.zeros((b.K, b.T), bool)
    bad[1, zero] = bad[2, wide] = True
    assert (tiles[bad] == -1).all(), "UINT64_MAX at a bad set entry"
    assert (tiles[~bad] == exp[~bad]).all(), "an entry beside the bad ones"
    left = exp.copy()
    left[bad] = 0
    assert (totals == b.totals(left)).all(), "the totals leave the bad entries out, and only those"
    check(gpu, b, 2, 3, "the clean call after a flagged one")


@pytest.mark.parametrize("src,dst", [PAIRS[1], PAIRS[0]], ids=[pair_id(*PAIRS[1]), pair_id(*PAIRS[0])])
@pytest.mark.parametrize("how", ["zero", "beyond"])
def test_a_bad_source_tile_marks_exactly_the_tiles_it_covers(gpu, oracle, src, dst, how):
    b = hand_batch(oracle, src, dst, [(130, 65), (70, 131)], "alpha")
    exp = b.expected(2, 3)
    image = 1
    bad_src = int(b.sto[image]) + 2  # a tile of image 1 in the source layout
    covered = b.covered_by(image, bad_src)
    assert 1 <= len(covered) < b.T - int(b.to[image]), covered  # some tiles of the image, not all of them
    if src == (64, 64):
        assert len(covered) > 1  # a stored tile that several new tiles split
    rtw, rth, rslots = (x.clone() for x in b.dev_ref)
    if how == "zero":
        rtw[bad_src] = 0
    else:
        rth[bad_src] = int(b.sfh[bad_src]) + 1
    rslots[bad_src] = 0xEE
    tiles, totals, flags, status = run(gpu, b, 2, 3, ref=(rtw, rth, rslots))
    assert status & 1 and flags.tolist() == [0, 1], (status, flags)
    bad = np.zeros((b.K, b.T), bool)
    bad[:, covered] = True
    assert (tiles[bad] == -1).all(), "UINT64_MAX at every set of every tile a bad source tile covers"
    assert (tiles[~bad] == exp[~bad]).all(), "an entry beside the covered ones"
    left = exp.copy()
    left[bad] = 0
    assert (totals == b.totals(left)).all(), "the totals leave the covered tiles out, and only those"
    check(gpu, b, 2, 3, "the clean call after a flagged one")


# ---- 3. against the library's own calls ---------------------------------------------------------------------------------------

# unsorted, with repeats; the scales at which tests/test_gpu_reshrink_distortion.py spreads the errors of the same golden image
LADDER_FACTORS = {0: [.5, .125, 1, 2, .03, .125, 1, .06], 1: [128, 32, 512, 1024, 4, 32, 512, 16]}
LADDER_FIRST = {0: 2.0, 1: 1024.0}  # the factor the archive was written at


def golden_image(golden_dir, name, crop):
    img = np.asarray(Image.open(os.path.join(golden_dir, name)))
    return np.ascontiguousarray(img[:crop[1], :crop[0]] if crop else img)


@pytest.mark.parametrize("mode", [0, 1], ids=["shrink_by", "directional"])
@pytest.mark.parametrize("src,dst", PAIRS[:3], ids=[pair_id(*p) for p in PAIRS[:3]])
def test_the_retile_ladders_rungs_as_the_sets(gpu, oracle, golden_dir, src, dst, mode):
    """an image shrunk once at the source block (the archive), the re-tile ladder at eight factors as the sets: the sums equal the
    oracle chain expand(source block) -> shrink(new block, factor) -> expand(new block), and the library's own composition
    pxz_expand_varied_frames_device at the source block + pxz_distortion_varied_frames_device at the new block, bit for bit"""
    import torch
    img = golden_image(golden_dir, "base.png", (200, 150))
    h, w, c = img.shape
    factors = LADDER_FACTORS[mode]
    _, atw, ath, aslots = oracle.shrink_image(img, *src, mode, DOWN, LADDER_FIRST[mode], nthreads=8)
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a).astype(np.int32)).cuda()  # noqa: E731
    ref = (i32(atw), i32(ath), torch.from_numpy(np.ascontiguousarray(aslots)).cuda())
    _, vals, ow, oh, slots = gpu.retile_varied_ladder_frames_device([(w, h)], c, *src, *dst, mode, DOWN, factors, XF, *ref)
    K, T = ow.shape
    tiles = torch.full((K, T, c), POISON64, dtype=torch.int64, device="cuda")
    totals = torch.full((K, 1, c), POISON64, dtype=torch.int64, device="cuda")
    gpu.retile_distortion_varied_device([(w, h)], c, *src, *dst, XF, UF, *ref, ow, oh, slots, out=(tiles, totals))
    torch.cuda.synchronize()
    tiles, totals = tiles.cpu().numpy(), totals.cpu().numpy()
    # the oracle chain
    now = oracle.expand_image(w, h, *src, c, XF, atw, ath, np.ascontiguousarray(aslots))
    for r, k in enumerate(factors):
        _, rw, rh, rs = oracle.shrink_image(now, *dst, mode, DOWN, k, nthreads=8)
        back = oracle.expand_image(w, h, *dst, c, UF, rw, rh, rs)
        exp = tile_sums((now.astype(np.int64) - back.astype(np.int64)) ** 2, w, h, *dst)
        assert (tiles[r] == exp).all(), f"factor {k}: tiles {np.argwhere((tiles[r] != exp).any(axis=1)).ravel()[:10].tolist()}"
        assert (totals[r, 0] == exp.sum(axis=0)).all(), f"factor {k}: totals"
    assert len({tuple(t) for t in totals[:, 0].tolist()}) >= 2 and totals.any()  # the factors spread the errors
    # the library's own composition
    image = torch.zeros(w * h * c, dtype=torch.uint8, device="cuda")
    descs = [(w, h, w * c, 0)]
    gpu.expand_varied_frames_device(descs, c, *src, XF, *ref, image)
    for r in range(K):
        t, tot = gpu.distortion_varied_frames_device(image, *dst, UF, ow[r], oh[r], slots[r], descs=descs, channels=c)
        torch.cuda.synchronize()
        assert (t.cpu().numpy() == tiles[r]).all() and (tot.cpu().numpy() == totals[r]).all(), f"rung {r}: differs from expand + distortion"


@pytest.mark.parametrize("kind", ["alpha", "rgb"])
def test_hand_made_sets_equal_expand_then_distortion(gpu, oracle, kind):
    import torch
    for (src, dst) in PAIRS[:3]:
        b = hand_batch(oracle, src, dst, [(50, 33), (9, 5), (83, 61)], kind)
        descs, at = [], 0
        for (w, h) in b.sizes:
            descs.append((w, h, w * b.c, at))
            at += w * h * b.c
        image = torch.zeros(at, dtype=torch.uint8, device="cuda")
        gpu.expand_varied_frames_device(descs, b.c, *src, 2, *b.dev_ref, image)
        tiles, totals, _, status = run(gpu, b, 2, 3)
        assert status == 0
        for k in range(b.K):
            t, tot = gpu.distortion_varied_frames_device(image, *dst, 3, b.dev_sets[0][k], b.dev_sets[1][k], b.dev_sets[2][k], descs=descs, channels=b.c)
            torch.cuda.synchronize()
            assert (t.cpu().numpy() == tiles[k]).all() and (tot.cpu().numpy() == totals[k]).all(), f"{pair_id(src, dst)} {kind} set {k}"


def test_one_geometry_another_a_trim_and_the_first_again(gpu, oracle):
    a = hand_batch(oracle, (64, 64), (32, 32), [(100, 70)], "alpha")
    z = hand_batch(oracle, (32, 32), (48, 20), [(130, 65), (70, 131)], "rgb")
    check(gpu, a, 2, 3, "first geometry")
    check(gpu, z, 4, 0, "second geometry")
    gpu.trim()
    check(gpu, a, 2, 3, "first geometry after a trim")
    check(gpu, z, 2, 3, "second geometry, other filters")


def test_device_form_errors_write_nothing(gpu, product, oracle):
    import torch
    b = hand_batch(oracle, (64, 64), (32, 32), [(50, 33), (9, 5), (83, 61)], "alpha")
    L, P, descs_of = gpu._L, product.binding.Params, product.binding.image_descs
    geoms = [(w, h, w * 4, 0) for (w, h) in b.sizes]
    ok = P(32, 32, 0, 3, 0.0, 0)
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    def call(code, text=None, geoms=geoms, count=3, channels=4, src=(64, 64), p=ok, xf=2, n_sets=3, missing=()):
        tiles = torch.full((b.K, b.T, 4), POISON64, dtype=torch.int64, device="cuda")
        totals = torch.full((b.K, b.n, 4), POISON64, dtype=torch.int64, device="cuda")
        flags = torch.full((b.n,), POISON32, dtype=torch.int32, device="cuda")
        dev = dict(zip(("rw", "rh", "rs", "w", "h", "s"), b.dev_ref + b.dev_sets))
        args = [None if k in missing else ptr(v) for k, v in dev.items()]
        rc = L.pxz_retile_distortion_varied_device(gpu._h, C.cast(descs_of(geoms), C.c_void_p) if geoms is not None else None, count, channels, *src,
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
    call(INVALID_ARG, p=P(32, 32, 0, 5, 0.0, 0))
    call(INVALID_ARG, p=P(0, 32, 0, 3, 0.0, 0))
    call(INVALID_ARG, "source block", src=(0, 64))
    call(INVALID_ARG, "source block", src=(64, 0))
    for k in ("rw", "rh", "rs", "w", "h", "s", "totals"):
        call(INVALID_ARG, missing=(k,))
    call(INVALID_ARG, "image 1", geoms=[geoms[0], geoms[1] + (1,), geoms[2]])          # reserved
    call(INVALID_ARG, "image 2", geoms=[geoms[0], geoms[1], (0, 61, 0, 0)])            # an empty image
    call(UNSUPPORTED, "image 0", geoms=[(2 ** 24 + 1, 4, 0, 0), geoms[1], geoms[2]])   # a side above 2^24
    call(UNSUPPORTED, p=P(128, 128, 0, 3, 0.0, 0))                                     # two planes of 64 KB and a whole tile staged
    call(UNSUPPORTED, p=P(200, 200, 0, 3, 0.0, 0))
    call(UNSUPPORTED, src=(129, 128))                                                  # a source plane above 64 KB
    call(UNSUPPORTED, "sets", geoms=[(2 ** 14, 2 ** 14, 0, 0)], count=1, p=P(16, 16, 0, 3, 0.0, 0), n_sets=2 ** 13)  # 2^20 tiles in 2^13 sets
    check(gpu, b, 2, 3, "the clean call after the refused ones")


# ---- 4. the host forms ----------------------------------------------------------------------------------------------------------

ARCHIVES = [(64, 3), (32, 4)]                # the files' block and channels: one archive at 64x64 RGB, one at 32x32 RGBA
NEW_BLOCKS = [(32, 32), (64, 64), (48, 20)]  # per archive: a block that divides or equals the files', one that merges, one that straddles
HOST_CASES = [(block, c, nb, mode) for (block, c) in ARCHIVES for nb in NEW_BLOCKS for mode in (0, 1)]
HOST_IDS = [f"{b}x{b}c{c}-to{nb[0]}x{nb[1]}-{['shrink_by', 'directional'][m]}" for (b, c, nb, m) in HOST_CASES]
_retiled = {}


class Retiled:
    """the archive of tests/test_gpu_reshrink_distortion.py (five files written by the oracle at `block`) and, computed once on the
    CPU, what the oracle chain decode -> expand(XF, the files' block) -> shrink(new block, factors[r]) -> encode / expand(UF, new
    block) makes of it: the table and every rung's files"""

    def __init__(self, oracle, block, c, mode, nb):
        a = archive(oracle, block, c, mode)
        self.files, self.decoded, self.factors, self.c, self.mode, self.nb = a.files, a.decoded, a.factors, c, mode, nb
        K, n = len(self.factors), len(self.files)
        if nb == (block, block):
            self.bytes, self.sse, self.rungs = a.bytes, a.sse, a.rungs
            return
        self.bytes, self.sse = np.zeros((K, n), np.uint64), np.zeros((K, n, c), np.uint64)
        self.rungs = [[None] * n for _ in range(K)]
        for i, ref in enumerate(self.decoded):
            h, w = ref.shape[:2]
            for r, k in enumerate(self.factors):
                rv, rw, rh, rs = oracle.shrink_image(ref, *nb, mode, DOWN, k, nthreads=8)
                self.rungs[r][i] = oracle.encode_container(w, h, *nb, c, FILTER_BYTE, rv, None, rw, rh, rs)
                self.bytes[r, i] = len(oracle.encode_container(w, h, *nb, c, 0, rv, None, rw, rh, rs))
                back = oracle.expand_image(w, h, *nb, c, UF, rw, rh, rs)
                self.sse[r, i] = ((ref.astype(np.int64) - back.astype(np.int64)) ** 2).sum(axis=(0, 1))


def retiled(oracle, block, c, mode, nb):
    key = (block, c, mode, nb)
    if key not in _retiled:
        _retiled[key] = Retiled(oracle, block, c, mode, nb)
    return _retiled[key]


@pytest.mark.parametrize("block,c,nb,mode", HOST_CASES, ids=HOST_IDS)
def test_the_table_equals_the_ladder_files_size_query_and_the_oracle(gpu, oracle, block, c, nb, mode):
    a = retiled(oracle, block, c, mode, nb)
    file_bytes, sse = gpu.rate_distortion_retile_files(a.files, *nb, mode, DOWN, XF, UF, a.factors)
    query = gpu.transcode_varied_ladder_files(a.files, *nb, mode, DOWN, a.factors, XF, filter_byte=0, sizes_only=True)
    assert file_bytes.shape == (len(a.factors), len(a.files)) and sse.shape == file_bytes.shape + (c,)
    assert (file_bytes.astype(np.int64) == query).all(), "the bytes column differs from pxz_transcode_varied_ladder_files' size query"
    print(f"block {block} -> {nb} c{c} mode {mode}: bytes\n{file_bytes}\nsse\n{sse.sum(axis=2)}")
    assert (file_bytes == a.bytes).all(), "the bytes column differs from the oracle's files"
    assert (sse == a.sse).all(), "the sse column differs from the oracle's"
    assert sse.any() and max(len(set(file_bytes[:, i].tolist())) for i in range(len(a.files))) >= 3  # the factors spread the files


def expected_choices(a, criterion):
    """the targets and what the rule picks from the oracle's table, with what the table must hold for the comparison to say anything"""
    Kf = len(a.factors)
    targets = targets_from(a.bytes, a.sse, criterion)
    exp_choice, exp_flags = select(a.bytes.tolist(), a.sse.tolist(), criterion, targets)
    total = a.sse.sum(axis=2)
    assert any(0 < r < Kf - 1 for r in exp_choice), "every expected choice is the first or the last rung"
    assert any(any(q != r and a.bytes[q, i] == a.bytes[r, i] and total[q, i] == total[r, i] for q in range(Kf))
               for i, r in enumerate(exp_choice)), "no choice is decided by the lowest index among equal rungs"
    assert any(exp_flags), "no file misses its target"
    return targets, exp_choice, exp_flags


@pytest.mark.parametrize("criterion", [FIT_BYTES, FIT_SSE], ids=["bytes", "sse"])
@pytest.mark.parametrize("block,c,nb,mode", HOST_CASES, ids=HOST_IDS)
def test_fit_files_equal_the_one_factor_transcode_and_todays_detour(gpu, product, oracle, block, c, nb, mode, criterion):
    a = retiled(oracle, block, c, mode, nb)
    n = len(a.files)
    targets, exp_choice, exp_flags = expected_choices(a, criterion)
    files, choice, flags, t_bytes, t_sse = gpu.retile_varied_files_fit(a.files, *nb, mode, DOWN, XF, UF, a.factors, criterion, targets,
                                                                       filter_byte=FILTER_BYTE, want_table=True)
    assert (t_bytes == a.bytes).all() and (t_sse == a.sse).all(), "the table differs from the oracle's"
    h_choice, h_flags = product.fit_select(t_bytes, t_sse, criterion, targets)
    assert choice.tolist() == h_choice.tolist() == exp_choice and flags.tolist() == h_flags.tolist() == exp_flags
    for i in range(n):
        k = a.factors[exp_choice[i]]
        alone = gpu.transcode_varied_files([a.files[i]], *nb, mode, DOWN, k, XF, filter_byte=FILTER_BYTE)[0]
        assert files[i] == alone, f"file {i} at factor {k}: differs from pxz_transcode_varied_files of the file alone"
        assert files[i] == a.rungs[exp_choice[i]][i], f"file {i} at factor {k}: differs from the oracle's file"
    # today's detour: decode to pixels, download, upload, fit from the image at the new block
    images, dflags = gpu.decode_varied_files(a.files, c, block, block, XF)
    assert (dflags == 0).all() and all((x == y).all() for x, y in zip(images, a.decoded))
    d_files, d_choice, d_fl, d_bytes, d_sse = gpu.encode_varied_images_fit(images, *nb, mode, DOWN, UF, a.factors, criterion, targets,
                                                                           filter_byte=FILTER_BYTE, want_table=True)
    assert d_files == files and d_choice.tolist() == choice.tolist() and d_fl.tolist() == flags.tolist()
    assert (d_bytes == t_bytes).all() and (d_sse == t_sse).all()
    if nb == (block, block):  # equal blocks: exactly the existing form
        s_files, s_choice, s_fl, s_bytes, s_sse = gpu.transcode_varied_files_fit(a.files, *nb, mode, DOWN, XF, UF, a.factors, criterion, targets,
                                                                                 filter_byte=FILTER_BYTE, want_table=True)
        assert s_files == files and s_choice.tolist() == choice.tolist() and s_fl.tolist() == flags.tolist()
        assert (s_bytes == t_bytes).all() and (s_sse == t_sse).all()
        e_bytes, e_sse = gpu.rate_distortion_varied_files(a.files, *nb, mode, DOWN, XF, UF, a.factors)
        r_bytes, r_sse = gpu.rate_distortion_retile_files(a.files, *nb, mode, DOWN, XF, UF, a.factors)
        assert (e_bytes == r_bytes).all() and (e_sse == r_sse).all()


@pytest.mark.parametrize("criterion", [FIT_BYTES, FIT_SSE], ids=["bytes", "sse"])
@pytest.mark.parametrize("block,c,nb,mode", HOST_CASES, ids=HOST_IDS)
def test_the_tile_form_equals_todays_detour(gpu, product, oracle, block, c, nb, mode, criterion):
    a = retiled(oracle, block, c, mode, nb)
    n = len(a.files)
    q = a.bytes.astype(np.int64) if criterion == FIT_BYTES else a.sse.sum(axis=2).astype(np.int64)
    for name, gf, targets in [("every file its own group", None, targets_from(a.bytes, a.sse, criterion)),
                              ("one group over all", [0, n], [int(np.sort(q.sum(axis=1))[len(a.factors) // 2])])]:
        got = gpu.retile_varied_files_fit_tiles(a.files, *nb, mode, DOWN, XF, UF, a.factors, criterion, targets, group_first=gf,
                                                filter_byte=FILTER_BYTE)
        want = gpu.encode_varied_images_fit_tiles(a.decoded, *nb, mode, DOWN, UF, a.factors, criterion, targets, group_first=gf,
                                                  filter_byte=FILTER_BYTE)
        assert got[0] == want[0], f"{name}: the files differ from decode + pxz_encode_varied_images_fit_tiles"
        for k, what in enumerate(("tile_choice", "lambda", "bytes", "sse", "flags"), start=1):
            assert got[k].tolist() == want[k].tolist(), f"{name}: {what}"
        assert len(got[1]) == sum(len(tile_rects(w, h, *nb)) for (w, h) in ARCHIVE_SIZES)
        # and the groups' totals are those of the files written, against what the input files decode to
        decoded, _ = gpu.decode_varied_files(got[0], c, *nb, UF)
        runs = [(i, i + 1) for i in range(n)] if gf is None else [(0, n)]
        for g, (i0, i1) in enumerate(runs):
            assert int(got[3][g]) == sum(len(f) for f in got[0][i0:i1]), f"{name} group {g}: group_bytes"
            sse = sum(int(((x.astype(np.int64) - y.astype(np.int64)) ** 2).sum()) for x, y in zip(a.decoded[i0:i1], decoded[i0:i1]))
            assert int(got[4][g]) == sse, f"{name} group {g}: group_sse"
        if nb == (block, block):
            same = gpu.transcode_varied_files_fit_tiles(a.files, *nb, mode, DOWN, XF, UF, a.factors, criterion, targets, group_first=gf,
                                                        filter_byte=FILTER_BYTE)
            assert same[0] == got[0] and all(x.tolist() == y.tolist() for x, y in zip(same[1:], got[1:])), f"{name}: differs from the existing form"


# ---- 5. size query and errors ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("block,c,nb", [(64, 3, (32, 32)), (32, 4, (48, 20))], ids=["dividing", "straddling"])
def test_size_query_then_exact_capacity(gpu, product, oracle, block, c, nb):
    a = retiled(oracle, block, c, 0, nb)
    targets = targets_from(a.bytes, a.sse, FIT_BYTES)
    files, choice, flags = gpu.retile_varied_files_fit(a.files, *nb, 0, DOWN, XF, UF, a.factors, FIT_BYTES, targets, filter_byte=FILTER_BYTE)
    total = sum(len(f) for f in files)
    for out in (np.zeros(0, np.uint8), np.full(total - 1, POISON, np.uint8)):
        with pytest.raises(product.PxzError) as e:
            gpu.retile_varied_files_fit(a.files, *nb, 0, DOWN, XF, UF, a.factors, FIT_BYTES, targets, filter_byte=FILTER_BYTE, out=out)
        assert e.value.code == BUFFER_TOO_SMALL and e.value.needed == total
        assert (e.value.choice == choice).all() and (e.value.fit_flags == flags).all()
        assert (e.value.table[0] == a.bytes).all() and (e.value.table[1] == a.sse).all()
        assert (out == POISON).all(), "a call that was short of room wrote to out"
    exact = np.full(total + 16, POISON, np.uint8)
    got, _, _ = gpu.retile_varied_files_fit(a.files, *nb, 0, DOWN, XF, UF, a.factors, FIT_BYTES, targets, filter_byte=FILTER_BYTE, out=exact[:total])
    assert got == files and (exact[total:] == POISON).all()
    # the tile form (a rung per tile: other files, another total)
    whole = gpu.retile_varied_files_fit_tiles(a.files, *nb, 0, DOWN, XF, UF, a.factors, FIT_BYTES, targets, filter_byte=FILTER_BYTE)
    total = sum(len(f) for f in whole[0])
    for out in (np.zeros(0, np.uint8), np.full(total - 1, POISON, np.uint8)):
        with pytest.raises(product.PxzError) as e:
            gpu.retile_varied_files_fit_tiles(a.files, *nb, 0, DOWN, XF, UF, a.factors, FIT_BYTES, targets, filter_byte=FILTER_BYTE, out=out)
        assert e.value.code == BUFFER_TOO_SMALL and e.value.needed == total
        assert (e.value.tile_choice == whole[1]).all() and all((x == y).all() for x, y in zip(e.value.groups, whole[2:]))
        assert (out == POISON).all(), "a call that was short of room wrote to out"
    exact = np.full(total + 16, POISON, np.uint8)
    got = gpu.retile_varied_files_fit_tiles(a.files, *nb, 0, DOWN, XF, UF, a.factors, FIT_BYTES, targets, filter_byte=FILTER_BYTE, out=exact[:total])
    assert got[0] == whole[0] and (exact[total:] == POISON).all()


class RawFit:
    """pxz_retile_varied_files_fit and pxz_rate_distortion_retile_files through ctypes, every output poisoned"""

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
        return self.gpu._L.pxz_retile_varied_files_fit(*head, self.criterion, None if null_targets else ptr(self.targets), FILTER_BYTE, ptr(self.out),
                                                       self.out.size, ptr(self.offs), ptr(self.choice), ptr(self.flags), ptr(self.t_bytes),
                                                       ptr(self.t_sse))

    def table(self, null_factors=False):
        head, ptr = self.head(null_factors)
        return self.gpu._L.pxz_rate_distortion_retile_files(*head, ptr(self.t_bytes), ptr(self.t_sse))

    def untouched(self):
        return bool((self.offs == U64).all() and (self.choice == POISON32).all() and (self.flags == POISON32).all() and
                    (self.t_bytes == U64).all() and (self.t_sse == U64).all() and (self.out == POISON).all())


@pytest.mark.parametrize("block,c,nb", [(64, 3, (32, 32)), (32, 4, (48, 20))], ids=["dividing", "straddling"])
def test_host_form_errors_write_nothing(gpu, product, oracle, block, c, nb):
    a = retiled(oracle, block, c, 0, nb)

    def refused(code, text=None, files=a.files, new_block=nb, factors=a.factors, both=True, **kw):
        for form in (("fit", "table") if both else ("fit",)):
            raw = RawFit(gpu, product, files, new_block, 0, factors)
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
    refused(INVALID_ARG, new_block=(0, 32))
    # a malformed file: all or nothing, and the image is named
    cut = list(a.files)
    cut[3] = cut[3][:len(cut[3]) - 9]
    refused(INVALID_ARG, "image 3", files=cut)
    refused(INVALID_ARG, "image 2", files=a.files[:2] + [a.files[2][:10]] + a.files[3:])
    # files of another channel count and block size among them
    other = archive(oracle, 96 - block, 7 - c, 0)
    refused(INVALID_ARG, "image 1", files=[a.files[0], other.files[1]])
    # the tile form: all or nothing as well
    out = np.full(1 << 20, POISON, np.uint8)
    with pytest.raises(product.PxzError) as e:
        gpu.retile_varied_files_fit_tiles(cut, *nb, 0, DOWN, XF, UF, a.factors, FIT_BYTES, [U64] * len(cut), out=out)
    assert e.value.code == INVALID_ARG and "image 3" in str(e.value) and (out == POISON).all()
    # and the handle still works
    file_bytes, sse = gpu.rate_distortion_retile_files(a.files, *nb, 0, DOWN, XF, UF, a.factors)
    assert (file_bytes == a.bytes).all() and (sse == a.sse).all()
