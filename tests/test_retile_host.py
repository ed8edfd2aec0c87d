"""Re-tile of stored tiles (pxz_retile_varied_frames_device, and pxz_transcode_varied_files with another block size), the part
that needs no GPU: the symbols, the LDS footprint of the kernel from its own layout function, and the inputs of
tests/test_gpu_retile.py -- built here, with their expected results from the oracle composition

    oracle.decode_container -> oracle.expand_image(source block, expand_filter) -> oracle.shrink_image(destination block, ...)

and held against the conditions that make them worth running (enough source tiles stored small and stored full, enough
destination tiles that straddle source tiles of different stored sizes or lie inside one, enough that come out reduced and
full), so that no GPU test passes on inputs that exercise nothing."""
import functools
import os
import subprocess

import numpy as np
import pytest

from test_reshrink_host import (DIRECTIONAL, FILTER_PAIRS, LANCZOS3, LDS_PER_CU, SHRINK_BY, factors_a, full_sizes)
from test_varied_decode_host import draw_tiles

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pixlzr_hip.h")

# (source block, destination block): what a destination tile is made of
SPLIT = [((32, 32), (16, 16)), ((64, 64), (32, 32))]  # it lies inside one source tile
MERGE = [((16, 16), (32, 32)), ((32, 32), (64, 64))]  # it covers four whole source tiles
STRADDLE = [((32, 32), (48, 20)), ((48, 20), (32, 32)), ((37, 61), (16, 16)), ((16, 16), (37, 61))]
TINY = [((3, 5), (4, 4)), ((5, 3), (3, 5))]           # 3x5 -> 4x4 RGB (45-byte slots), 5x3 -> 3x5 RGBA
SAME = [((32, 32), (32, 32))]
PAIRS = SPLIT + MERGE + STRADDLE + TINY + SAME
# the pairs that run the five filters on both sides and Nearest in / Lanczos3 out; Lanczos3 elsewhere
ALL_FILTERS = [((32, 32), (16, 16)), ((16, 16), (32, 32)), ((32, 32), (48, 20)), ((48, 20), (32, 32))]
# the pairs pxz_retile_lds_bytes must admit, in both modes and with all five filters (the footprint has no channel count)
PROMISED = [(s, d) for s in [(16, 16), (32, 32), (64, 64)] for d in [(16, 16), (32, 32), (64, 64)]] + \
           [((32, 32), (48, 20)), ((48, 20), (32, 32)), ((37, 61), (16, 16)), ((16, 16), (37, 61))]


def channels_of(pair):
    return {TINY[0]: (3,), TINY[1]: (4,)}.get(pair, (3, 4))


CASES = [(fam, mode, pair, c) for fam in "AB" for mode in (SHRINK_BY, DIRECTIONAL) for pair in PAIRS for c in channels_of(pair)]


def case_id(case):
    fam, mode, ((sw, sh), (dw, dh)), c = case
    return f"{fam}-{'by' if mode == SHRINK_BY else 'dir'}-{sw}x{sh}to{dw}x{dh}-c{c}"


def filter_pairs(pair):
    return FILTER_PAIRS if pair in ALL_FILTERS else [(LANCZOS3, LANCZOS3)]


# Family A: (the factor a file was written with at the source block, the one it is shrunk at again at the destination block).
# The start is factors_a of tests/test_reshrink_host.py for the source block; a batch that missed a condition there has its own
# pair here -- the factor pair is changed, never the threshold.  What each missed at the start pair is said beside it.
FACTORS_A = {
    # shrink_by, RGBA (every second image DIST_ALPHA): under a third of the source tiles stored small at 1.0 -> 0.5
    (SHRINK_BY, ((32, 32), (16, 16)), 4): (0.5, 0.25),
    (SHRINK_BY, ((16, 16), (32, 32)), 4): (0.5, 0.25),
    (SHRINK_BY, ((32, 32), (64, 64)), 4): (0.5, 0.25),
    (SHRINK_BY, ((48, 20), (32, 32)), 4): (0.5, 0.25),
    (SHRINK_BY, ((32, 32), (32, 32)), 4): (0.5, 0.25),
    (SHRINK_BY, ((32, 32), (48, 20)), 4): (0.6, 0.3),     # (at 0.5 -> 0.25 under a tenth of the 48x20 tiles stay full)
    (SHRINK_BY, ((16, 16), (37, 61)), 4): (0.6, 0.3),     # (the same for the 37x61 tiles)
    (SHRINK_BY, ((37, 61), (16, 16)), 4): (0.42, 0.42),   # (small sources and full results only meet at one factor for both)
    # shrink_by, RGB: 13 % of the 64x64 and 37x61 source tiles stored small at 2.0 -> 1.0
    (SHRINK_BY, ((64, 64), (32, 32)), 3): (1.0, 0.5),
    (SHRINK_BY, ((37, 61), (16, 16)), 3): (1.0, 0.5),
    # 16x16 -> 32x32: neighbouring 16x16 tiles of the smooth frames mostly share a stored size; 3-9 % of the destination tiles
    # covered different ones at the start pairs
    (SHRINK_BY, ((16, 16), (32, 32)), 3): (0.7, 0.35),
    (DIRECTIONAL, ((16, 16), (32, 32)), 3): (20.0, 10.0),
    (DIRECTIONAL, ((16, 16), (32, 32)), 4): (20.0, 10.0),
    # the tiny pairs: tiles of 15 pixels are stored small or full nearly all at once (1-8 % stored full at the start pairs); the
    # window in which both kinds, and both kinds of result, reach their share is one factor wide in three of the four
    (SHRINK_BY, ((3, 5), (4, 4)), 3): (12.0, 12.0),
    (SHRINK_BY, ((5, 3), (3, 5)), 4): (8.0, 4.0),
    (DIRECTIONAL, ((3, 5), (4, 4)), 3): (300.0, 300.0),
    (DIRECTIONAL, ((5, 3), (3, 5)), 4): (300.0, 300.0),
}


def retile_factors_a(mode, pair, c):
    return FACTORS_A.get((mode, pair, c), factors_a(mode, pair[0], c))


# Family B: drawn tiles.  FACTOR_B of tests/test_reshrink_host.py (1.0 / 8.0) is the start; at 1.0 no destination tile of the
# shrink_by batches came out reduced (a tile of random bytes keeps its size, and so does every destination tile that has a part of
# one), so shrink_by takes the factor at which a tenth and more come out reduced and a tenth and more full.
FACTORS_B = {SHRINK_BY: {3: 0.21, 4: 0.125}, DIRECTIONAL: {3: 8.0, 4: 8.0}}
FACTORS_B_OF = {
    # (at 0.21 nearly every 32x32 / 16x16 tile cut out of these oblong source tiles came out reduced: 2 of 36 and 12 of 123 full)
    (SHRINK_BY, ((48, 20), (32, 32)), 3): 0.25,
    (SHRINK_BY, ((37, 61), (16, 16)), 3): 0.25,
    (DIRECTIONAL, ((16, 16), (37, 61)), 3): 6.0,  # (8 % of the 26 destination tiles reduced on exactly one axis at 8.0)
}


def retile_factor_b(mode, pair, c):
    return FACTORS_B_OF.get((mode, pair, c), FACTORS_B[mode][c])


def retile_sizes(src, dst, mode, family):
    """5-9 images of sides <= 300, as batch_sizes of tests/test_reshrink_host.py builds them, for both blocks of the pair: the
    smallest image the mode takes; for each block an image one pixel short of it and one a pixel past it on both axes
    (directional: two pixels past -- the call refuses 1-px edge tiles); and three images of several tiles, sized from the larger
    block of each axis and ragged against both grids (a side that is a multiple of either block grows until it is none).  In directional mode a side that would leave a 1-px edge tile against
    either grid grows by a pixel (the oracle's writer panics on the source grid's, the call refuses the destination grid's)."""
    past = 1 if mode == SHRINK_BY else 2
    sizes = [(1, 1) if mode == SHRINK_BY else (2, 2)]
    for (bw, bh) in (src, dst):
        sizes += [(bw - 1, bh - 1), (bw + past, bh + past)]
    bw, bh = max(src[0], dst[0]), max(src[1], dst[1])
    if family == "A":
        big = [(min(5 * bw + 3, 290), min(4 * bh + 5, 290)), (min(4 * bw + 7, 290 - bw // 4), min(5 * bh + 2, 290 - bh // 3)), (3 * bw + 9, 2 * bh + 3)]
    else:
        big = [(2 * bw + 3, bh + 6), (bw + 5, 3 * bh + 2), (3 * bw + 1, bh + 1)]

    def grown(side, blocks, avoid):
        while any(side % b in avoid for b in blocks):
            side += 1
        return side
    # ragged: a side that is a multiple of either block grows until it is none
    sizes += [(grown(w, (src[0], dst[0]), (0,)), grown(h, (src[1], dst[1]), (0,))) for (w, h) in big]
    if mode == DIRECTIONAL:
        sizes = [(grown(w, (src[0], dst[0]), (1,)), grown(h, (src[1], dst[1]), (1,))) for (w, h) in sizes]
        sizes[-3:] = [(grown(w, (src[0], dst[0]), (0, 1)), grown(h, (src[1], dst[1]), (0, 1))) for (w, h) in sizes[-3:]]
    sizes = list(dict.fromkeys(sizes))
    assert 5 <= len(sizes) <= 9 and all(1 <= w <= 300 and 1 <= h <= 300 for (w, h) in sizes), sizes
    return sizes


def covering(w, h, src, dst):
    """per destination tile of a w x h image, row-major: the source tiles (indices into the source grid) that cover it, as
    (columns, rows) ranges"""
    (sw, sh), (dw, dh) = src, dst
    out = []
    for y0 in range(0, h, dh):
        for x0 in range(0, w, dw):
            x1, y1 = min(x0 + dw, w), min(y0 + dh, h)
            out.append((range(x0 // sw, (x1 - 1) // sw + 1), range(y0 // sh, (y1 - 1) // sh + 1), (x0, y0, x1, y1)))
    return out


class RetileCase:
    """one batch of stored tiles at the source block (as files of the oracle's writer and as the oracle's reader returns them)
    and what the oracle composition makes of them at the destination block"""

    def __init__(self, oracle, family, mode, pair, c, expand_filter, filt, sizes=None, factor=None):
        from oracle import binding as ob
        self.src, self.dst = pair
        (sw, sh), (dw, dh) = pair
        self.family, self.mode, self.pair, self.c, self.expand_filter, self.filt = family, mode, pair, c, expand_filter, filt
        self.sizes = sizes if sizes is not None else retile_sizes(self.src, self.dst, mode, family)
        rng = np.random.default_rng(sw * 131 + sh * 7 + dw * 17 + dh * 3 + c + 1000 * mode)
        self.files = []
        if family == "A":
            f1, self.factor = retile_factors_a(mode, pair, c)
            for k, (w, h) in enumerate(self.sizes):
                dist = ob.DIST_ALPHA if c == 4 and k % 2 == 1 else ob.DIST_OPAQUE
                img = oracle.synth_frame(w, h, c, frame_index=k, dist=dist)
                vals, tw, th, slots = oracle.shrink_image(img, sw, sh, mode, filt, f1)
                self.files.append(oracle.encode_container(w, h, sw, sh, c, 0, vals, None, tw, th, slots))
        else:
            self.factor = retile_factor_b(mode, pair, c)
            counts = [-(-w // sw) * -(-h // sh) for (w, h) in self.sizes]
            dealt = np.split(rng.permutation(np.arange(sum(counts)) % 3), np.cumsum(counts)[:-1])  # FULL / HALVED / ANY, evenly
            for (w, h), cl in zip(self.sizes, dealt):
                vals, tw, th, slots, _ = draw_tiles(rng, w, h, sw, sh, c, cl)
                self.files.append(oracle.encode_container(w, h, sw, sh, c, 0, vals, None, tw, th, slots))
        if factor is not None:
            self.factor = factor
        # the oracle composition, image by image
        self.inputs, self.expected, self.src_full, self.dst_full = [], [], [], []
        for raw, (w, h) in zip(self.files, self.sizes):
            d = oracle.decode_container(raw)
            slots = np.ascontiguousarray(d["slots"][:, : sw * sh * c])
            self.inputs.append((d["values"], d["tw"], d["th"], slots))
            img = oracle.expand_image(w, h, sw, sh, c, expand_filter, d["tw"], d["th"], slots)
            self.expected.append(oracle.shrink_image(img, dw, dh, mode, filt, self.factor))
            self.src_full.append(full_sizes(w, h, sw, sh))
            self.dst_full.append(full_sizes(w, h, dw, dh))

    def cat(self, which, k):
        return np.concatenate([x[k] for x in which])

    def counts(self):
        (sw, sh), (dw, dh) = self.pair
        tw, th = self.cat(self.inputs, 1), self.cat(self.inputs, 2)
        sfw, sfh = self.cat(self.src_full, 0), self.cat(self.src_full, 1)
        ow, oh = self.cat(self.expected, 1), self.cat(self.expected, 2)
        dfw, dfh = self.cat(self.dst_full, 0), self.cat(self.dst_full, 1)
        two_x = two_y = mixed = inside = 0
        for (w, h), inp in zip(self.sizes, self.inputs):
            cols = -(-w // sw)
            for (cs, rs, (x0, y0, x1, y1)) in covering(w, h, self.src, self.dst):
                two_x += len(cs) >= 2
                two_y += len(rs) >= 2
                stored = {(int(inp[1][r * cols + q]), int(inp[2][r * cols + q])) for r in rs for q in cs}
                mixed += len(stored) >= 2
                # strictly inside: one source tile covers it, and that tile is larger than it
                fw, fh = min(sw, w - cs[0] * sw), min(sh, h - rs[0] * sh)
                inside += len(cs) == 1 and len(rs) == 1 and (x1 - x0) * (y1 - y0) < fw * fh
        return dict(n_src=tw.size, n_dst=ow.size, src_small=int(((tw < sfw) | (th < sfh)).sum()), src_full=int(((tw == sfw) & (th == sfh)).sum()),
                    two_x=two_x, two_y=two_y, mixed=mixed, inside=inside, reduced=int(((ow < dfw) | (oh < dfh)).sum()),
                    full=int(((ow == dfw) & (oh == dfh)).sum()), one=int(((ow < dfw) != (oh < dfh)).sum()))

    def check_conditions(self):
        k = self.counts()
        what = f"{case_id((self.family, self.mode, self.pair, self.c))} filters {self.expand_filter}/{self.filt}: {k}"
        ns, nd = k["n_src"], k["n_dst"]
        assert k["src_small"] * 3 >= ns, what       # source tiles that are expanded
        assert k["src_full"] * 10 >= ns, what       # source tiles that are cloned in
        if self.pair in STRADDLE + MERGE + TINY:
            assert k["two_x"] * 10 >= nd, what      # destination tiles over at least two source tiles on x
            assert k["two_y"] * 10 >= nd, what      # ... on y
            assert k["mixed"] * 10 >= nd, what      # ... over source tiles of different stored sizes
        if self.pair in SPLIT:
            assert k["inside"] * 2 >= nd, what      # destination tiles strictly inside one source tile
        assert k["reduced"] * 10 >= nd, what        # destination tiles that come out reduced
        assert k["full"] * 10 >= nd, what           # ... and full (clone out)
        if self.family == "B" and self.mode == DIRECTIONAL:
            assert k["one"] * 10 >= nd, what        # reduced on exactly one axis
        # the images: the smallest, one short of and one past each block, several-tile images ragged against both grids
        (sw, sh), (dw, dh) = self.pair
        past = 1 if self.mode == SHRINK_BY else 2
        assert ((1, 1) if self.mode == SHRINK_BY else (2, 2)) in self.sizes, what
        for (bw, bh) in self.pair:
            if self.mode == SHRINK_BY:
                assert (bw - 1, bh - 1) in self.sizes and (bw + 1, bh + 1) in self.sizes, what
            else:  # (a side may have grown by a pixel off a 1-px edge against the other grid)
                assert any(bw - 1 <= w <= bw and bh - 1 <= h <= bh and (w, h) != (bw, bh) for (w, h) in self.sizes), what
                assert any(bw + past <= w <= bw + past + 1 and bh + past <= h <= bh + past + 1 for (w, h) in self.sizes), what
        several = [(w, h) for (w, h) in self.sizes if w > max(sw, dw) and h > max(sh, dh)]
        ragged = [(w, h) for (w, h) in several if all(w % b for b in (sw, dw)) and all(h % b for b in (sh, dh))]
        assert len(ragged) >= 2, what


@functools.lru_cache(maxsize=None)
def cached_retile_case(family, mode, pair, c, expand_filter, filt):
    """the batches are built once and shared, unchanged, by the tests that need them"""
    from oracle import binding
    binding.build()
    return RetileCase(binding, family, mode, pair, c, expand_filter, filt)


# ---- 1. symbols -----------------------------------------------------------------------------------------------------------

def test_symbols_are_exported_declared_and_bound(product):
    """fails before the re-tile exists"""
    names = ["pxz_retile_varied_frames_device", "pxz_retile_lds_bytes"]
    lib = product.load_library()
    text = open(HEADER).read()
    for name in names:
        assert hasattr(lib, name), name
        assert f"int {name}(" in text, name
        assert name in product.EXPORTED_SYMBOLS, name
    out = subprocess.run(["nm", "-D", "--defined-only", product.library_path()], capture_output=True, text=True, check=True).stdout
    for name in names:
        assert f" T {name}" in out, name
    assert hasattr(product.Handle, "retile_varied_frames_device") and hasattr(product, "retile_lds_bytes")


# ---- 2. footprint ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", [SHRINK_BY, DIRECTIONAL])
@pytest.mark.parametrize("filt", range(5))
def test_lds_footprint_admits_the_promised_pairs(product, mode, filt):
    """the function the launch sizes its LDS with (no channel count: an image is a dword per pixel for RGB and RGBA)"""
    wdw = 5  # dwords of a staged window at most: 1 + ceil(7 taps / 2) -- an up-scaling window has at most 7 taps
    for (src, dst) in PROMISED:
        got = product.retile_lds_bytes(*src, *dst, mode, filt)
        d = (dst[0] * dst[1] * 4 + 15) & ~15
        tables = 14336 if mode == SHRINK_BY else 0
        # at least the image and its other plane (shrink_by: the detector's 16 KB of planes); at most the image and an assembly of a
        # whole source tile staged, as large an intermediate, and the windows of both source axes
        floor = tables + d + max(d, 16384 if mode == SHRINK_BY else 0)
        roof = tables + d + max(d, 16384, 2 * (src[0] * src[1] * 4 + 16) + (src[0] + src[1] + 3) * wdw * 4)
        assert floor <= got <= roof <= LDS_PER_CU, (src, dst, got)
    # the default pair of the reference CLI, and 32x32 -> 48x20, as many blocks per CU as varied_kernel runs at those tiles
    assert product.retile_lds_bytes(64, 64, 32, 32, mode, filt) <= LDS_PER_CU // 4
    assert product.retile_lds_bytes(32, 32, 48, 20, mode, filt) <= LDS_PER_CU // 4
    assert product.retile_lds_bytes(32, 32, 64, 64, mode, filt) <= LDS_PER_CU // 3
    # beyond the CU: a plane above 64 KB on either side; two blocks that leave parts as large as a 64 KB source tile; a one-row block
    for (src, dst) in [((129, 128), (129, 128)), ((128, 129), (16, 16)), ((16, 16), (129, 128)), ((128, 128), (128, 128)), ((128, 128), (128, 127)),
                       ((16384, 1), (16384, 1)), ((1, 16384), (1, 16384))]:
        assert product.retile_lds_bytes(*src, *dst, mode, filt) > LDS_PER_CU, (src, dst)
    for (src, dst) in [((64, 64), (128, 128)), ((128, 128), (16, 16)), ((128, 128), (64, 64)), ((1, 1), (1, 1)), ((256, 16), (16, 256))]:
        assert product.retile_lds_bytes(*src, *dst, mode, filt) <= LDS_PER_CU, (src, dst)


def test_lds_footprint_refuses_bad_arguments(product):
    for args in [(0, 16, 16, 16, 0, 0), (16, 0, 16, 16, 0, 0), (16, 16, 0, 16, 0, 0), (16, 16, 16, 0, 0, 0), (16, 16, 16, 16, 2, 0), (16, 16, 16, 16, 0, 5)]:
        with pytest.raises(product.PxzError) as e:
            product.retile_lds_bytes(*args)
        assert e.value.code == -1
    assert product.load_library().pxz_retile_lds_bytes(16, 16, 16, 16, 0, 0, None) == -1


# ---- 3. the inputs of the GPU tests ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_gpu_inputs_meet_their_conditions(oracle, case):
    fam, mode, pair, c = case
    for (xf, sf) in filter_pairs(pair):
        batch = cached_retile_case(fam, mode, pair, c, xf, sf)
        assert 5 <= len(batch.sizes) <= 9
        batch.check_conditions()


def test_tiny_slots_meet_every_alignment(oracle):
    """3x5 RGB: source slot t starts at a multiple of 45 bytes -- every alignment of a dword; 5x3 and 3x5 RGBA: 60 bytes -- every
    dword alignment of 16 bytes"""
    rgb = cached_retile_case("B", SHRINK_BY, TINY[0], 3, LANCZOS3, LANCZOS3)
    assert {(t * 45) % 4 for t in range(sum(x[1].size for x in rgb.inputs))} == {0, 1, 2, 3}
    rgba = cached_retile_case("B", SHRINK_BY, TINY[1], 4, LANCZOS3, LANCZOS3)
    assert {(t * 60) % 16 for t in range(sum(x[1].size for x in rgba.inputs))} == {0, 4, 8, 12}


# ---- 4. what the staging's bound rests on ---------------------------------------------------------------------------------

@pytest.mark.parametrize("filt", range(5))
def test_windows_of_a_part_span_what_the_layout_reserves(product, filt):
    """retile_lds reserves, per axis, n + 2 (wdw - 1) + 2 stored samples for a part of n wanted samples (wdw = 1 + ceil(widest
    window / 2) dwords).  The up-scaling tables themselves, every (full size, stored size) of a selection of sides and every
    run of n consecutive samples: the window starts ascend, the window ends ascend, and from the first sample's start to the
    last one's end there are at most n + (widest window) stored samples -- two fewer than reserved, at the least."""
    for full in list(range(2, 41)) + [48, 61, 64, 128]:
        for stored in range(1, full):
            starts, sizes, _, _ = product.axis_table(stored, full, filt)
            starts = starts.astype(np.int64)
            ends = starts + (sizes.astype(np.int64) if filt else 1)
            widest = int((ends - starts).max())
            wdw = 1 + (widest + 1) // 2
            assert (np.diff(starts) >= 0).all() and (np.diff(ends) >= 0).all(), (full, stored)
            assert starts[0] >= 0 and ends[-1] <= stored, (full, stored)
            for n in range(1, full + 1):
                span = int((ends[n - 1:] - starts[: full - n + 1]).max())
                assert span <= n + widest <= n + 2 * (wdw - 1) + 2, (full, stored, n, span, widest)
