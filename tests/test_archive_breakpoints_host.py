"""The level decision at its breakpoints on the ladder and archive kernels, the part that needs no GPU: the inputs of
tests/test_gpu_archive_breakpoints.py -- built here, once, through cached builders that module imports -- with their expected
results from the oracle, and held against the conditions that make them worth running.

The re-shrink, the re-tile and their ladders decide a destination tile's size on the EXPANSION of stored tiles, so a tile that
sits on a breakpoint has to get there through a file:

  directional  the breakpoint images of tests/test_gpu_level_breakpoints.py (integer gradient sums S - 1, S, S + 1 for every flip
               S of every tile class on either axis), laid out on the DESTINATION grid and cut into stored tiles at the SOURCE
               block by the oracle at a factor that keeps every tile full.  A full tile is a clone on both sides, so the oracle's
               expansion is the image, byte for byte, and the expected result is the oracle's shrink of the image itself;
  Oklab        noise frames written by the oracle at shrink_by 1.0 (tiles stored at 32, 16, 8, ... px), read back and expanded by
               the oracle; the factors are searched on the full destination tiles of the DECODED images, those over reduced source
               tiles first, so that a parsed value equal to a threshold's bit pattern comes out of the expand path.

Nothing here comes from the product: flips, thresholds and factors are the oracle's, by the builders of
tests/test_gpu_level_breakpoints.py."""
import functools

import numpy as np
import pytest

from test_gpu_level_breakpoints import (EDGE_H, EDGE_W, FRAME_FACTOR, LANCZOS3, NEAREST, bits, build_tile, factor_onto, flips, lay_out,
                                        levels_of, nearest_attainable, oklab_frame, oracle_never_reaches, parsed, threshold_bits, with_form)
from test_gpu_reshrink import cat_expected
from test_reshrink_host import DIRECTIONAL, SHRINK_BY, full_sizes
from test_retile_host import covering

SHAPES = ((2, 2), (3, 1), (1, 3))                 # full tiles across and down, of the three image shapes of a directional batch
FRAME_FACTORS = (16.0, -3.0, 2.0)                 # the factors whose flips the directional images sit on
CALL_FACTORS = (16.0, -3.0, 2.0, 1e-3, -1e-3)     # the factors of a call; the sentinels ride on the frames of 16 (FRAME_FACTOR)
KEEP_FULL = -1e-3                                 # the writing factor of the directional archives: every tile is stored full
OKLAB_WRITTEN_AT = 1.0                            # the writing factor of the Oklab archives

# (source block, destination block, channels)
DIR_RESHRINK = [((32, 32), (32, 32), 3), ((32, 32), (32, 32), 4), ((24, 24), (24, 24), 3), ((24, 24), (24, 24), 4)]
DIR_RETILE = [((64, 64), (32, 32), 3), ((64, 64), (32, 32), 4),   # the destination block divides the source block
              ((16, 16), (32, 32), 4),                             # tiles merge
              ((48, 20), (32, 32), 4),                             # tiles straddle
              ((32, 32), (24, 24), 4)]
DIR_VARIED = [((32, 32), 4), ((32, 32), 3), ((24, 24), 4), ((24, 24), 3)]   # the varied ladder, from the images themselves
OKLAB_RESHRINK = [((32, 32), (32, 32), 4), ((32, 32), (32, 32), 3), ((24, 24), (24, 24), 4)]  # (and the varied ladder on their images)
OKLAB_RETILE = [((64, 64), (32, 32), 4), ((64, 64), (32, 32), 3), ((32, 32), (24, 24), 4)]


def archive_id(case):
    return "-".join(f"{v[0]}x{v[1]}" if isinstance(v, tuple) else f"c{v}" for v in case)


def the_oracle():
    from oracle import binding
    binding.build()
    binding.lib()
    return binding


def write_and_read(oracle, img, src, mode, factor):
    """the image as a file of the oracle's writer at block `src`, and what the oracle's reader makes of it
    -> (file, (values, w, h, slots) of the stored tiles, the oracle's Lanczos3 expansion)"""
    (sw, sh), (h, w, c) = src, img.shape
    vals, tw, th, slots = oracle.shrink_image(np.ascontiguousarray(img), sw, sh, mode, LANCZOS3, factor)
    raw = oracle.encode_container(w, h, sw, sh, c, 0, vals, None, tw, th, slots)
    d = oracle.decode_container(raw)
    stored = (d["values"], d["tw"], d["th"], np.ascontiguousarray(d["slots"][:, : sw * sh * c]))
    return raw, stored, oracle.expand_image(w, h, sw, sh, c, LANCZOS3, d["tw"], d["th"], stored[3])


class Archive:
    """a batch of images as stored tiles at the block `src`: .images (what the oracle expands the tiles to), .sizes, .files,
    .inputs (per image: values, w, h, slots), .src_full (per image: full w, h of every source tile)"""

    def __init__(self, src, dst, c):
        self.src, self.dst, self.c = src, dst, c
        self.pair = (src, dst)
        self.images, self.sizes, self.files, self.inputs, self.src_full = [], [], [], [], []

    def add(self, raw, stored, image):
        h, w = image.shape[:2]
        self.images.append(image)
        self.sizes.append((w, h))
        self.files.append(raw)
        self.inputs.append(stored)
        self.src_full.append(full_sizes(w, h, *self.src))

    def stored_reduced(self):
        """per image, per source tile: stored below its full size"""
        return [(inp[1] < fw) | (inp[2] < fh) for inp, (fw, fh) in zip(self.inputs, self.src_full)]

    def n_dst_tiles(self):
        return sum(-(-w // self.dst[0]) * -(-h // self.dst[1]) for (w, h) in self.sizes)

    def dst_full(self):
        fs = [full_sizes(w, h, *self.dst) for (w, h) in self.sizes]
        return np.concatenate([f[0] for f in fs]), np.concatenate([f[1] for f in fs])


def joined(archives):
    """several archives of one (src, dst, c) as one batch"""
    out = Archive(archives[0].src, archives[0].dst, archives[0].c)
    for a in archives:
        for k in range(len(a.images)):
            out.add(a.files[k], a.inputs[k], a.images[k])
    return out


# ---- directional ----------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def dir_images(dst, frame_factor, c):
    """the breakpoint tiles of `frame_factor`, every class, laid out on the grid of `dst` in images of three shapes"""
    imgs = [np.ascontiguousarray(with_form(i, "rgb" if c == 3 else "rgba", *dst)) for i in lay_out(the_oracle(), *dst, frame_factor, list(SHAPES))]
    assert len({i.shape for i in imgs}) == 3
    return imgs


@functools.lru_cache(maxsize=None)
def dir_archive(src, dst, frame_factor, c):
    """dir_images cut into stored tiles at `src`, every one of them at its full size"""
    oracle, out = the_oracle(), Archive(src, dst, c)
    for img in dir_images(dst, frame_factor, c):
        raw, stored, _ = write_and_read(oracle, img, src, DIRECTIONAL, KEEP_FULL)
        out.add(raw, stored, img)  # (check_dir_archive asserts that the oracle's expansion IS the image)
    return out


@functools.lru_cache(maxsize=None)
def dir_ladder_archive(src, dst, c):
    """the frames of 16, -3 and 2 as one batch"""
    return joined([dir_archive(src, dst, f, c) for f in FRAME_FACTORS])


@functools.lru_cache(maxsize=None)
def dir_expected(dst, frame_factor, c, filt, factor):
    """the oracle on the images themselves -> (values, w, h, slots) over the whole batch, in the varied layout"""
    oracle = the_oracle()
    return cat_expected([oracle.shrink_image(i, *dst, DIRECTIONAL, filt, factor, nthreads=8) for i in dir_images(dst, frame_factor, c)])


@functools.lru_cache(maxsize=None)
def dir_ladder_expected(dst, c, filt, factor):
    return cat_expected([dir_expected(dst, f, c, filt, factor) for f in FRAME_FACTORS])


def tiles_on_flips(oracle, images, dst, frame_factor):
    """-> {(class, axis): tiles of the batch whose oracle sum on that axis is S - 1, S or S + 1 for a flip S of that class};
    asserts that every flip of every class and axis is there at all three"""
    bw, bh = dst
    sizes = [(bw, bh), (EDGE_W, bh), (bw, EDGE_H), (EDGE_W, EDGE_H)]
    seen = {(cl, axis): {} for cl in range(4) for axis in (0, 1)}
    for img in images:
        h, w = img.shape[:2]
        for y0 in range(0, h, bh):
            for x0 in range(0, w, bw):
                t = img[y0:y0 + bh, x0:x0 + bw]
                cl = sizes.index((t.shape[1], t.shape[0]))
                sums = oracle.lod_directional(t)[2:]
                for axis in (0, 1):
                    seen[(cl, axis)][sums[axis]] = seen[(cl, axis)].get(sums[axis], 0) + 1
    counts = {}
    for (cl, axis), have in seen.items():
        fl = flips(oracle, *sizes[cl], frame_factor, axis)
        assert len(fl) >= 3, (dst, frame_factor, cl, axis, fl)
        for s in fl:
            for d in (-1, 0, 1):
                assert have.get(s + d, 0) >= 1, f"block {dst} factor {frame_factor} class {cl} axis {axis}: no tile with sum {s}{d:+d}"
        counts[(cl, axis)] = sum(have.get(s + d, 0) for s in fl for d in (-1, 0, 1))
    return counts


def check_dir_archive(oracle, arch, frame_factor):
    """the conditions of a directional archive -> the number of destination tiles on S - 1, S, S + 1 of a flip"""
    what = f"{archive_id((arch.src, arch.dst, arch.c))} factor {frame_factor}"
    for img, (w, h), (vals, tw, th, slots), (fw, fh) in zip(arch.images, arch.sizes, arch.inputs, arch.src_full):
        assert (tw == fw).all() and (th == fh).all(), f"{what}: a source tile is stored below its full size"
        back = oracle.expand_image(w, h, *arch.src, arch.c, LANCZOS3, tw, th, slots)
        assert (back == img).all(), f"{what}: the oracle's expansion is not the image"
    counts = tiles_on_flips(oracle, arch.images, arch.dst, frame_factor)
    return sum(counts.values())


# ---- Oklab ----------------------------------------------------------------------------------------------------------------

class OklabArchive(Archive):
    """.factors: {(k, d, negative): factor}, .on_expanded: the keys whose factor was found on a destination tile over nothing but
    source tiles stored reduced, .skipped: the patterns nearest_attainable passed over"""


@functools.lru_cache(maxsize=None)
def oklab_archive(src, dst, c):
    """the noise frame of the source block and two smaller cuts of it (a ragged one, and one of a single row of tiles), written
    by the oracle at shrink_by 1.0 and read back; the factors that put a full destination tile of the decoded images on every
    target"""
    oracle, out = the_oracle(), OklabArchive(src, dst, c)
    b = src[0]
    assert src[0] == src[1]
    frame = oklab_frame(b, c)
    for img in (frame, np.ascontiguousarray(frame[:2 * b + 5, :3 * b]), np.ascontiguousarray(frame[:b, :2 * b + 3])):
        out.add(*write_and_read(oracle, img, src, SHRINK_BY, OKLAB_WRITTEN_AT))
    # the pool: every full destination tile of the decoded images, those whose every source tile was stored reduced first
    expanded, others = [], []
    for img, (w, h), red in zip(out.images, out.sizes, out.stored_reduced()):
        cols = -(-w // src[0])
        for (cs, rs, (x0, y0, x1, y1)) in covering(w, h, src, dst):
            if (x1 - x0, y1 - y0) == dst:
                under = [bool(red[r * cols + q]) for r in rs for q in cs]
                (expanded if all(under) else others).append(img[y0:y1, x0:x1])
    out.pool_sizes = (len(expanded), len(others))
    out.factors, out.hit, out.on_expanded, out.skipped = {}, {}, set(), []
    for negative in (False, True):
        for k in (levels_of(max(dst)) if not negative else (0, 1)):
            for d in (-1, 0, 1):
                target, skipped = nearest_attainable(threshold_bits(oracle, k), d, negative)
                out.skipped += [(b_, negative) for b_ in skipped]
                for pool in (expanded, others):
                    f, t = next(((f, t) for (f, t) in ((factor_onto(oracle, t, target, negative), t) for t in pool) if f is not None), (None, None))
                    if f is not None:
                        out.factors[(k, d, negative)] = f
                        out.hit[(k, d, negative)] = (target, t)
                        if pool is expanded:
                            out.on_expanded.add((k, d, negative))
                        break
    return out


def oklab_targets(dst):
    return [(k, d, negative) for negative in (False, True) for k in (levels_of(max(dst)) if not negative else (0, 1)) for d in (-1, 0, 1)]


def oklab_ladder_factors(arch):
    """the positive-factor targets and one negative as a single ladder, with their keys"""
    keys = [key for key in arch.factors if not key[2]] + [(0, 0, True)]
    return keys, [arch.factors[key] for key in keys]


@functools.lru_cache(maxsize=None)
def oklab_expected(src, dst, c, filt, factor):
    """the oracle composition: decode -> expand at the source block -> shrink_image at the destination block"""
    oracle = the_oracle()
    return cat_expected([oracle.shrink_image(i, *dst, SHRINK_BY, filt, factor) for i in oklab_archive(src, dst, c).images])


def check_oklab_archive(oracle, arch):
    """the conditions of an Oklab archive -> the number of targets hit on expanded tiles"""
    what = archive_id((arch.src, arch.dst, arch.c))
    for key in oklab_targets(arch.dst):
        assert key in arch.factors, f"{what}: no full destination tile reaches T_{key[0]}{key[1]:+d} (negative {key[2]})"
    for (pattern, negative) in arch.skipped:
        assert oracle_never_reaches(oracle, pattern, negative), (what, hex(pattern), negative)
    for k in levels_of(max(arch.dst)):
        assert any((k, d, False) in arch.on_expanded for d in (-1, 0, 1)), f"{what}: no target of level {k} is hit on an expanded tile"
    red = np.concatenate(arch.stored_reduced())
    assert red.any() and (~red).any(), f"{what}: {int(red.sum())} of {red.size} source tiles stored reduced"
    # and each factor does what it was searched for: the parsed value of its tile has the target's bit pattern, and between the
    # targets d = -1 and d = 0 the oracle's level changes
    side, level = 1 << 30, {}
    for key, (target, tile) in arch.hit.items():
        v = parsed(oracle.lod_oklab(tile, arch.factors[key]))
        assert bits(v) == target, (what, key)
        level[key] = oracle.reduce_dims(v, v, side, side)[0]
    for (k, d, negative) in arch.hit:
        if d == 0:
            assert level[(k, 0, negative)] == level[(k, 1, negative)] == side >> k and level[(k, -1, negative)] == side >> (k + 1), (what, k, negative)
    return len(arch.on_expanded)


# ---- the tests ------------------------------------------------------------------------------------------------------------

def test_helpers_give_the_known_values(oracle):
    """what this module rests on, on numbers worked out against the oracle: the flips of the tile classes used here, the
    thresholds' bit patterns, and the tile builder"""
    assert flips(oracle, 32, 32, 16.0, 0) == [10183, 20365, 40730, 81459, 162918]
    assert flips(oracle, 32, 32, -3.0, 0) == [359908, 794354, 1011577, 1120189, 1174495]
    assert flips(oracle, 13, 32, 16.0, 0) == [7468, 14935, 29869, 59737]
    assert flips(oracle, 32, 32, 16.0, 1) == flips(oracle, 32, 32, 16.0, 0)  # (a square tile: the same divisor on both axes)
    assert [len(flips(oracle, *g, a)) for g in ((24, 24, 16.0), (24, 24, -3.0), (24, 24, 2.0)) for a in (0, 1)] == [5, 5, 5, 5, 5, 5]
    # T_k: the first float whose log2f rounds to -k: one to three patterns past 2^(-k - 1/2), as log2f rounds
    assert [threshold_bits(oracle, k) for k in range(5)] == [0x3F3504F4, 0x3EB504F4, 0x3E3504F5, 0x3DB504F5, 0x3D3504F6]
    for k in range(5):
        t = threshold_bits(oracle, k)
        assert 1 <= t - bits(np.float32(2.0 ** (-k - 0.5))) <= 3
        for negative in ((False, True) if k < 2 else (False,)):  # (every threshold that is a target can itself be a value)
            assert nearest_attainable(t, 0, negative) == (t, [])
    for s in (0, 10182, 10183, 10184):
        assert oracle.lod_directional(build_tile(oracle, 32, 32, s))[2] == s
    assert FRAME_FACTOR[1e-3] == FRAME_FACTOR[-1e-3] == 16.0 and all(FRAME_FACTOR[f] == f for f in FRAME_FACTORS)


@pytest.mark.parametrize("frame_factor", FRAME_FACTORS)
@pytest.mark.parametrize("case", DIR_RESHRINK + DIR_RETILE, ids=archive_id)
def test_directional_archives_meet_their_conditions(oracle, case, frame_factor):
    """every source tile stored full, the expansion equal to the image, every flip of every class and axis at S - 1, S, S + 1"""
    src, dst, c = case
    arch = dir_archive(src, dst, frame_factor, c)
    n = check_dir_archive(oracle, arch, frame_factor)
    assert (len(arch.images), arch.n_dst_tiles(), n) == (23, 192, 176)  # (of 192 destination tiles, 176 sit on S - 1, S or S + 1 of a flip)
    print(f"{archive_id(case)} factor {frame_factor}: {len(arch.images)} images, {arch.n_dst_tiles()} destination tiles, {n} on S-1/S/S+1")
    # the sentinels: nothing but 1x1 tiles, nothing but whole ones
    if frame_factor == 16.0:
        fw, fh = arch.dst_full()
        for filt in (NEAREST, LANCZOS3):
            _, ow, oh, _ = dir_expected(dst, 16.0, c, filt, 1e-3)
            assert (ow == 1).all() and (oh == 1).all()
            _, ow, oh, _ = dir_expected(dst, 16.0, c, filt, -1e-3)
            assert (ow == fw).all() and (oh == fh).all()


@pytest.mark.parametrize("block,c", DIR_VARIED, ids=[archive_id(v) for v in DIR_VARIED])
def test_directional_images_of_the_varied_ladder(oracle, block, c):
    """the varied ladder takes the images themselves: the same flips, counted on the images"""
    n = sum(sum(tiles_on_flips(oracle, dir_images(block, f, c), block, f).values()) for f in FRAME_FACTORS)
    assert n == 3 * 176
    print(f"varied ladder {archive_id((block, c))}: {n} tiles on S-1/S/S+1")


@pytest.mark.parametrize("case", OKLAB_RESHRINK + OKLAB_RETILE, ids=archive_id)
def test_oklab_archives_meet_their_conditions(oracle, case):
    """every target has its factor, every level has one found on an expanded tile, the archive mixes full and reduced tiles"""
    src, dst, c = case
    arch = oklab_archive(src, dst, c)
    n = check_oklab_archive(oracle, arch)
    assert n == len(arch.factors) == 21  # (every target was found on a tile that had been stored reduced and expanded again)
    keys, factors = oklab_ladder_factors(arch)
    assert len(arch.factors) == 3 * len(levels_of(max(dst))) + 6 and len(factors) == 3 * len(levels_of(max(dst))) + 1 <= 32
    assert len(set(factors)) == len(factors)
    print(f"{archive_id(case)}: {len(arch.factors)} targets, {n} on expanded tiles; pool {arch.pool_sizes}; "
          f"{int(np.concatenate(arch.stored_reduced()).sum())} of {sum(len(i[1]) for i in arch.inputs)} source tiles stored reduced")
