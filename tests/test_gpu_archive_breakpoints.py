"""The level decision at its exact breakpoints on the ladder and archive kernels.  tests/test_gpu_level_breakpoints.py pins the
single-geometry kernels, varied_kernel, the factor ladder and the tree; the compare has since been written out four more
times ("copied, not called"), each text deriving v0 / v1 itself, and the ladders fold the result into the key that decides
whether a rung is cloned or resampled:

  varied_ladder_tail (pxz_varied_tile.h)   varied_ladder_kernel, retile_ladder_kernel
  its copy in pxz_reshrink_ladder.hip      reshrink_ladder_kernel
  pxz_reshrink.hip                         reshrink_kernel (out of place and in place)
  pxz_retile.hip                           retile_kernel

Here every one of them meets tiles ON the breakpoints: the directional images of that module (gradient sums S - 1, S, S + 1
for every flip S) as archives whose every tile is stored full, and Oklab archives with factors at which a tile that was
stored reduced and expanded again has a parsed value of exactly a threshold's bit pattern, its predecessor or its successor.
Every comparison covers value bits, both sizes and the valid bytes of every slot, against the oracle composition
(decode -> expand at the source block -> shrink_image at the destination block), with no tolerance; every output is poisoned
before each call.  The batches are those of tests/test_archive_breakpoints_host.py, which holds them against their conditions
without a GPU."""
import numpy as np
import pytest

from test_archive_breakpoints_host import (CALL_FACTORS, DIR_RESHRINK, DIR_RETILE, DIR_VARIED, FRAME_FACTORS, OKLAB_RESHRINK, OKLAB_RETILE,
                                           archive_id, dir_archive, dir_expected, dir_images, dir_ladder_archive, dir_ladder_expected,
                                           oklab_archive, oklab_expected, oklab_ladder_factors)
from test_gpu_level_breakpoints import FRAME_FACTOR, LANCZOS3, NEAREST
from test_gpu_parity import assert_same_tiles
from test_gpu_reshrink import SIZE_POISON, VAL_POISON, to_host, upload_tiles
from test_gpu_varied_decode import POISON, assert_tiles_equal, poisoned
from test_reshrink_host import DIRECTIONAL, SHRINK_BY

pytestmark = pytest.mark.gpu

FILTERS = (NEAREST, LANCZOS3)  # the shrink's filter; the expand filter is Lanczos3 throughout
SENTINEL = 0x5A                # the slots of the second run at the k = 0 targets


@pytest.fixture(scope="module")
def gpu(product):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    h = product.Handle(0)
    yield h
    h.close()


# ---- the calls ------------------------------------------------------------------------------------------------------------

def fresh(arch, rungs=1, sentinel=None):
    """poisoned outputs of `rungs` rungs at the destination block (a ladder asks for one more: the guard), and the image flags"""
    out, flags = poisoned(rungs * arch.n_dst_tiles(), arch.dst[0] * arch.dst[1] * arch.c, len(arch.sizes))
    if sentinel is not None:
        out[3].fill_(sentinel)
    return out, flags


def finish(gpu, out, flags, what):
    import torch
    status = gpu.decode_status()
    torch.cuda.synchronize()
    assert status == 0 and (flags.cpu().numpy() == 0).all(), f"{what}: status {status}, flags {flags.cpu().numpy()}"
    return to_host(out)


def reshrink(gpu, arch, dev, mode, filt, factor, what, sentinel=None, in_place=False):
    out, flags = fresh(arch, sentinel=sentinel)
    if in_place:
        out = (out[0],) + tuple(x.clone() for x in dev)
        dev = out[1:]
    gpu.reshrink_varied_frames_device(arch.sizes, arch.c, *arch.dst, mode, filt, factor, LANCZOS3, *dev, out=out, image_flags=flags)
    return finish(gpu, out, flags, what)


def retile(gpu, arch, dev, mode, filt, factor, what, sentinel=None):
    out, flags = fresh(arch, sentinel=sentinel)
    gpu.retile_varied_frames_device(arch.sizes, arch.c, *arch.src, *arch.dst, mode, filt, factor, LANCZOS3, *dev, out=out, image_flags=flags)
    return finish(gpu, out, flags, what)


def varied(gpu, arch, dev_images, mode, filt, factor, what, sentinel=None):
    import torch
    out, _ = fresh(arch, sentinel=sentinel)
    gpu.shrink_varied_frames_device(dev_images, *arch.dst, mode, filt, factor, out=out)
    torch.cuda.synchronize()
    return to_host(out)


def one_factor(gpu, arch, dev, mode, filt, factor, what, sentinel=None):
    """the one-factor call of an archive: the re-shrink where the blocks agree, the re-tile where they differ"""
    call = reshrink if arch.src == arch.dst else retile
    return call(gpu, arch, dev, mode, filt, factor, what, sentinel=sentinel)


def split(host, K, T, what):
    """the rungs of a ladder's outputs; the guard rung behind the last must be untouched"""
    vals, ow, oh, px = host
    assert (vals[K * T:].view(np.uint32) == VAL_POISON).all() and (ow[K * T:] == SIZE_POISON).all() and (oh[K * T:] == SIZE_POISON).all(), \
        f"{what}: the guard rung's values or sizes were written"
    assert (px[K * T:] == POISON).all(), f"{what}: the guard rung's slots were written"
    return [tuple(x[r * T:(r + 1) * T] for x in host) for r in range(K)]


def archive_ladder(gpu, arch, dev, mode, filt, factors, what):
    """the ladder of an archive: the re-shrink ladder where the blocks agree, the re-tile ladder where they differ"""
    K = len(factors)
    out, flags = fresh(arch, rungs=K + 1)
    if arch.src == arch.dst:
        gpu.reshrink_varied_ladder_frames_device(arch.sizes, arch.c, *arch.dst, mode, filt, factors, LANCZOS3, *dev, out=out, image_flags=flags)
    else:
        gpu.retile_varied_ladder_frames_device(arch.sizes, arch.c, *arch.src, *arch.dst, mode, filt, factors, LANCZOS3, *dev, out=out,
                                               image_flags=flags)
    return split(finish(gpu, out, flags, what), K, arch.n_dst_tiles(), what)


def varied_ladder(gpu, arch, dev_images, mode, filt, factors, what):
    import torch
    K = len(factors)
    out, _ = fresh(arch, rungs=K + 1)
    gpu.shrink_varied_ladder_frames_device(dev_images, *arch.dst, mode, filt, factors, out=out)
    torch.cuda.synchronize()
    return split(to_host(out), K, arch.n_dst_tiles(), what)


def check(got, exp, c, what, slot_fill=POISON):
    """value bits, both sizes, the valid bytes of every slot; and nothing beyond a tile's valid bytes is written"""
    assert_tiles_equal(got, exp, c, what)
    assert_same_tiles(got, tuple(exp[:3]) + (exp[3][:, : got[3].shape[1]],), c, what)
    valid = got[1].astype(np.int64) * got[2] * c
    beyond = np.arange(got[3].shape[1])[None, :] >= valid[:, None]
    assert (got[3][beyond] == slot_fill).all(), f"{what}: bytes beyond the stored tiles were written"


def check_sentinels(arch, got, factor, what):
    """at +-1e-3 every break is a sentinel: nothing but 1x1 tiles, or nothing but whole ones"""
    if factor == 1e-3:
        assert (got[1] == 1).all() and (got[2] == 1).all(), f"{what}: a tile larger than 1x1"
    if factor == -1e-3:
        fw, fh = arch.dst_full()
        assert (got[1] == fw).all() and (got[2] == fh).all(), f"{what}: a tile below its full size"


def upload_images(arch):
    import torch
    return [torch.from_numpy(i).cuda() for i in arch.images]


# ---- 1, 3. directional, one factor per call -------------------------------------------------------------------------------

@pytest.mark.parametrize("factor", CALL_FACTORS)
@pytest.mark.parametrize("case", DIR_RESHRINK + DIR_RETILE, ids=archive_id)
def test_directional_breakpoints_one_factor(gpu, case, factor):
    """reshrink_kernel (the blocks agree) and retile_kernel (64x64 -> 32x32: the new block divides the old; 16x16 -> 32x32: tiles
    merge; 48x20 -> 32x32: tiles straddle; 32x32 -> 24x24).  The images of the factor's frames in three shapes as one batch, every
    source tile stored full, every flip of every class and axis at S - 1, S, S + 1"""
    src, dst, c = case
    arch = dir_archive(src, dst, FRAME_FACTOR[factor], c)
    dev = upload_tiles(arch.inputs)
    for filt in FILTERS:
        what = f"directional {archive_id(case)} k={factor} filter {filt}"
        got = one_factor(gpu, arch, dev, DIRECTIONAL, filt, factor, what)
        check(got, dir_expected(dst, FRAME_FACTOR[factor], c, filt, factor), c, what)
        check_sentinels(arch, got, factor, what)


# ---- 2, 3. directional, the five factors as one ladder --------------------------------------------------------------------

@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("case", DIR_RESHRINK + DIR_RETILE, ids=archive_id)
def test_directional_breakpoints_on_the_archive_ladders(gpu, case, filt):
    """reshrink_ladder_kernel and retile_ladder_kernel: the frames of 16, -3 and 2 as one batch, the five factors as one ladder;
    every rung against the oracle and against the one-factor call on the same batch"""
    src, dst, c = case
    arch = dir_ladder_archive(src, dst, c)
    dev = upload_tiles(arch.inputs)
    factors = list(CALL_FACTORS)
    what = f"directional ladder {archive_id(case)} filter {filt}"
    rungs = archive_ladder(gpu, arch, dev, DIRECTIONAL, filt, factors, what)
    for r, factor in enumerate(factors):
        check(rungs[r], dir_ladder_expected(dst, c, filt, factor), c, f"{what} rung {r} (k={factor}) against the oracle")
        check_sentinels(arch, rungs[r], factor, what)
        one = one_factor(gpu, arch, dev, DIRECTIONAL, filt, factor, what)
        check(rungs[r], one, c, f"{what} rung {r} (k={factor}) against the one-factor call")


# ---- 4. directional, the varied ladder ------------------------------------------------------------------------------------

@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("block,c", DIR_VARIED, ids=[archive_id(v) for v in DIR_VARIED])
def test_directional_breakpoints_on_the_varied_ladder(gpu, block, c, filt):
    """varied_ladder_kernel, from the images themselves: the same batch, the same five rungs, against the oracle and against
    shrink_varied_frames_device"""
    arch = dir_ladder_archive(block, block, c)
    dev = upload_images(arch)
    factors = list(CALL_FACTORS)
    what = f"directional varied ladder {archive_id((block, c))} filter {filt}"
    rungs = varied_ladder(gpu, arch, dev, DIRECTIONAL, filt, factors, what)
    for r, factor in enumerate(factors):
        check(rungs[r], dir_ladder_expected(block, c, filt, factor), c, f"{what} rung {r} (k={factor}) against the oracle")
        check_sentinels(arch, rungs[r], factor, what)
        check(rungs[r], varied(gpu, arch, dev, DIRECTIONAL, filt, factor, what), c, f"{what} rung {r} (k={factor}) against the one-factor call")


# ---- 5. Oklab: values EQUAL to a threshold, out of the expand path --------------------------------------------------------

def oklab_what(case, key, factor, filt):
    k, d, negative = key
    return f"oklab {archive_id(case)} T_{k}{d:+d} negative={negative} k={factor!r} filter {filt}"


@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("case", OKLAB_RESHRINK + OKLAB_RETILE, ids=archive_id)
def test_oklab_thresholds_one_factor(gpu, case, filt):
    """reshrink_kernel and retile_kernel: one call per found factor.  k = 0 is the "stored at full size" decision, the clone out:
    those calls run again into slots filled with another byte, where a wrongly kept or wrongly cloned tile shows"""
    src, dst, c = case
    arch = oklab_archive(src, dst, c)
    dev = upload_tiles(arch.inputs)
    for key, factor in arch.factors.items():
        what = oklab_what(case, key, factor, filt)
        exp = oklab_expected(src, dst, c, filt, factor)
        check(one_factor(gpu, arch, dev, SHRINK_BY, filt, factor, what), exp, c, what)
        if key[0] == 0:
            check(one_factor(gpu, arch, dev, SHRINK_BY, filt, factor, what, sentinel=SENTINEL), exp, c, what + " into sentinel slots", SENTINEL)


@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("case", OKLAB_RESHRINK + OKLAB_RETILE, ids=archive_id)
def test_oklab_thresholds_on_the_archive_ladders(gpu, case, filt):
    """reshrink_ladder_kernel and retile_ladder_kernel: the positive-factor targets and a negative one as a single ladder (16 rungs);
    every rung against the oracle composition and against its one-factor call"""
    src, dst, c = case
    arch = oklab_archive(src, dst, c)
    dev = upload_tiles(arch.inputs)
    keys, factors = oklab_ladder_factors(arch)
    assert len(factors) == 16
    rungs = archive_ladder(gpu, arch, dev, SHRINK_BY, filt, factors, f"oklab ladder {archive_id(case)} filter {filt}")
    for r, (key, factor) in enumerate(zip(keys, factors)):
        what = f"rung {r} of the ladder, " + oklab_what(case, key, factor, filt)
        check(rungs[r], oklab_expected(src, dst, c, filt, factor), c, what + " against the oracle")
        check(rungs[r], one_factor(gpu, arch, dev, SHRINK_BY, filt, factor, what), c, what + " against the one-factor call")


@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("case", OKLAB_RESHRINK, ids=archive_id)
def test_oklab_thresholds_on_the_varied_ladder(gpu, case, filt):
    """varied_ladder_kernel on the images the oracle decodes from the archives (the tiles that carry the targets are expanded
    ones): one-rung ladders at every found factor, the k = 0 ones again into sentinel slots, and the 16-rung ladder; against
    the oracle and against shrink_varied_frames_device"""
    src, dst, c = case
    arch = oklab_archive(src, dst, c)
    dev = upload_images(arch)
    for key, factor in arch.factors.items():
        what = "varied ladder of one rung, " + oklab_what(case, key, factor, filt)
        exp = oklab_expected(src, dst, c, filt, factor)
        check(varied_ladder(gpu, arch, dev, SHRINK_BY, filt, [factor], what)[0], exp, c, what)
        if key[0] == 0:
            import torch
            out, _ = fresh(arch, sentinel=SENTINEL)
            gpu.shrink_varied_ladder_frames_device(dev, *dst, SHRINK_BY, filt, [factor], out=out)
            torch.cuda.synchronize()
            check(to_host(out), exp, c, what + " into sentinel slots", SENTINEL)
    keys, factors = oklab_ladder_factors(arch)
    assert len(factors) == 16
    rungs = varied_ladder(gpu, arch, dev, SHRINK_BY, filt, factors, f"oklab varied ladder {archive_id(case)} filter {filt}")
    for r, (key, factor) in enumerate(zip(keys, factors)):
        what = f"rung {r} of the varied ladder, " + oklab_what(case, key, factor, filt)
        check(rungs[r], oklab_expected(src, dst, c, filt, factor), c, what + " against the oracle")
        check(rungs[r], varied(gpu, arch, dev, SHRINK_BY, filt, factor, what), c, what + " against the one-factor call")


# ---- 6. the re-shrink in place --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", OKLAB_RESHRINK, ids=archive_id)
def test_oklab_full_size_decision_in_place(gpu, case):
    """the outputs alias the inputs, at the k = 0 targets: whether a tile is cloned out is the k = 0 compare.  (The slots of an
    in-place call hold the inputs: what lies beyond a tile's valid bytes is not looked at.)"""
    src, dst, c = case
    arch = oklab_archive(src, dst, c)
    dev = upload_tiles(arch.inputs)
    hit = 0
    for key, factor in arch.factors.items():
        if key[0] != 0:
            continue
        for filt in FILTERS:
            what = "in place, " + oklab_what(case, key, factor, filt)
            apart = reshrink(gpu, arch, dev, SHRINK_BY, filt, factor, what)
            together = reshrink(gpu, arch, dev, SHRINK_BY, filt, factor, what, in_place=True)
            assert_tiles_equal(together, apart, c, what + " against out of place")
            assert_tiles_equal(together, oklab_expected(src, dst, c, filt, factor), c, what + " against the oracle")
            hit += 1
    assert hit == 6 * len(FILTERS)  # T_0 - 1, T_0, T_0 + 1 with positive and with negative factors


@pytest.mark.parametrize("case", DIR_RESHRINK, ids=archive_id)
def test_directional_flips_in_place(gpu, case):
    """the flips of factor 16 (and the sentinels on its frames) through the in-place re-shrink"""
    src, dst, c = case
    arch = dir_archive(src, dst, 16.0, c)
    dev = upload_tiles(arch.inputs)
    for factor in (16.0, 1e-3, -1e-3):
        for filt in FILTERS:
            what = f"in place, directional {archive_id(case)} k={factor} filter {filt}"
            apart = reshrink(gpu, arch, dev, DIRECTIONAL, filt, factor, what)
            together = reshrink(gpu, arch, dev, DIRECTIONAL, filt, factor, what, in_place=True)
            assert_tiles_equal(together, apart, c, what + " against out of place")
            assert_tiles_equal(together, dir_expected(dst, 16.0, c, filt, factor), c, what + " against the oracle")
            check_sentinels(arch, together, factor, what)
