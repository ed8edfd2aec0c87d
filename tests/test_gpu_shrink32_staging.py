"""shrink32_kernel's staging, tile addresses and opacity test, against the oracle -- value bits, sizes and every stored pixel.

The kernel stages a tile's pixels into three planes of zero-extended u16 (byte permutes, or any cheaper form tried in their
place); the next tile's loads take a wave-uniform 64-bit pointer (the tile's first byte, stepped by eight rows on the scalar unit)
plus ONE 32-bit lane offset, lane/8 rows + the lane's pixel quad; the detector's two sums are joined across the wave by DPP row
broadcasts.  What can go wrong there: a swapped byte lane, a half that is not zero-extended, a lane offset that forgets the pitch,
a frame or tile base that does not reach the scalar pointer, a row of lanes left out of a sum, an opacity test that misses a
pixel.  The frames here are small, with R, G and B drawn independently, so that any of these changes a detector sum or a stored
byte."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LANCZOS3, NEAREST = 4, 0
DIRECTIONAL, FACTOR = 1, 16.0  # the benchmark's caller and factor


@pytest.fixture(scope="module")
def gpu(product):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    h = product.Handle(0)
    yield h
    h.close()


# ---- inputs ---------------------------------------------------------------------------------------------------------------

KINDS = ("constant", "vertical-edge", "horizontal-edge", "noise", "soft", "columns")


def tile_of_kind(kind, rng):
    """one opaque 32x32 RGBA tile; the three colour channels never share a value stream"""
    t = np.empty((32, 32, 4), np.uint8)
    t[..., 3] = 255
    if kind == "constant":
        t[..., :3] = rng.integers(0, 256, 3, dtype=np.uint8)
    elif kind == "vertical-edge":  # left | right: all variation along x
        t[:, :13, :3] = rng.integers(0, 256, 3, dtype=np.uint8)
        t[:, 13:, :3] = rng.integers(0, 256, 3, dtype=np.uint8)
    elif kind == "horizontal-edge":
        t[:21, :, :3] = rng.integers(0, 256, 3, dtype=np.uint8)
        t[21:, :, :3] = rng.integers(0, 256, 3, dtype=np.uint8)
    elif kind == "noise":
        t[..., :3] = rng.integers(0, 256, (32, 32, 3), dtype=np.uint8)
    elif kind == "soft":  # weak noise on three different bases: 8x8 or 16x16 at factor 16, the matrix-core resample
        t[..., :3] = rng.integers(30, 190, 3)[None, None, :] + rng.integers(0, int(rng.choice([28, 56])), (32, 32, 3))
    else:  # "columns": strong along x, weak along y -- a one-pass class or a narrow output
        t[..., :3] = np.clip(rng.integers(0, 256, (1, 32, 3)) + rng.integers(0, 4, (32, 1, 3)), 0, 255)
    return t


def frame_of_kinds(cols, rows, seed, first_kind=0):
    rng = np.random.default_rng(seed)
    img = np.empty((rows * 32, cols * 32, 4), np.uint8)
    for ty in range(rows):
        for tx in range(cols):
            kind = KINDS[(first_kind + ty * cols + tx) % len(KINDS)]
            img[ty * 32:ty * 32 + 32, tx * 32:tx * 32 + 32] = tile_of_kind(kind, rng)
    return img


def sizes_of(exp):
    return {(int(w), int(h)) for w, h in zip(exp[1].tolist(), exp[2].tolist())}


def assert_same_tiles(got, exp, what):
    gv, gw, gh, gs = got
    ev, ew, eh, es = exp
    assert (gw == ew).all() and (gh == eh).all(), f"{what}: sizes differ on tiles {np.nonzero((gw != ew) | (gh != eh))[0][:8].tolist()}"
    gb, eb = gv.view(np.uint32), ev.view(np.uint32)
    assert (gb == eb).all(), f"{what}: value bits differ on tiles {np.nonzero(gb != eb)[0][:8].tolist()}"
    valid = np.arange(es.shape[1])[None, :] < (ew.astype(np.int64) * eh * 4)[:, None]
    diff = (gs != es) & valid
    assert not diff.any(), f"{what}: {int(diff.sum())} stored bytes differ in tiles {np.nonzero(diff.any(axis=1))[0][:8].tolist()}"


@pytest.fixture(scope="module")
def mixed(oracle):
    """96x64: one tile of each kind, and what the oracle makes of it with both filters (computed once)"""
    img = frame_of_kinds(3, 2, seed=20240607)
    return img, {f: oracle.shrink_image(img, 32, 32, DIRECTIONAL, f, FACTOR) for f in (LANCZOS3, NEAREST)}


# ---- 1. mixed tile paths ----------------------------------------------------------------------------------------------------

def test_the_mixed_frame_spans_the_paths(mixed):
    """A check of this file's own input (the oracle alone, no GPU): clone, a 1x1, a one-pass class and two-pass sizes all occur."""
    img, exp = mixed
    assert img.shape == (64, 96, 4) and (img[..., 3] == 255).all()
    for f in (LANCZOS3, NEAREST):
        s = sizes_of(exp[f])
        assert len(s) >= 4, s
        assert (32, 32) in s and (1, 1) in s, s                  # clone (the noise tile), the constant tile
        assert any((w == 32) != (h == 32) for w, h in s), s      # a one-pass class: a hard edge along one axis only
        assert any(4 <= w < 32 and 4 <= h < 32 for w, h in s), s  # a two-pass resample on the matrix cores
        assert any(w <= 4 and 1 < h <= 16 for w, h in s), s       # a narrow output


@pytest.mark.gpu
@pytest.mark.parametrize("filt", [LANCZOS3, NEAREST], ids=["lanczos3", "nearest"])
def test_mixed_tile_paths(gpu, mixed, filt):
    img, exp = mixed
    got = gpu.shrink_image(img, 32, 32, DIRECTIONAL, filt, FACTOR)
    assert_same_tiles(got, exp[filt], f"96x64 mixed, filter {filt}")


# ---- 2. second frame, small and large pitch ---------------------------------------------------------------------------------

@pytest.mark.gpu
def test_second_frame_is_reached_through_the_tile_base(gpu, oracle):
    """two frames of 64x32 in one device batch: frame 1's tiles lie a frame stride behind frame 0's"""
    import torch
    frames = np.stack([frame_of_kinds(2, 1, seed=5, first_kind=3), frame_of_kinds(2, 1, seed=6, first_kind=4)])
    assert frames.shape == (2, 32, 64, 4) and (frames[0] != frames[1]).any()
    vals, ow, oh, slots = gpu.shrink_frames_device(torch.from_numpy(frames).cuda(), 32, 32, DIRECTIONAL, LANCZOS3, FACTOR)
    torch.cuda.synchronize()
    for n in range(2):
        exp = oracle.shrink_image(frames[n], 32, 32, DIRECTIONAL, LANCZOS3, FACTOR)
        got = (vals[n].cpu().numpy(), ow[n].cpu().numpy().astype(np.uint32), oh[n].cpu().numpy().astype(np.uint32), slots[n].cpu().numpy())
        assert_same_tiles(got, exp, f"frame {n} of two")


@pytest.mark.gpu
def test_a_row_of_256_tiles_at_pitch_32768(gpu, oracle):
    """8192x32 (1 MB): the lane offset's row term is the pitch, 32768 bytes here against 256 and 384 above"""
    img = frame_of_kinds(256, 1, seed=77)
    assert img.shape == (32, 8192, 4) and img.strides[0] == 32768
    exp = oracle.shrink_image(img, 32, 32, DIRECTIONAL, LANCZOS3, FACTOR, nthreads=8)
    assert len(sizes_of(exp)) >= 4
    got = gpu.shrink_image(img, 32, 32, DIRECTIONAL, LANCZOS3, FACTOR)
    assert_same_tiles(got, exp, "8192x32")


def test_host_decision_about_32_bit_lane_offsets():
    """No GPU: pxz_offset_check.bin holds fast32_lane_offset_fits (what the host asks before it lets a batch onto the 32x32 fast
    kernels) against 64-bit arithmetic at the boundary -- 7 rows + 7 pixel quads must fit 32 bits: the last pitch that does is
    (2^32 - 1 - 112) / 7 = 613566740 -- and checks that below it the kernel's 32-bit product does not wrap."""
    tool = os.path.join(ROOT, "pixlzr-rust_amd", "csrc", "pxz_offset_check.bin")
    assert os.path.exists(tool), "run __graft_entry__.build()"
    r = subprocess.run([tool], capture_output=True, text=True)
    words = r.stdout.split()
    assert r.returncode == 0 and words[:2] == ["ok", str((2 ** 32 - 1 - 112) // 7)] and int(words[2]) > 4000, r.stdout + r.stderr


# ---- 3. one transparent pixel -----------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_one_transparent_pixel_sends_exactly_its_tile_to_the_list(product, oracle):
    """64x64, four full tiles (constant, noise, noise, soft: none of them a class the fast kernel hands on), alpha 254 in ONE pixel
    of the last tile -- the 16th dword of lane 63's share, the last operand of the opacity test.  That tile, and no other, is
    listed (Handle.state(): list A counts the full tiles with transparency, the second count lists A and B together); the
    outputs equal the oracle's.  The same frame without the pixel lists nothing."""
    h = product.Handle(0)
    try:
        rng = np.random.default_rng(31)
        img = np.empty((64, 64, 4), np.uint8)
        for t, kind in enumerate(("constant", "noise", "noise", "soft")):
            img[(t // 2) * 32:(t // 2) * 32 + 32, (t % 2) * 32:(t % 2) * 32 + 32] = tile_of_kind(kind, rng)
        opaque = img.copy()
        img[63, 63, 3] = 254
        for frame, listed in ((img, 1), (opaque, 0), (img, 1)):
            got = h.shrink_image(frame, 32, 32, DIRECTIONAL, LANCZOS3, FACTOR)
            st = h.state()
            exp = oracle.shrink_image(frame, 32, 32, DIRECTIONAL, LANCZOS3, FACTOR)
            assert_same_tiles(got, exp, f"64x64 with {listed} transparent pixel(s)")
            assert st["transparent_tiles_seen_by_last_finished_launch"] == listed, st
            assert st["tiles_listed_by_last_finished_launch"] == listed, st
    finally:
        h.close()
