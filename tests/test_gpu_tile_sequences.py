"""The tile loops' carried state, driven by frames whose tile kinds come in a known order (tests/tile_sequences.py; what the frames
make the oracle do is asserted in tests/test_tile_sequences_host.py).  Everything is compared bit for bit with the oracle: value
bits, sizes, every valid slot byte, every expanded pixel.

In this process no knob is set: the launches are those of the whole chip, and on it every wave of a small frame gets one tile.
The loops' steady state is reached by the SAME tests in child processes with a small launch (knobs are read once per process):

  PXZ_WPB=1 PXZ_CHUNK_LG=6             one wave of shrink32_kernel walks 64 adjacent tiles in flat order; one wave per block elsewhere
  PXZ_CUS=1                            every grid is that of a one-CU chip: a handful of blocks, each walks tiles b, b + G, b + 2G, ...
  PXZ_CUS=1 PXZ_WPB=1 PXZ_CHUNK_LG=0   two blocks of one wave: stride 2, one wave's list batches fill
  PXZ_CUS=1 PXZ_NO_CLONE_AHEAD=1       shrink_by without the detector's copies (frames b, d and e)
  PXZ_CUS=1 PXZ_OKLAB_V1=1             frames e on oklab_kernel<16 | 32 | 64>: 15 tiles per batch, 64x64 tiles parked in HBM

and the directed suites that were there before run once more under PXZ_CUS=1.  The children run one at a time, each under a time
limit of four times its measured wall time; after a child that ended abnormally, or whose output reports a GPU fault, no
further child is started."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import tile_sequences as ts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCKS = (16, 32, 64)
GEOMS = [(b, c) for b in BLOCKS for c in (4, 3)]
GEOM_IDS = [f"{b}x{b}-c{c}" for b, c in GEOMS]


@pytest.fixture(scope="module")
def gpu(product):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    h = product.Handle(0)
    yield h
    h.close()


# ---- frames and references: made once, shared, never written to ----------------------------------------------------------------

_frames, _expected = {}, {}


def frame(oracle, what, *key):
    if (what,) + key not in _frames:
        make = {"pairs": ts.pair_frame, "triples": ts.triple_frame}[what]
        _frames[(what,) + key] = make(oracle, *key)[0]
    return _frames[(what,) + key]


def expected(oracle, key, img, bw, bh, mode, filt, factor):
    key = key + (bw, bh, mode, filt, factor)
    if key not in _expected:
        out = oracle.shrink_image(img, bw, bh, mode, filt, factor, nthreads=8)
        for a in out:
            a.setflags(write=False)
        _expected[key] = out
    return _expected[key]


def assert_same_tiles(got, exp, channels, what):
    gv, gw, gh, gs = got
    ev, ew, eh, es = exp
    gw, gh = np.asarray(gw).astype(np.uint32), np.asarray(gh).astype(np.uint32)
    assert (gw == ew).all() and (gh == eh).all(), f"{what}: sizes differ on tiles {np.nonzero((gw != ew) | (gh != eh))[0][:8].tolist()}"
    gb, eb = np.asarray(gv).view(np.uint32), ev.view(np.uint32)
    assert (gb == eb).all(), f"{what}: value bits differ on tiles {np.nonzero(gb != eb)[0][:8].tolist()}"
    valid = np.arange(es.shape[1])[None, :] < (ew.astype(np.int64) * eh * channels)[:, None]
    diff = (gs != es) & valid
    assert not diff.any(), f"{what}: {int(diff.sum())} stored bytes differ in tiles {np.nonzero(diff.any(axis=1))[0][:8].tolist()}"


def upload(imgs):
    """[N, H, W, C] on the device, every row on a 4-byte boundary (the view [:, :, :W] of a tensor whose width is the next multiple
    of four pixels): what the native RGB instances of the fast kernels ask for; RGBA rows that are no 16-byte multiples are
    re-pitched by the library"""
    import torch
    H, W, C = imgs[0].shape
    wide = torch.zeros((len(imgs), H, (W + 3) & ~3, C), dtype=torch.uint8).cuda()
    frames = wide[:, :, :W]
    frames.copy_(torch.from_numpy(np.stack([np.array(i) for i in imgs])))
    return frames


def fetch(out, n=0):
    vals, ow, oh, slots = out
    return vals[n].cpu().numpy(), ow[n].cpu().numpy(), oh[n].cpu().numpy(), slots[n].cpu().numpy()


# ---- a. pairs: the directional fast paths ------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("filt", [ts.LANCZOS3, ts.NEAREST], ids=["lanczos3", "nearest"])
@pytest.mark.parametrize("block,channels", GEOMS, ids=GEOM_IDS)
def test_pairs_on_the_fast_paths(gpu, oracle, block, channels, filt):
    """shrink16 / shrink32 / shrink64_kernel (the parked output of the previous tile and its flush, the prefetched registers, the
    list batches) and the worklist kernel behind them: the host form, then two frames in one device batch -- the second one upside
    down in tile rows, so that a wave's next tile comes from another frame with other kinds."""
    import torch
    img = frame(oracle, "pairs", block, channels)
    exp = expected(oracle, ("pairs", channels), img, block, block, ts.DIRECTIONAL, filt, ts.FACTOR)
    got = gpu.shrink_image(img, block, block, ts.DIRECTIONAL, filt, ts.FACTOR)
    assert_same_tiles(got, exp, channels, f"pairs {block} c{channels} filter {filt}, host form")
    rows = img.reshape(ts.PAIR_ROWS, block, img.shape[1], channels)
    flipped = np.ascontiguousarray(rows[::-1]).reshape(img.shape)
    exp2 = expected(oracle, ("pairs flipped", channels), flipped, block, block, ts.DIRECTIONAL, filt, ts.FACTOR)
    out = gpu.shrink_frames_device(upload([img, flipped]), block, block, ts.DIRECTIONAL, filt, ts.FACTOR)
    torch.cuda.synchronize()
    assert_same_tiles(fetch(out, 0), exp, channels, f"pairs {block} c{channels} filter {filt}, device form, frame 0")
    assert_same_tiles(fetch(out, 1), exp2, channels, f"pairs {block} c{channels} filter {filt}, device form, frame 1")


@pytest.mark.gpu
@pytest.mark.parametrize("mode,factor", [(ts.DIRECTIONAL, ts.FACTOR), (ts.SHRINK_BY, ts.BY_FACTOR)], ids=["directional", "by"])
@pytest.mark.parametrize("bw,bh,channels", [(24, 24, 4), (40, 24, 3), (32, 32, 4)], ids=["24x24-c4", "40x24-c3", "32x32-c4-shifted"])
def test_pairs_on_the_generic_kernel(gpu, oracle, bw, bh, channels, mode, factor):
    """the 32x32 pair frame cut into tiles of another size (the generic kernel's ticket loop; 24x24 shrink_by: the run-time
    geometry detector in front of it); 32x32 "shifted": the frame without its first pixel column and row, so that every tile
    straddles four of the drawn ones"""
    img = frame(oracle, "pairs", 32, channels)
    key = ("pairs", channels)
    if (bw, bh) == (32, 32):
        img, key = np.ascontiguousarray(img[1:, 1:]), ("pairs shifted", channels)
    exp = expected(oracle, key, img, bw, bh, mode, ts.LANCZOS3, factor)
    got = gpu.shrink_image(img, bw, bh, mode, ts.LANCZOS3, factor)
    assert_same_tiles(got, exp, channels, f"pair frame at {bw}x{bh} c{channels} mode {mode}")


@pytest.mark.gpu
@pytest.mark.parametrize("block,channels", GEOMS, ids=GEOM_IDS)
def test_pairs_and_triples_on_the_ladder(gpu, oracle, block, channels):
    """pxz_shrink_image_ladder: the pair frame at three directional factors, the triple frame at three shrink_by factors"""
    for what, mode, factors in (("pairs", ts.DIRECTIONAL, (ts.FACTOR, 4.0, 64.0)), ("triples", ts.SHRINK_BY, (ts.BY_FACTOR, 0.5, 4.0))):
        img = frame(oracle, what, block, channels)
        vals, ow, oh, slots = gpu.shrink_image_ladder(img, block, block, mode, ts.LANCZOS3, factors)
        for r, k in enumerate(factors):
            exp = expected(oracle, (what, channels), img, block, block, mode, ts.LANCZOS3, k)
            assert_same_tiles((vals[r], ow[r], oh[r], slots[r]), exp, channels, f"{what} {block} c{channels} ladder rung {r} (k={k})")


@pytest.mark.gpu
@pytest.mark.parametrize("block,channels", GEOMS, ids=GEOM_IDS)
def test_pairs_and_triples_in_a_varied_batch(gpu, oracle, block, channels):
    """pxz_shrink_varied_frames_device (grid-stride loop, resample windows kept in LDS between tiles): the frame, a crop of it that
    ends in other ragged tiles, and the frame again"""
    import torch
    for what, mode, factor in (("pairs", ts.DIRECTIONAL, ts.FACTOR), ("triples", ts.SHRINK_BY, ts.BY_FACTOR)):
        img = frame(oracle, what, block, channels)
        crop = np.ascontiguousarray(img[: 5 * block + 3, : 4 * block + 9])
        imgs = [img, crop, img]
        keys = [(what, channels), (what + " crop", channels), (what, channels)]
        offs, vals, ow, oh, slots = gpu.shrink_varied_frames_device([torch.from_numpy(np.array(i)).cuda() for i in imgs], block, block, mode,
                                                                    ts.LANCZOS3, factor)
        torch.cuda.synchronize()
        vals, ow, oh, slots = vals.cpu().numpy(), ow.cpu().numpy(), oh.cpu().numpy(), slots.cpu().numpy()
        for i, (im, key) in enumerate(zip(imgs, keys)):
            exp = expected(oracle, key, im, block, block, mode, ts.LANCZOS3, factor)
            lo, hi = int(offs[i]), int(offs[i + 1])
            assert_same_tiles((vals[lo:hi], ow[lo:hi], oh[lo:hi], slots[lo:hi]), exp, channels, f"{what} {block} c{channels} varied image {i}")


@pytest.mark.gpu
@pytest.mark.parametrize("filt", [ts.LANCZOS3, ts.NEAREST], ids=["lanczos3", "nearest"])
@pytest.mark.parametrize("block,channels", GEOMS, ids=GEOM_IDS)
def test_expand_of_the_pair_frames_tiles(gpu, oracle, block, channels, filt):
    """expand16 / expand64 / expand_kernel (ticket loops; the first stored pixel prefetched a tile ahead; the list behind the
    group kernels): the oracle's shrunk tiles of the pair frame, in the same order, and of the triple frame (many clones)"""
    import torch
    for what, mode, factor in (("pairs", ts.DIRECTIONAL, ts.FACTOR), ("triples", ts.SHRINK_BY, ts.BY_FACTOR)):
        img = frame(oracle, what, block, channels)
        H, W = img.shape[:2]
        _, ew, eh, es = expected(oracle, (what, channels), img, block, block, mode, ts.LANCZOS3, factor)
        key = ("expanded", what, block, channels, filt)
        if key not in _expected:
            _expected[key] = oracle.expand_image(W, H, block, block, channels, filt, ew, eh, es)
        got = gpu.expand_image(W, H, channels, block, block, filt, ew, eh, es)
        assert gpu.decode_status() == 0
        bad = (got != _expected[key]).any(axis=2)
        cols = -(-W // block)
        assert not bad.any(), f"{what} {block} c{channels} filter {filt}: tiles {sorted({int(y // block) * cols + int(x // block) for y, x in zip(*np.nonzero(bad))})[:8]}"
        # the device form: the same tiles twice in one batch
        dev = [torch.from_numpy(np.stack([a, a])).cuda() for a in (ew.astype(np.int32), eh.astype(np.int32), es)]
        out = torch.full((2, H, W, channels), 0xA5, dtype=torch.uint8, device="cuda")
        gpu.expand_frames_device(tuple(out.shape), block, block, filt, *dev, out=out)
        torch.cuda.synchronize()
        assert gpu.decode_status() == 0
        both = out.cpu().numpy()
        assert (both[0] == _expected[key]).all() and (both[1] == _expected[key]).all(), f"{what} {block} c{channels} filter {filt}, device form"


# ---- b. shrink_by triples: the values that travel two tiles ahead ----------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("block,channels", GEOMS, ids=GEOM_IDS)
def test_triples_in_shrink_by(gpu, oracle, block, channels):
    """vb_cur / vb_next / fl_next / pre_skipped of shrink32_kernel and shrink64_kernel, the clone list of 64x64, the groups of
    shrink16_kernel: whole and reduced tiles in all eight orders of three.  The host form, then two frames in one device batch
    (the second with its tile rows in reverse order)."""
    import torch
    img = frame(oracle, "triples", block, channels)
    exp = expected(oracle, ("triples", channels), img, block, block, ts.SHRINK_BY, ts.LANCZOS3, ts.BY_FACTOR)
    got = gpu.shrink_image(img, block, block, ts.SHRINK_BY, ts.LANCZOS3, ts.BY_FACTOR)
    assert_same_tiles(got, exp, channels, f"triples {block} c{channels}, host form")
    rows = img.reshape(ts.TRIPLE_ROWS, block, img.shape[1], channels)
    flipped = np.ascontiguousarray(rows[::-1]).reshape(img.shape)
    exp2 = expected(oracle, ("triples flipped", channels), flipped, block, block, ts.SHRINK_BY, ts.LANCZOS3, ts.BY_FACTOR)
    for filt, e0, e1 in ((ts.LANCZOS3, exp, exp2),):
        out = gpu.shrink_frames_device(upload([img, flipped]), block, block, ts.SHRINK_BY, filt, ts.BY_FACTOR)
        torch.cuda.synchronize()
        assert_same_tiles(fetch(out, 0), e0, channels, f"triples {block} c{channels}, device form, frame 0")
        assert_same_tiles(fetch(out, 1), e1, channels, f"triples {block} c{channels}, device form, frame 1")


# ---- c. list batches ------------------------------------------------------------------------------------------------------------------

LIST_CASES = ([(32, n, 0, False) for n in ts.LIST_COUNTS] + [(32, 0, n, False) for n in ts.LIST_COUNTS] + [(32, 17, 17, False)] +
              [(64, n, 0, False) for n in ts.LIST_COUNTS] + [(64, n, 0, True) for n in ts.LIST_COUNTS])


@pytest.mark.gpu
@pytest.mark.parametrize("block,n_alpha,n_sliver,tall", LIST_CASES, ids=[f"{b}{'-tall' if t else ''}-alpha{a}-sliver{s}" for b, a, s, t in LIST_CASES])
def test_list_batches(product, oracle, block, n_alpha, n_sliver, tall):
    """Full tiles of which exactly n_alpha have one pixel of alpha 254 (list A) and n_sliver are of the 16 x (2|1) class
    shrink32_kernel hands on (list B): Handle.state() counts exactly them, and every tile equals the oracle's -- a batch of
    kListBatch = 16 that drops or repeats an entry when it fills, or is not flushed after the loop, changes the count and leaves
    a tile unwritten.  Twice on one handle (the second launch sizes the worklist kernel's grid by what the first one listed),
    then with the transparency hint: shrink32a_kernel / shrink64_kernel<ALPHA> walk list A.
    32x32, 8 x 8 tiles: shrink32_kernel's batches are per wave; in the one-wave children one wave lists all n.
    64x64: shrink64_kernel's batches are per BLOCK and PXZ_WPB does not reach it.  The 8 x 8 frames spread their n tiles over
    the four blocks of a one-CU launch, so no block's batch fills there (at most 11 entries); the "tall" frames (18 x 8 tiles)
    put all n on the tiles 0, 4, 8, ... that block 0 of that launch walks, and with PXZ_CUS=1 its batch fills once (16, 17,
    31), twice (32, 33) and is flushed partly full after the loop.  No full tile is handed on by shrink64_kernel, so there is
    no list-B frame for it."""
    import torch
    img, alpha, sliver = ts.tall_list_frame(oracle, n_alpha) if tall else ts.list_frame(oracle, block, n_alpha, n_sliver)
    exp = expected(oracle, ("list", n_alpha, n_sliver, tall), img, block, block, ts.DIRECTIONAL, ts.LANCZOS3, ts.FACTOR)
    h = product.Handle(0)  # (a handle of its own: what state() reports is this test's launches alone)
    try:
        for run in range(2):
            got = h.shrink_image(img, block, block, ts.DIRECTIONAL, ts.LANCZOS3, ts.FACTOR)
            st = h.state()
            assert_same_tiles(got, exp, 4, f"list frame {block}, {n_alpha} alpha, {n_sliver} sliver, run {run}")
            assert st["transparent_tiles_seen_by_last_finished_launch"] == n_alpha, st
            assert st["tiles_listed_by_last_finished_launch"] == n_alpha + n_sliver, st
        out = h.shrink_frames_device(upload([img]), block, block, ts.DIRECTIONAL, ts.LANCZOS3, ts.FACTOR, transparency_hint=True)
        torch.cuda.synchronize()
        st = h.state()
        assert_same_tiles(fetch(out), exp, 4, f"list frame {block}, {n_alpha} alpha, {n_sliver} sliver, hinted")
        # (list B now also holds what the four-plane kernel hands on: only list A's count is pinned)
        assert st["alpha_kernel"] and st["transparent_tiles_seen_by_last_finished_launch"] == n_alpha, st
    finally:
        h.close()


# ---- d. detector batch seams ------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("channels", [4, 3])
@pytest.mark.parametrize("geom", ts.SEAM_GEOMS, ids=lambda g: f"{g[0]}x{g[1]}")
def test_detector_batch_seams(gpu, oracle, geom, channels):
    """oklab2_kernel<16 | 32 | 64>, oklab_kernel (24x24: run-time geometry): one row of n tiles for every n around one, two and
    three batches of 15 / 14 / 3 -- a block's pipeline drains through a partial last batch; a single tile; fewer tiles than waves."""
    bw, bh = geom
    for n in ts.SEAM_COUNTS:
        img, _ = ts.seam_frame(oracle, bw, bh, channels, n)
        exp = expected(oracle, ("seam", n, channels), img, bw, bh, ts.SHRINK_BY, ts.LANCZOS3, ts.BY_FACTOR)
        got = gpu.shrink_image(img, bw, bh, ts.SHRINK_BY, ts.LANCZOS3, ts.BY_FACTOR)
        assert_same_tiles(got, exp, channels, f"{n} tiles of {bw}x{bh} c{channels}")


# ---- e. detector alpha sequences ----------------------------------------------------------------------------------------------------
# ("seams" in the names: the PXZ_NO_CLONE_AHEAD child selects them with frames d)

def alpha_frame(oracle, bw, bh, edge_w=0, edge_h=0):
    key = ("alpha", bw, bh, edge_w, edge_h)
    if key not in _frames:
        _frames[key] = ts.alpha_sequence_frame(oracle, bw, bh, edge_w, edge_h)[0]
    return _frames[key]


@pytest.mark.gpu
@pytest.mark.parametrize("block", BLOCKS)
def test_detector_alpha_seams_square(gpu, oracle, block):
    """oklab2_kernel<16 | 32 | 64> (PXZ_OKLAB_V1: oklab_kernel<16 | 32 | 64>, the last one parked in HBM): cur_opaque / old_opaque /
    band_opaque, al_cur[] / al_old[] and their hand-over, alpha_px[] and the parked alpha word.  Tiles that are opaque, transparent
    everywhere, in their first, their last or one inner row only, or in one pixel of alpha 254, in every order of two (and of
    three over opaque / not opaque) at the strides 3, 14 and 15 at which a one-block launch hands a producer wave its tiles.  The
    host form, then two frames in one device batch, the second with its tile rows in reverse order; 32 and 64: once more with a
    row of tiles transparent everywhere and a last row 8 px high behind it, twice in one batch (a short tile after a full one, a
    full tile of the next frame after a short one)."""
    import torch
    img = alpha_frame(oracle, block, block)
    exp = expected(oracle, ("alpha",), img, block, block, ts.SHRINK_BY, ts.LANCZOS3, ts.BY_FACTOR)
    got = gpu.shrink_image(img, block, block, ts.SHRINK_BY, ts.LANCZOS3, ts.BY_FACTOR)
    assert_same_tiles(got, exp, 4, f"alpha sequence {block}, host form")
    rows = img.reshape(ts.ALPHA_ROWS, block, img.shape[1], 4)
    flipped = np.ascontiguousarray(rows[::-1]).reshape(img.shape)
    exp2 = expected(oracle, ("alpha flipped",), flipped, block, block, ts.SHRINK_BY, ts.LANCZOS3, ts.BY_FACTOR)
    out = gpu.shrink_frames_device(upload([img, flipped]), block, block, ts.SHRINK_BY, ts.LANCZOS3, ts.BY_FACTOR)
    torch.cuda.synchronize()
    assert_same_tiles(fetch(out, 0), exp, 4, f"alpha sequence {block}, device form, frame 0")
    assert_same_tiles(fetch(out, 1), exp2, 4, f"alpha sequence {block}, device form, frame 1")
    if block in (32, 64):
        short = alpha_frame(oracle, block, block, 0, ts.ALPHA_SHORT_ROW)
        exp = expected(oracle, ("alpha short row",), short, block, block, ts.SHRINK_BY, ts.LANCZOS3, ts.BY_FACTOR)
        got = gpu.shrink_image(short, block, block, ts.SHRINK_BY, ts.LANCZOS3, ts.BY_FACTOR)
        assert_same_tiles(got, exp, 4, f"alpha sequence {block} with a short last row, host form")
        out = gpu.shrink_frames_device(upload([short, short]), block, block, ts.SHRINK_BY, ts.LANCZOS3, ts.BY_FACTOR)
        torch.cuda.synchronize()
        for n in range(2):
            assert_same_tiles(fetch(out, n), exp, 4, f"alpha sequence {block} with a short last row, device form, frame {n}")


@pytest.mark.gpu
@pytest.mark.parametrize("geom", sorted(ts.ALPHA_RAGGED), ids=lambda g: f"{g[0]}x{g[1]}")
def test_detector_alpha_seams_run_time_geometry(gpu, oracle, geom):
    """oklab_kernel<0, 3> (24x24: three bands, alpha_px[] in registers) and oklab_kernel<0, 0> (40x32: five bands, the alpha word
    parked in HBM and read back through tile_prev a period later), 15 tiles per batch; the 6 px right column (rows padded to whole
    quads, masked by `have`), the ragged bottom row and the corner go through the three edge-region launches, transparent pixels
    in all of them."""
    bw, bh = geom
    img = alpha_frame(oracle, bw, bh, *ts.ALPHA_RAGGED[geom])
    exp = expected(oracle, ("alpha ragged",), img, bw, bh, ts.SHRINK_BY, ts.LANCZOS3, ts.BY_FACTOR)
    got = gpu.shrink_image(img, bw, bh, ts.SHRINK_BY, ts.LANCZOS3, ts.BY_FACTOR)
    assert_same_tiles(got, exp, 4, f"alpha sequence {bw}x{bh} with ragged edges")


@pytest.mark.gpu
@pytest.mark.parametrize("block", BLOCKS)
def test_detector_alpha_seams_on_the_ladder(gpu, oracle, block):
    """pxz_shrink_image_ladder: one detector pass over the alpha sequence, three shrink_by factors decided from its values"""
    img = alpha_frame(oracle, block, block)
    factors = (ts.BY_FACTOR, 0.5, 4.0)
    vals, ow, oh, slots = gpu.shrink_image_ladder(img, block, block, ts.SHRINK_BY, ts.LANCZOS3, factors)
    for r, k in enumerate(factors):
        exp = expected(oracle, ("alpha",), img, block, block, ts.SHRINK_BY, ts.LANCZOS3, k)
        assert_same_tiles((vals[r], ow[r], oh[r], slots[r]), exp, 4, f"alpha sequence {block}, ladder rung {r} (k={k})")


# ---- the same under small launches: child processes -----------------------------------------------------------------------------

ABNORMAL = (124, 134, 137, 139)
# a GPU fault that a child's test met and reported as an ordinary failure (return code 1): nothing more is started on that card either
GPU_FAULTS = ("illegal memory access", "hipErrorIllegalAddress", "Memory access fault", "HSA_STATUS_ERROR", "hipErrorLaunchFailure",
              "unspecified launch failure")
_abnormal = []   # the first child that ended abnormally: no child is started after it

# (id, environment, -k expression over this file, measured wall time of the child on an MI355X in seconds: DESIGN §8r)
OWN = [
    ("wpb1-chunk6", {"PXZ_WPB": "1", "PXZ_CHUNK_LG": "6"}, "not child", 6.1),
    ("cus1", {"PXZ_CUS": "1"}, "not child", 5.9),
    ("cus1-wpb1-chunk0", {"PXZ_CUS": "1", "PXZ_WPB": "1", "PXZ_CHUNK_LG": "0"}, "not child", 6.0),
    ("cus1-no-clone-ahead", {"PXZ_CUS": "1", "PXZ_NO_CLONE_AHEAD": "1"}, "(triples or seams) and not child", 5.3),
    ("cus1-oklab-v1", {"PXZ_CUS": "1", "PXZ_OKLAB_V1": "1"}, "alpha_seams and not child", 4.3),
]
# (file, -k expression: the directed cases without the full-size, 8K and 2049-image ones, measured seconds under PXZ_CUS=1)
OTHERS = [
    ("test_gpu_value_domain.py", "", 8.8),
    ("test_gpu_expand_domain.py", "", 9.7),
    ("test_gpu_level_breakpoints.py", "", 8.4),
    ("test_gpu_archive_breakpoints.py", "", 7.9),
    ("test_gpu_stream_seams.py", "", 23.4),
    ("test_gpu_distortion.py", "test_windows_kept_across_sets_that_repeat_a_stored_size", 5.1),
    ("test_gpu_varied.py", "test_random_batches_equal_single_calls_and_oracle", 4.8),
    ("test_gpu_varied_decode.py", "test_batches_equal_single_calls_and_oracle", 4.9),
    ("test_gpu_reshrink.py", "test_parity_with_the_oracle_and_the_chained_calls", 6.1),
    ("test_gpu_retile.py", "test_parity_with_the_oracle_and_the_chained_calls", 5.7),
    ("test_gpu_retile_distortion.py", "test_hand_made_sizes_equal_the_oracle", 4.4),
]


def child_command(path, k):
    cmd = [sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", path), "-x", "-q", "-m", "gpu", "-p", "no:cacheprovider"]
    return cmd + (["-k", k] if k else [])


def run_child(what, path, k, env_add, measured):
    if _abnormal:
        pytest.fail(f"not started: an earlier child ended abnormally ({_abnormal[0]})")
    assert measured > 0.0, "no measured wall time for this child"
    env = dict(os.environ)
    env.update(env_add)
    t0 = time.monotonic()
    try:
        r = subprocess.run(child_command(path, k), env=env, cwd=ROOT, capture_output=True, text=True, timeout=4.0 * measured)
    except subprocess.TimeoutExpired:
        _abnormal.append(f"{what}: no end after {4.0 * measured:.0f} s")
        pytest.fail(_abnormal[0])
    tail = "\n".join(r.stdout.splitlines()[-15:])
    if r.returncode < 0 or r.returncode in ABNORMAL:
        _abnormal.append(f"{what}: return code {r.returncode}")
        pytest.fail(f"{_abnormal[0]}\n{tail}\n{r.stderr[-2000:]}")
    fault = next((f for f in GPU_FAULTS if f in r.stdout or f in r.stderr), None)
    if fault is not None:
        _abnormal.append(f"{what}: the child reported a GPU fault ({fault})")
        pytest.fail(f"{_abnormal[0]}\n{tail}\n{r.stderr[-2000:]}")
    print(f"{what}: {time.monotonic() - t0:.1f} s")
    assert r.returncode == 0, f"{what}:\n{tail}\n{r.stderr[-2000:]}"
    assert " passed" in tail and " failed" not in tail and " skipped" not in tail, tail


@pytest.mark.gpu
@pytest.mark.parametrize("name,env,k,measured", OWN, ids=[c[0] for c in OWN])
def test_child_this_file_under_a_small_launch(name, env, k, measured):
    run_child(name, "test_gpu_tile_sequences.py", k, env, measured)


@pytest.mark.gpu
@pytest.mark.parametrize("path,k,measured", OTHERS, ids=[c[0][9:-3] for c in OTHERS])
def test_child_directed_suites_on_one_cu(path, k, measured):
    run_child(f"PXZ_CUS=1 {path}", path, k, {"PXZ_CUS": "1"}, measured)
