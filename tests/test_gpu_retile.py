"""Re-tile of stored tiles on the device (pxz_retile_varied_frames_device, and pxz_transcode_varied_files with another block
size): value bits, sizes and the valid bytes of every slot equal the oracle composition

    oracle.decode_container -> oracle.expand_image(source block, expand_filter) -> oracle.shrink_image(destination block, ...)

and the composition of the calls that existed before (pxz_expand_varied_frames_device at the source block +
pxz_shrink_varied_frames_device at the destination block), with every output poisoned before each call.  The batches and what
they must exercise are those of tests/test_retile_host.py, which holds them against their conditions without a GPU."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_reshrink import SIZE_POISON, VAL_POISON, assert_still_poisoned, cat_expected, to_host, upload_tiles
from test_gpu_varied_decode import POISON, assert_tiles_equal, poisoned
from test_reshrink_host import DIRECTIONAL, LANCZOS3, LDS_PER_CU, SHRINK_BY
from test_retile_host import CASES, RetileCase, cached_retile_case, case_id, covering, filter_pairs

pytestmark = pytest.mark.gpu

INVALID_ARG, TILE_TOO_SMALL, UNSUPPORTED = -1, -4, -5


@pytest.fixture(scope="module")
def gpu(product):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    h = product.Handle(0)
    yield h
    h.close()


# ---- helpers --------------------------------------------------------------------------------------------------------------

def n_dst_tiles(case):
    (dw, dh) = case.dst
    return sum(-(-w // dw) * -(-h // dh) for (w, h) in case.sizes)


def retile(gpu, case, dev_tiles, want_pixels=True):
    """-> ((values, w, h, slots) on the host, per-image flags, pxz_decode_status)"""
    import torch
    tw, th, slots = dev_tiles
    (sw, sh), (dw, dh) = case.pair
    out, flags = poisoned(n_dst_tiles(case), dw * dh * case.c, len(case.sizes))
    if not want_pixels:
        out = (out[0], out[1], out[2], None)
    gpu.retile_varied_frames_device(case.sizes, case.c, sw, sh, dw, dh, case.mode, case.filt, case.factor, case.expand_filter, tw, th, slots,
                                    out=out, image_flags=flags)
    status = gpu.decode_status()
    torch.cuda.synchronize()
    return to_host(out), flags.cpu().numpy(), status


def chained(gpu, case, dev_tiles):
    """the calls that were there before: expand-varied at the source block into a tightly packed image batch, shrink-varied at
    the destination block on it"""
    import torch
    tw, th, slots = dev_tiles
    (sw, sh), (dw, dh) = case.pair
    descs, at = [], 0
    for (w, h) in case.sizes:
        descs.append((w, h, w * case.c, at))
        at += w * h * case.c
    images = torch.full((at,), POISON, dtype=torch.uint8, device="cuda")
    gpu.expand_varied_frames_device(descs, case.c, sw, sh, case.expand_filter, tw, th, slots, images)
    out, _ = poisoned(n_dst_tiles(case), dw * dh * case.c, len(case.sizes))
    gpu.shrink_varied_frames_device(images, dw, dh, case.mode, case.filt, case.factor, descs=descs, channels=case.c, out=out)
    torch.cuda.synchronize()
    return to_host(out)


def check_case(gpu, case, what, with_chain=True):
    dev = upload_tiles(case.inputs)
    got, flags, status = retile(gpu, case, dev)
    assert status == 0 and (flags == 0).all(), f"{what}: status {status}, flags {flags}"
    assert_tiles_equal(got, cat_expected(case.expected), case.c, f"{what} against the oracle")
    # nothing beyond a tile's valid bytes is written
    valid = got[1].astype(np.int64) * got[2] * case.c
    beyond = np.arange(got[3].shape[1])[None, :] >= valid[:, None]
    assert (got[3][beyond] == POISON).all(), f"{what}: bytes beyond the stored tiles were written"
    if with_chain:
        assert_tiles_equal(got, chained(gpu, case, dev), case.c, f"{what} against expand-varied + shrink-varied")
    return dev, got


# ---- results --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_parity_with_the_oracle_and_the_chained_calls(gpu, case):
    """every pair of blocks, channel count, mode and family; on the 32x32 <-> 16x16 and 32x32 <-> 48x20 pairs the five filters on
    both sides and Nearest in / Lanczos3 out, Lanczos3 elsewhere"""
    fam, mode, pair, c = case
    for (xf, sf) in filter_pairs(pair):
        check_case(gpu, cached_retile_case(fam, mode, pair, c, xf, sf), f"{case_id(case)} filters {xf}/{sf}")


@pytest.mark.parametrize("mode", [SHRINK_BY, DIRECTIONAL])
@pytest.mark.parametrize("c", [3, 4])
@pytest.mark.parametrize("fam", "AB")
def test_same_block_equals_the_reshrink(gpu, fam, mode, c):
    case = cached_retile_case(fam, mode, ((32, 32), (32, 32)), c, LANCZOS3, LANCZOS3)
    import torch
    dev = upload_tiles(case.inputs)
    got, flags, status = retile(gpu, case, dev)
    assert status == 0 and (flags == 0).all()
    out, rflags = poisoned(dev[0].numel(), 32 * 32 * c, len(case.sizes))
    gpu.reshrink_varied_frames_device(case.sizes, c, 32, 32, mode, case.filt, case.factor, case.expand_filter, *dev, out=out, image_flags=rflags)
    torch.cuda.synchronize()
    assert_tiles_equal(got, to_host(out), c, "re-tile at the same block against the re-shrink")


@pytest.mark.parametrize("mode", [SHRINK_BY, DIRECTIONAL])
def test_values_and_sizes_only(gpu, mode):
    case = cached_retile_case("A", mode, ((32, 32), (48, 20)), 4, LANCZOS3, LANCZOS3)
    got, flags, status = retile(gpu, case, upload_tiles(case.inputs), want_pixels=False)
    exp = cat_expected(case.expected)
    assert status == 0 and (flags == 0).all()
    assert got[3] is None
    assert (got[0].view(np.uint32) == exp[0].view(np.uint32)).all() and (got[1] == exp[1]).all() and (got[2] == exp[2]).all()


# ---- shape extremes -------------------------------------------------------------------------------------------------------

def test_one_image_of_2500_source_tiles(gpu, oracle):
    """800x800 at 16x16 -> 32x32: 2500 source tiles under 625 destination tiles"""
    case = RetileCase(oracle, "A", SHRINK_BY, ((16, 16), (32, 32)), 4, LANCZOS3, LANCZOS3, sizes=[(800, 800)])
    assert sum(x[1].size for x in case.inputs) == 2500
    k = case.counts()
    assert k["src_small"] * 10 >= k["n_src"] and k["src_full"] * 10 >= k["n_src"] and k["mixed"] * 20 >= k["n_dst"], k
    check_case(gpu, case, "800x800 at 16x16 -> 32x32")


def test_more_destination_tiles_than_blocks(gpu, oracle):
    """800x800 at 32x32 -> 16x16: 2500 destination tiles, more than the largest grid (8 blocks on each of 256 CUs), so blocks walk
    the grid-stride loop"""
    case = RetileCase(oracle, "A", SHRINK_BY, ((32, 32), (16, 16)), 3, LANCZOS3, LANCZOS3, sizes=[(800, 800)])
    assert n_dst_tiles(case) == 2500 > 8 * 256
    k = case.counts()
    assert k["src_small"] * 10 >= k["n_src"] and k["src_full"] * 10 >= k["n_src"], k
    check_case(gpu, case, "800x800 at 32x32 -> 16x16")


def test_forty_one_tile_images(gpu, oracle):
    """the owner search: every tile, in both layouts, belongs to another image"""
    sizes = [(1 + (7 * i) % 16, 1 + (5 * i) % 16) for i in range(40)]
    case = RetileCase(oracle, "B", SHRINK_BY, ((16, 16), (32, 32)), 3, LANCZOS3, LANCZOS3, sizes=sizes)
    assert all(x[1].size == 1 for x in case.inputs) and n_dst_tiles(case) == 40
    check_case(gpu, case, "40 one-tile images")


# ---- flagged source tiles -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", [3, 4])
@pytest.mark.parametrize("pair", [((32, 32), (48, 20)), ((32, 32), (16, 16)), ((16, 16), (32, 32))], ids=lambda p: f"{p[0][0]}x{p[0][1]}to{p[1][0]}x{p[1][1]}")
def test_flagged_source_tiles(gpu, product, pair, c):
    """two source tiles of one image carry stored sizes that cannot be: a stored width of zero, and -- an edge tile -- a stored
    width one pixel beyond its place in the source grid (still within the block).  Exactly the destination tiles that cover
    them come back 0 x 0 with value bits 0 and their slots untouched"""
    case = cached_retile_case("B", SHRINK_BY, pair, c, LANCZOS3, LANCZOS3)
    (sw, sh), (dw, dh) = pair
    clean, flags, status = retile(gpu, case, upload_tiles(case.inputs))
    assert status == 0 and (flags == 0).all()
    assert_tiles_equal(clean, cat_expected(case.expected), c, "the clean run")
    geoms = [(w, h, w * c, 0) for (w, h) in case.sizes]
    src_to, dst_to = product.varied_layout(geoms, sw, sh), product.varied_layout(geoms, dw, dh)
    victim = max(range(len(case.sizes)), key=lambda i: int(src_to[i + 1] - src_to[i]))
    a, b = int(src_to[victim]), int(src_to[victim + 1])
    w, h = case.sizes[victim]
    cols, rows = -(-w // sw), -(-h // sh)
    assert b - a == cols * rows >= 3
    edge_w = w - (cols - 1) * sw
    assert edge_w < sw  # (the last tile's place is narrower than the block: edge_w + 1 fits a slot, not the tile)
    tw, th, slots = upload_tiles(case.inputs)
    tw[a] = 0
    tw[b - 1] = edge_w + 1
    hit = [k for k, (cs, rs, _) in enumerate(covering(w, h, pair[0], pair[1]))
           if (0 in cs and 0 in rs) or (cols - 1 in cs and rows - 1 in rs)]
    n_victim = int(dst_to[victim + 1] - dst_to[victim])
    assert 2 <= len(hit) < n_victim
    hit = [int(dst_to[victim]) + k for k in hit]
    got, flags, status = retile(gpu, case, (tw, th, slots))
    assert status == 1
    assert [int(f) for f in flags] == [1 if i == victim else 0 for i in range(len(case.sizes))]
    for t in hit:
        assert got[1][t] == 0 and got[2][t] == 0 and got[0].view(np.uint32)[t] == 0, t
        assert (got[3][t] == POISON).all(), t
    keep = np.ones(got[1].size, bool)
    keep[hit] = False
    assert_tiles_equal(tuple(x[keep] for x in got), tuple(x[keep] for x in clean), c, "tiles that cover no flagged source tile")
    # and the next clean call starts from a clean status
    again, flags, status = retile(gpu, case, upload_tiles(case.inputs))
    assert status == 0 and (flags == 0).all()
    assert_tiles_equal(again, clean, c, "the clean run after a flagged one")


# ---- validation -----------------------------------------------------------------------------------------------------------

def raw_call(gpu, product, sizes, c, sw, sh, bw, bh, mode, filt, factor, xf, tw, th, slots, out, flags, n_images=None, null=None, params=True):
    vals, ow, oh, ns = out
    geoms = [(w, h, w * c, 0) for (w, h) in sizes]
    pd = product.binding.Params(bw, bh, mode, filt, factor, 0)
    ptr = {"descs": C.cast(product.image_descs(geoms), C.c_void_p), "tw": C.c_void_p(tw.data_ptr()), "th": C.c_void_p(th.data_ptr()),
           "slots": C.c_void_p(slots.data_ptr()), "vals": C.c_void_p(vals.data_ptr()), "ow": C.c_void_p(ow.data_ptr()),
           "oh": C.c_void_p(oh.data_ptr())}
    if null:
        ptr[null] = None
    rc = gpu._L.pxz_retile_varied_frames_device(gpu._h, ptr["descs"], len(geoms) if n_images is None else n_images, c, sw, sh,
                                                C.byref(pd) if params else None, xf, ptr["tw"], ptr["th"], ptr["slots"], ptr["vals"],
                                                ptr["ow"], ptr["oh"], C.c_void_p(ns.data_ptr()), C.c_void_p(flags.data_ptr()))
    return rc, (gpu._L.pxz_last_error(gpu._h) or b"").decode()


def test_validation_runs_before_anything_is_written(gpu, product):
    import torch
    sw, sh, bw, bh, c = 32, 32, 16, 16, 4
    sizes = [(40, 40), (33, 64), (64, 64)]  # image 1 has a 1-px edge column in both grids
    S, T = 4 + 4 + 4, 9 + 12 + 16
    tw = torch.ones(S, dtype=torch.int32, device="cuda")
    th = torch.ones(S, dtype=torch.int32, device="cuda")
    slots = torch.zeros((S, 128 * 128 * c), dtype=torch.uint8, device="cuda")  # (room for the largest source block below)
    out, flags = poisoned(T, bw * bh * c, len(sizes))
    base = dict(sizes=sizes, c=c, sw=sw, sh=sh, bw=bw, bh=bh, mode=SHRINK_BY, filt=LANCZOS3, factor=1.0, xf=LANCZOS3, tw=tw, th=th, slots=slots,
                out=out, flags=flags)

    def expect(code, text, **change):
        rc, err = raw_call(gpu, product, **{**base, **change})
        assert rc == code and text in err, (rc, err, change)
        torch.cuda.synchronize()
        assert_still_poisoned(out, flags)

    for name in ("tw", "th", "slots", "vals", "ow", "oh"):
        expect(INVALID_ARG, "null device pointer", null=name)
    expect(INVALID_ARG, "null image descriptors", null="descs")
    expect(INVALID_ARG, "null params", params=False)
    expect(INVALID_ARG, "empty image batch", n_images=0)
    expect(INVALID_ARG, "zero source block", sw=0)
    expect(INVALID_ARG, "zero source block", sh=0)
    expect(INVALID_ARG, "zero block size", bw=0)
    expect(INVALID_ARG, "expand_filter", xf=5)
    expect(INVALID_ARG, "filter must be 0..4", filt=5)
    expect(INVALID_ARG, "channels must be 3 or 4", c=5)
    expect(INVALID_ARG, "factor must be finite", factor=float("nan"))
    expect(INVALID_ARG, "image 1: empty image", sizes=[(40, 40), (0, 7), (64, 64)])
    expect(TILE_TOO_SMALL, "image 1: directional detector needs tiles of at least 2x2 px", mode=DIRECTIONAL)
    # a pair beyond the footprint: a source plane above 64 KB, and two blocks whose parts are as large as a 64 KB source tile
    assert product.retile_lds_bytes(129, 128, bw, bh, SHRINK_BY, LANCZOS3) > LDS_PER_CU
    expect(UNSUPPORTED, "160 KB", sw=129, sh=128)
    assert product.retile_lds_bytes(128, 128, 128, 127, SHRINK_BY, LANCZOS3) > LDS_PER_CU
    expect(UNSUPPORTED, "160 KB", sw=128, sh=128, bw=128, bh=127)
    # the same batch is fine for shrink_by: every source tile is 1 x 1, every destination tile comes out 1 x 1
    rc, err = raw_call(gpu, product, **base)
    assert rc == 0, err
    torch.cuda.synchronize()
    assert (out[1].cpu().numpy() == 1).all() and (out[2].cpu().numpy() == 1).all() and (flags.cpu().numpy() == 0).all()


# ---- host form ------------------------------------------------------------------------------------------------------------

def oracle_files(oracle, case, filter_byte):
    """the oracle composition's files at the destination block"""
    (dw, dh) = case.dst
    return [oracle.encode_container(w, h, dw, dh, case.c, filter_byte, vals, None, ow, oh, ns)
            for (w, h), (vals, ow, oh, ns) in zip(case.sizes, case.expected)]


@pytest.mark.parametrize("mode", [SHRINK_BY, DIRECTIONAL])
@pytest.mark.parametrize("pair", [((64, 64), (32, 32)), ((32, 32), (64, 64))], ids=["64to32", "32to64"])
def test_files_in_files_out_fitting_pairs(gpu, product, oracle, pair, mode):
    """the CLI's -b on a .pix input: files at the CLI's default 64x64 come back at 32x32 (through the re-tile: the new block
    divides the files'), and the reverse (a pair that fits, but merges tiles: the host form keeps its four calls for it)"""
    assert product.retile_lds_bytes(*pair[0], *pair[1], mode, LANCZOS3) <= LDS_PER_CU
    for c in (3, 4):
        case = cached_retile_case("A", mode, pair, c, LANCZOS3, LANCZOS3)
        got = gpu.transcode_varied_files(case.files, *pair[1], mode, case.filt, case.factor, case.expand_filter, filter_byte=2)
        assert got == oracle_files(oracle, case, 2)


def test_files_in_files_out_fallback(gpu, product, oracle):
    """a pair the footprint refuses still comes back as the oracle's files, through the image batch in handle scratch"""
    refused = [(pair, mode) for pair in [((128, 128), (16, 16)), ((128, 128), (64, 64)), ((128, 128), (128, 127))] for mode in (SHRINK_BY, DIRECTIONAL)
               if product.retile_lds_bytes(*pair[0], *pair[1], mode, LANCZOS3) > LDS_PER_CU]
    pair, mode = refused[0]
    assert (pair, mode) == (((128, 128), (128, 127)), SHRINK_BY)  # (128x128 -> 16x16 fits: the staging is bounded by the part)
    case = RetileCase(oracle, "A", mode, pair, 4, LANCZOS3, LANCZOS3, sizes=[(130, 129), (200, 140), (97, 260)])
    k = case.counts()
    assert k["src_small"] >= 2 and k["src_full"] >= 2 and k["reduced"] * 10 >= k["n_dst"] and k["full"] * 10 >= k["n_dst"], k
    got = gpu.transcode_varied_files(case.files, *pair[1], mode, case.filt, case.factor, case.expand_filter, filter_byte=3)
    assert got == oracle_files(oracle, case, 3)


# ---- handle hygiene -------------------------------------------------------------------------------------------------------

def test_single_geometry_state_is_left_alone(gpu):
    """a single-geometry 32x32 shrink before and after re-tiles on the same handle: the same results, the same handle state"""
    import torch
    frames = gpu.synth_frames_device(3, 96, 160, 4)

    def single():
        out = gpu.shrink_frames_device(frames, 32, 32, SHRINK_BY, LANCZOS3, 1.0)
        torch.cuda.synchronize()
        return [x.cpu().numpy().copy() for x in out], gpu.state()

    single()  # (the first launch on a handle has no statistics of a launch before it)
    before, state_before = single()
    for pair in [((32, 32), (16, 16)), ((16, 16), (32, 32))]:
        case = cached_retile_case("A", SHRINK_BY, pair, 4, LANCZOS3, LANCZOS3)
        got, flags, status = retile(gpu, case, upload_tiles(case.inputs))
        assert status == 0
    after, state_after = single()
    assert state_after == state_before
    assert (before[1] == after[1]).all() and (before[2] == after[2]).all()
    assert (before[0].view(np.uint32) == after[0].view(np.uint32)).all()
    valid = before[1].astype(np.int64) * before[2] * 4
    idx = np.arange(before[3].shape[-1])[None, None, :] < valid[..., None]
    assert (before[3][idx] == after[3][idx]).all()
