"""Re-tile ladder on the device (pxz_retile_varied_ladder_frames_device, and pxz_transcode_varied_ladder_files with another block
size): every rung's value bits, sizes and valid slot bytes equal the oracle composition

    oracle.decode_container -> oracle.expand_image(source block, expand_filter) -> oracle.shrink_image(destination block, factors[r])

and, on the device, pxz_retile_varied_frames_device at that rung's factor and rung r of pxz_expand_varied_frames_device at the
source block + pxz_shrink_varied_ladder_frames_device at the destination block.  Every output is poisoned before each call, and
one guard rung behind the last must come back untouched.  The batches and what they must exercise are those of
tests/test_retile_ladder_host.py, which holds them against their conditions without a GPU."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_reshrink import SIZE_POISON, VAL_POISON, assert_still_poisoned, to_host, upload_tiles
from test_gpu_retile import n_dst_tiles
from test_gpu_varied_decode import POISON, assert_tiles_equal, poisoned
from test_reshrink_host import DIRECTIONAL, LANCZOS3, LDS_PER_CU, SHRINK_BY
from test_reshrink_ladder_host import FACTORS
from test_retile_host import CASES, RetileCase, case_id, covering, filter_pairs
from test_retile_ladder_host import cached_retile_ladder, oracle_retile_rungs

pytestmark = pytest.mark.gpu

INVALID_ARG, TILE_TOO_SMALL, UNSUPPORTED, BUFFER_TOO_SMALL = -1, -4, -5, -7
MODES = [SHRINK_BY, DIRECTIONAL]


@pytest.fixture(scope="module")
def gpu(product):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    h = product.Handle(0)
    yield h
    h.close()


# ---- helpers --------------------------------------------------------------------------------------------------------------

def split_rungs(out, K, T):
    vals, ow, oh, px = to_host(out)
    assert (vals[K * T:].view(np.uint32) == VAL_POISON).all() and (ow[K * T:] == SIZE_POISON).all() and (oh[K * T:] == SIZE_POISON).all(), \
        "the guard rung's values or sizes were written"
    assert (px[K * T:] == POISON).all(), "the guard rung's slots were written"
    return [tuple(x[r * T:(r + 1) * T] for x in (vals, ow, oh, px)) for r in range(K)], px


def ladder(gpu, case, dev_tiles, factors, want_pixels=True):
    """one ladder call into poisoned outputs of len(factors) rungs and a guard rung, which is checked here
    -> ([(values, w, h, slots) per rung, on the host], per-image flags, pxz_decode_status)"""
    import torch
    tw, th, slots = dev_tiles
    (sw, sh), (dw, dh) = case.pair
    K, T = len(factors), n_dst_tiles(case)
    out, flags = poisoned((K + 1) * T, dw * dh * case.c, len(case.sizes))
    gpu.retile_varied_ladder_frames_device(case.sizes, case.c, sw, sh, dw, dh, case.mode, case.filt, factors, case.expand_filter, tw, th, slots,
                                           out=out if want_pixels else (out[0], out[1], out[2], None), image_flags=flags)
    status = gpu.decode_status()
    torch.cuda.synchronize()
    rungs, px = split_rungs(out, K, T)
    if not want_pixels:
        assert (px == POISON).all(), "slots were written by a call that was given none"
    return rungs, flags.cpu().numpy(), status


def retile_at(gpu, case, dev_tiles, factor):
    """the one-factor re-tile at `factor` into poisoned outputs"""
    import torch
    tw, th, slots = dev_tiles
    (sw, sh), (dw, dh) = case.pair
    out, flags = poisoned(n_dst_tiles(case), dw * dh * case.c, len(case.sizes))
    gpu.retile_varied_frames_device(case.sizes, case.c, sw, sh, dw, dh, case.mode, case.filt, factor, case.expand_filter, tw, th, slots,
                                    out=out, image_flags=flags)
    torch.cuda.synchronize()
    return to_host(out)


def chained_ladder(gpu, case, dev_tiles, factors):
    """the calls that were there before: expand-varied at the source block into a tightly packed image batch, the varied ladder
    at the destination block on it"""
    import torch
    tw, th, slots = dev_tiles
    (sw, sh), (dw, dh) = case.pair
    descs, at = [], 0
    for (w, h) in case.sizes:
        descs.append((w, h, w * case.c, at))
        at += w * h * case.c
    images = torch.full((at,), POISON, dtype=torch.uint8, device="cuda")
    gpu.expand_varied_frames_device(descs, case.c, sw, sh, case.expand_filter, tw, th, slots, images)
    K, T = len(factors), n_dst_tiles(case)
    out, _ = poisoned((K + 1) * T, dw * dh * case.c, len(case.sizes))
    gpu.shrink_varied_ladder_frames_device(images, dw, dh, case.mode, case.filt, factors, descs=descs, channels=case.c, out=out)
    torch.cuda.synchronize()
    return split_rungs(out, K, T)[0]


def assert_rung(got, exp, c, what):
    assert_tiles_equal(got, exp, c, what)
    valid = got[1].astype(np.int64) * got[2] * c  # nothing beyond a tile's valid bytes is written
    beyond = np.arange(got[3].shape[1])[None, :] >= valid[:, None]
    assert (got[3][beyond] == POISON).all(), f"{what}: bytes beyond the stored tiles were written"


def check_ladder(gpu, case, factors, expected, what, on_device=True):
    """expected: per rung the oracle composition's tiles"""
    dev = upload_tiles(case.inputs)
    rungs, flags, status = ladder(gpu, case, dev, factors)
    assert status == 0 and (flags == 0).all(), f"{what}: status {status}, flags {flags}"
    chain = chained_ladder(gpu, case, dev, factors) if on_device else None
    for r, f in enumerate(factors):
        assert_rung(rungs[r], expected[r], case.c, f"{what} rung {r} (factor {f}) against the oracle")
        if on_device:
            assert_rung(rungs[r], retile_at(gpu, case, dev, f), case.c, f"{what} rung {r} (factor {f}) against the one-factor re-tile")
            assert_tiles_equal(rungs[r], chain[r], case.c, f"{what} rung {r} (factor {f}) against expand-varied + the varied ladder")
    return rungs


# ---- 1. parity ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_every_rung_equals_the_oracle_and_the_calls_that_were_there(gpu, case):
    """every pair of blocks, channel count, mode and family; on the 32x32 <-> 16x16 and 32x32 <-> 48x20 pairs the five filters on
    both sides and Nearest in / Lanczos3 out, Lanczos3 elsewhere"""
    fam, mode, pair, c = case
    for (xf, sf) in filter_pairs(pair):
        lad = cached_retile_ladder(fam, mode, pair, c, xf, sf)
        check_ladder(gpu, lad.case, lad.factors, lad.rungs, f"{case_id(case)} filters {xf}/{sf}")


# ---- 2. the same block ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("c", [3, 4])
@pytest.mark.parametrize("fam", "AB")
def test_same_block_equals_the_reshrink_ladder(gpu, fam, mode, c):
    import torch
    lad = cached_retile_ladder(fam, mode, ((32, 32), (32, 32)), c, LANCZOS3, LANCZOS3)
    case, K = lad.case, len(lad.factors)
    dev = upload_tiles(case.inputs)
    rungs, flags, status = ladder(gpu, case, dev, lad.factors)
    assert status == 0 and (flags == 0).all()
    T = dev[0].numel()
    out, rflags = poisoned((K + 1) * T, 32 * 32 * c, len(case.sizes))
    gpu.reshrink_varied_ladder_frames_device(case.sizes, c, 32, 32, mode, case.filt, lad.factors, case.expand_filter, *dev, out=out, image_flags=rflags)
    torch.cuda.synchronize()
    for r, exp in enumerate(split_rungs(out, K, T)[0]):
        assert_rung(rungs[r], exp, c, f"rung {r} at the same block against the re-shrink ladder out of place")


# ---- 3. rung handling -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("c", [3, 4])
def test_one_rung_thirty_two_rungs_repeats_and_order(gpu, mode, c):
    lad = cached_retile_ladder("B", mode, ((32, 32), (48, 20)), c, LANCZOS3, LANCZOS3)
    for r in (0, 5):  # K = 1
        check_ladder(gpu, lad.case, [lad.factors[r]], [lad.rungs[r]], f"K = 1, factor {lad.factors[r]}")
    pick = [int(i) % 8 for i in np.random.default_rng(5).permutation(32)]  # K = 32: every factor four times, in no order
    check_ladder(gpu, lad.case, [lad.factors[i] for i in pick], [lad.rungs[i] for i in pick], "K = 32", on_device=False)
    pick = [6, 2, 7, 0, 5, 1, 4, 3]  # the same list in another order: the rungs permuted
    check_ladder(gpu, lad.case, [lad.factors[i] for i in pick], [lad.rungs[i] for i in pick], "reordered", on_device=False)
    pick = [7, 7, 0, 7, 3, 0]  # repeats side by side and apart, the last rung a repeat of the first-met key
    got = check_ladder(gpu, lad.case, [lad.factors[i] for i in pick], [lad.rungs[i] for i in pick], "repeated factors", on_device=False)
    for (p, q) in [(0, 1), (0, 3), (2, 5)]:
        assert_tiles_equal(got[p], got[q], c, f"rungs {p} and {q} of one factor")


@pytest.mark.parametrize("mode", MODES)
def test_values_and_sizes_only(gpu, mode):
    lad = cached_retile_ladder("A", mode, ((32, 32), (48, 20)), 4, LANCZOS3, LANCZOS3)
    rungs, flags, status = ladder(gpu, lad.case, upload_tiles(lad.case.inputs), lad.factors, want_pixels=False)
    assert status == 0 and (flags == 0).all()
    for got, exp in zip(rungs, lad.rungs):
        assert (got[0].view(np.uint32) == exp[0].view(np.uint32)).all() and (got[1] == exp[1]).all() and (got[2] == exp[2]).all()


# ---- 4. tile counts -------------------------------------------------------------------------------------------------------

def test_more_destination_tiles_than_blocks(gpu, oracle):
    """800x800 at 32x32 -> 16x16: 2500 destination tiles, more than the largest grid (8 blocks on each of 256 CUs), so blocks walk
    the grid-stride loop, and rung r's outputs start 2500 tiles behind rung r - 1's"""
    case = RetileCase(oracle, "A", SHRINK_BY, ((32, 32), (16, 16)), 3, LANCZOS3, LANCZOS3, sizes=[(800, 800)])
    assert n_dst_tiles(case) == 2500 > 8 * 256
    factors = [1.0, 0.05, 0.25]
    expected = oracle_retile_rungs(oracle, case, factors)
    k = case.counts()
    assert k["src_small"] * 10 >= k["n_src"] and k["src_full"] * 10 >= k["n_src"], k
    fw, fh = case.cat(case.dst_full, 0), case.cat(case.dst_full, 1)
    clone = np.stack([(e[1] == fw) & (e[2] == fh) for e in expected])
    assert (clone.any(axis=0) & (~clone).any(axis=0)).sum() * 10 >= 2500
    check_ladder(gpu, case, factors, expected, "800x800 at 32x32 -> 16x16", on_device=False)


def test_forty_one_tile_images(gpu, oracle):
    """the owner search: every tile, in both layouts, belongs to another image"""
    sizes = [(1 + (7 * i) % 16, 1 + (5 * i) % 16) for i in range(40)]
    case = RetileCase(oracle, "B", SHRINK_BY, ((16, 16), (32, 32)), 3, LANCZOS3, LANCZOS3, sizes=sizes)
    assert all(x[1].size == 1 for x in case.inputs) and n_dst_tiles(case) == 40
    check_ladder(gpu, case, FACTORS[SHRINK_BY], oracle_retile_rungs(oracle, case, FACTORS[SHRINK_BY]), "40 one-tile images")


# ---- 5. flagged source tiles ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", [3, 4])
@pytest.mark.parametrize("pair", [((32, 32), (48, 20)), ((32, 32), (16, 16)), ((16, 16), (32, 32))], ids=lambda p: f"{p[0][0]}x{p[0][1]}to{p[1][0]}x{p[1][1]}")
def test_flagged_source_tiles(gpu, product, pair, c):
    """two source tiles of one image carry stored sizes that cannot be: a stored width of zero, and -- an edge tile -- a stored
    width one pixel beyond its place in the source grid (still within the block).  Exactly the destination tiles that cover
    them come back 0 x 0 with value bits 0 at EVERY rung and their slots untouched"""
    lad = cached_retile_ladder("B", SHRINK_BY, pair, c, LANCZOS3, LANCZOS3)
    case, K = lad.case, len(lad.factors)
    (sw, sh), (dw, dh) = pair
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
    rungs, flags, status = ladder(gpu, case, (tw, th, slots), lad.factors)
    assert status == 1
    assert [int(f) for f in flags] == [1 if i == victim else 0 for i in range(len(case.sizes))]
    keep = np.ones(rungs[0][1].size, bool)
    keep[hit] = False
    for r in range(K):
        got = rungs[r]
        for t in hit:
            assert got[1][t] == 0 and got[2][t] == 0 and got[0].view(np.uint32)[t] == 0, (r, t)
            assert (got[3][t] == POISON).all(), (r, t)
        assert_rung(tuple(x[keep] for x in got), tuple(x[keep] for x in lad.rungs[r]), c, f"tiles that cover no flagged source tile, rung {r}")
    # and the next clean call starts from a clean status
    rungs, flags, status = ladder(gpu, case, upload_tiles(case.inputs), lad.factors)
    assert status == 0 and (flags == 0).all()
    for r in range(K):
        assert_rung(rungs[r], lad.rungs[r], c, f"the clean run after a flagged one, rung {r}")


# ---- 6. validation --------------------------------------------------------------------------------------------------------

def raw_call(gpu, product, sizes, c, sw, sh, bw, bh, mode, filt, xf, factors, tw, th, slots, out, flags, n_images=None, null=None, params=True,
             n_factors=None):
    vals, ow, oh, ns = out
    geoms = [(w, h, w * c, 0) for (w, h) in sizes]
    pd = product.binding.Params(bw, bh, mode, filt, float("nan"), 0)  # (params->factor is ignored)
    fac = None if factors is None else np.ascontiguousarray(factors, np.float32)
    ptr = {"descs": C.cast(product.image_descs(geoms), C.c_void_p), "tw": C.c_void_p(tw.data_ptr()), "th": C.c_void_p(th.data_ptr()),
           "slots": C.c_void_p(slots.data_ptr()), "vals": C.c_void_p(vals.data_ptr()), "ow": C.c_void_p(ow.data_ptr()),
           "oh": C.c_void_p(oh.data_ptr())}
    if null:
        ptr[null] = None
    rc = gpu._L.pxz_retile_varied_ladder_frames_device(
        gpu._h, ptr["descs"], len(geoms) if n_images is None else n_images, c, sw, sh, C.byref(pd) if params else None, xf,
        fac.ctypes.data_as(C.c_void_p) if fac is not None and fac.size else None, (0 if fac is None else fac.size) if n_factors is None else n_factors,
        ptr["tw"], ptr["th"], ptr["slots"], ptr["vals"], ptr["ow"], ptr["oh"], C.c_void_p(ns.data_ptr()), C.c_void_p(flags.data_ptr()))
    return rc, (gpu._L.pxz_last_error(gpu._h) or b"").decode()


def test_validation_runs_before_anything_is_written(gpu, product):
    import torch
    sw, sh, bw, bh, c, K = 32, 32, 16, 16, 4, 3
    sizes = [(40, 40), (33, 64), (64, 64)]  # image 1 has a 1-px edge column in both grids
    S, T = 4 + 4 + 4, 9 + 12 + 16
    tw = torch.ones(S, dtype=torch.int32, device="cuda")
    th = torch.ones(S, dtype=torch.int32, device="cuda")
    slots = torch.zeros((S, 128 * 128 * c), dtype=torch.uint8, device="cuda")  # (room for the largest source block below)
    out, flags = poisoned(33 * T, bw * bh * c, len(sizes))
    base = dict(sizes=sizes, c=c, sw=sw, sh=sh, bw=bw, bh=bh, mode=SHRINK_BY, filt=LANCZOS3, xf=LANCZOS3, factors=[1.0, 0.5, 0.25], tw=tw, th=th,
                slots=slots, out=out, flags=flags)

    def expect(code, text, **change):
        rc, err = raw_call(gpu, product, **{**base, **change})
        assert rc == code and text in err, (rc, err, change)
        torch.cuda.synchronize()
        assert_still_poisoned(out, flags)

    # the re-tile's cases
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
    expect(INVALID_ARG, "image 1: empty image", sizes=[(40, 40), (0, 7), (64, 64)])
    expect(TILE_TOO_SMALL, "image 1: directional detector needs tiles of at least 2x2 px", mode=DIRECTIONAL)
    # the ladder's
    expect(INVALID_ARG, "null factors", factors=None, n_factors=3)
    expect(INVALID_ARG, "n_factors must be 1..32", factors=[1.0], n_factors=0)
    expect(INVALID_ARG, "n_factors must be 1..32", factors=[1.0] * 33)
    expect(INVALID_ARG, "factor 1 must be finite", factors=[1.0, float("nan"), 0.5])
    expect(INVALID_ARG, "factor 2 must be finite", factors=[1.0, 0.5, float("inf")])
    # a pair beyond the footprint: a source plane above 64 KB, and two blocks whose parts are as large as a 64 KB source tile
    assert product.retile_ladder_lds_bytes(129, 128, bw, bh, c, SHRINK_BY, LANCZOS3) > LDS_PER_CU
    expect(UNSUPPORTED, "160 KB", sw=129, sh=128)
    assert product.retile_ladder_lds_bytes(128, 128, 128, 127, c, SHRINK_BY, LANCZOS3) > LDS_PER_CU
    expect(UNSUPPORTED, "160 KB", sw=128, sh=128, bw=128, bh=127)
    # the same batch is fine for shrink_by (params->factor, a NaN here, is ignored): every source tile is 1 x 1, every destination
    # tile comes out 1 x 1 at every rung, and the rungs behind the third are left alone
    rc, err = raw_call(gpu, product, **base)
    assert rc == 0, err
    torch.cuda.synchronize()
    ow = out[1].cpu().numpy()
    assert (ow[: K * T] == 1).all() and (out[2].cpu().numpy()[: K * T] == 1).all() and (flags.cpu().numpy() == 0).all()
    assert (ow[K * T:].view(np.uint32) == SIZE_POISON).all()


# ---- 7. the host form -----------------------------------------------------------------------------------------------------

def oracle_ladder_files(oracle, case, rungs, filter_byte):
    """per rung the oracle composition's files at the destination block, from the rungs' concatenated tiles"""
    (dw, dh) = case.dst
    counts = [-(-w // dw) * -(-h // dh) for (w, h) in case.sizes]
    cuts = np.cumsum([0] + counts)
    return [[oracle.encode_container(w, h, dw, dh, case.c, filter_byte, vals[a:b], None, ow[a:b], oh[a:b], ns[a:b])
             for (w, h), a, b in zip(case.sizes, cuts[:-1], cuts[1:])] for (vals, ow, oh, ns) in rungs]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("pair", [((64, 64), (32, 32)), ((32, 32), (48, 20))], ids=["64to32", "32to48x20"])
def test_files_in_files_out(gpu, product, oracle, pair, mode):
    """files at the CLI's default 64x64 come back at 32x32 at every factor (the new block divides the files': reader, re-tile
    ladder, writer), and files at 32x32 at 48x20 (a straddling pair: the four calls)"""
    assert product.retile_ladder_lds_bytes(*pair[0], *pair[1], 4, mode, LANCZOS3) <= LDS_PER_CU
    for c in (3, 4):
        lad = cached_retile_ladder("A", mode, pair, c, LANCZOS3, LANCZOS3)
        case, factors = lad.case, lad.factors
        exp = oracle_ladder_files(oracle, case, lad.rungs, 2)
        got = gpu.transcode_varied_ladder_files(case.files, *pair[1], mode, case.filt, factors, case.expand_filter, filter_byte=2)
        assert [[len(f) for f in rung] for rung in got] == [[len(f) for f in rung] for rung in exp]
        assert got == exp
        # the size query is the rate table at the new block size: the offsets are the real ones and no byte is written
        table = gpu.transcode_varied_ladder_files(case.files, *pair[1], mode, case.filt, factors, case.expand_filter, filter_byte=2, sizes_only=True)
        assert table.shape == (len(factors), len(case.files)) and table.tolist() == [[len(f) for f in rung] for rung in exp]
        total = int(table.sum())
        short = np.full(total - 1, POISON, np.uint8)
        with pytest.raises(product.PxzError) as e:
            gpu.transcode_varied_ladder_files(case.files, *pair[1], mode, case.filt, factors, case.expand_filter, filter_byte=2, out=short)
        assert e.value.code == BUFFER_TOO_SMALL and e.value.needed == total and (short == POISON).all()
        assert np.diff(e.value.offsets.astype(np.int64)).reshape(table.shape).tolist() == table.tolist()
        # and a rung is the one-factor host form's answer
        assert gpu.transcode_varied_files(case.files, *pair[1], mode, case.filt, factors[3], case.expand_filter, filter_byte=2) == got[3]


def test_files_in_files_out_beyond_the_footprint(gpu, product, oracle):
    """a pair the footprint refuses still comes back as the oracle's files, through the image batch in handle scratch"""
    pair, mode = ((128, 128), (128, 127)), SHRINK_BY
    assert product.retile_ladder_lds_bytes(*pair[0], *pair[1], 4, mode, LANCZOS3) > LDS_PER_CU
    case = RetileCase(oracle, "A", mode, pair, 4, LANCZOS3, LANCZOS3, sizes=[(130, 129), (200, 140), (97, 260)])
    factors = [1.0, 0.125, 2.0]
    rungs = oracle_retile_rungs(oracle, case, factors)
    assert len({tuple(r[1]) + tuple(r[2]) for r in rungs}) >= 2  # (the rungs differ)
    got = gpu.transcode_varied_ladder_files(case.files, *pair[1], mode, case.filt, factors, case.expand_filter, filter_byte=3)
    assert got == oracle_ladder_files(oracle, case, rungs, 3)


# ---- 8. handle hygiene ----------------------------------------------------------------------------------------------------

def test_single_geometry_state_is_left_alone(gpu):
    """a single-geometry 32x32 shrink before and after re-tile ladders on the same handle: the same results, the same handle
    state; and a trim between two ladders changes nothing"""
    import torch
    frames = gpu.synth_frames_device(3, 96, 160, 4)

    def single():
        out = gpu.shrink_frames_device(frames, 32, 32, SHRINK_BY, LANCZOS3, 1.0)
        torch.cuda.synchronize()
        return [x.cpu().numpy().copy() for x in out], gpu.state()

    single()  # (the first launch on a handle has no statistics of a launch before it)
    before, state_before = single()
    for pair in [((32, 32), (16, 16)), ((16, 16), (32, 32))]:
        lad = cached_retile_ladder("A", SHRINK_BY, pair, 4, LANCZOS3, LANCZOS3)
        for _ in range(2):
            rungs, flags, status = ladder(gpu, lad.case, upload_tiles(lad.case.inputs), lad.factors)
            assert status == 0
            for r in range(len(lad.factors)):
                assert_rung(rungs[r], lad.rungs[r], 4, f"rung {r}")
            gpu.trim()
    after, state_after = single()
    assert state_after == state_before
    assert (before[1] == after[1]).all() and (before[2] == after[2]).all()
    assert (before[0].view(np.uint32) == after[0].view(np.uint32)).all()
    valid = before[1].astype(np.int64) * before[2] * 4
    idx = np.arange(before[3].shape[-1])[None, None, :] < valid[..., None]
    assert (before[3][idx] == after[3][idx]).all()
