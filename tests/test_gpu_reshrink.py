"""Re-shrink of stored tiles on the device (pxz_reshrink_varied_frames_device, pxz_transcode_varied_files): value bits, sizes and
the valid bytes of every slot equal the oracle composition

    oracle.decode_container -> oracle.expand_image(expand_filter) -> oracle.shrink_image(mode, filter, factor) -> oracle.encode_container

and the composition of the calls that existed before (pxz_expand_varied_frames_device + pxz_shrink_varied_frames_device), with
every output poisoned before each call.  The batches and what they must exercise are those of tests/test_reshrink_host.py, which
holds them against their conditions without a GPU."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_varied_decode import POISON, assert_tiles_equal, poisoned
from test_reshrink_host import (CASES, DIRECTIONAL, FILTER_PAIRS, LANCZOS3, LIMIT_BLOCK, NEAREST, SHRINK_BY, TRIANGLE, Case, cached_case,
                                case_id, full_sizes)
from test_reshrink_ladder_host import FACTORS, oracle_rungs
from test_varied_decode_host import ANY, FULL, HALVED, draw_tiles

pytestmark = pytest.mark.gpu

INVALID_ARG, TILE_TOO_SMALL, UNSUPPORTED, BUFFER_TOO_SMALL = -1, -4, -5, -7
VAL_POISON, SIZE_POISON = 0x7F7F7F7F, 0x5A5A5A5A


@pytest.fixture(scope="module")
def gpu(product):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    h = product.Handle(0)
    yield h
    h.close()


# ---- helpers --------------------------------------------------------------------------------------------------------------

def upload_tiles(inputs):
    """the stored tiles of a batch (per image: values, w, h, slots) -> CUDA tensors in the varied layout"""
    import torch
    tw = torch.tensor(np.concatenate([x[1] for x in inputs]).astype(np.int32)).cuda()
    th = torch.tensor(np.concatenate([x[2] for x in inputs]).astype(np.int32)).cuda()
    slots = torch.tensor(np.concatenate([x[3] for x in inputs])).cuda()
    return tw, th, slots


def to_host(out):
    vals, ow, oh, slots = out
    return (vals.cpu().numpy(), ow.cpu().numpy().astype(np.uint32), oh.cpu().numpy().astype(np.uint32),
            None if slots is None else slots.cpu().numpy())


def cat_expected(expected):
    return tuple(np.concatenate([x[k] for x in expected]) for k in range(4))


def reshrink(gpu, case, dev_tiles, factor=None, want_pixels=True, in_place=False):
    """-> ((values, w, h, slots) on the host, per-image flags, pxz_decode_status)"""
    import torch
    tw, th, slots = dev_tiles
    T = tw.numel()
    out, flags = poisoned(T, case.bw * case.bh * case.c, len(case.sizes))
    if in_place:
        out = (out[0], tw, th, slots)
    elif not want_pixels:
        out = (out[0], out[1], out[2], None)
    gpu.reshrink_varied_frames_device(case.sizes, case.c, case.bw, case.bh, case.mode, case.filt, case.factor if factor is None else factor,
                                      case.expand_filter, tw, th, slots, out=out, image_flags=flags)
    status = gpu.decode_status()
    torch.cuda.synchronize()
    return to_host(out), flags.cpu().numpy(), status


def chained(gpu, case, dev_tiles):
    """the calls that were there before: expand-varied into a tightly packed image batch, shrink-varied on it"""
    import torch
    tw, th, slots = dev_tiles
    descs, at = [], 0
    for (w, h) in case.sizes:
        descs.append((w, h, w * case.c, at))
        at += w * h * case.c
    images = torch.full((at,), POISON, dtype=torch.uint8, device="cuda")
    gpu.expand_varied_frames_device(descs, case.c, case.bw, case.bh, case.expand_filter, tw, th, slots, images)
    out, _ = poisoned(tw.numel(), case.bw * case.bh * case.c, len(case.sizes))
    gpu.shrink_varied_frames_device(images, case.bw, case.bh, case.mode, case.filt, case.factor, descs=descs, channels=case.c, out=out)
    torch.cuda.synchronize()
    return to_host(out)


def check_case(gpu, case, what, with_chain=True):
    dev = upload_tiles(case.inputs)
    got, flags, status = reshrink(gpu, case, dev)
    assert status == 0 and (flags == 0).all(), f"{what}: status {status}, flags {flags}"
    assert_tiles_equal(got, cat_expected(case.expected), case.c, f"{what} against the oracle")
    # nothing beyond a tile's valid bytes is written
    valid = got[1].astype(np.int64) * got[2] * case.c
    beyond = np.arange(got[3].shape[1])[None, :] >= valid[:, None]
    assert (got[3][beyond] == POISON).all(), f"{what}: bytes beyond the stored tiles were written"
    if with_chain:
        assert_tiles_equal(got, chained(gpu, case, dev), case.c, f"{what} against expand-varied + shrink-varied")
    return dev, got


def drawn_case(oracle, sizes, tile, c, mode, expand_filter, filt, classes, seed):
    """images of drawn tiles (random bytes, stored at the sizes their classes say), as a Case without the one-factor expectation"""
    case = Case.__new__(Case)
    bw, bh = tile
    rng = np.random.default_rng(seed)
    case.family, case.mode, case.bw, case.bh, case.c, case.expand_filter, case.filt, case.factor = "B", mode, bw, bh, c, expand_filter, filt, None
    case.sizes, case.inputs, case.full = list(sizes), [], []
    for (w, h), cl in zip(sizes, classes):
        vals, tw, th, slots, _ = draw_tiles(rng, w, h, bw, bh, c, None if cl is None else np.array(cl))
        case.inputs.append((vals, tw, th, slots))
        case.full.append(full_sizes(w, h, bw, bh))
    return case


# ---- parity ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_parity_with_the_oracle_and_the_chained_calls(gpu, case):
    """every tile size, channel count, mode and family; the five filters on both sides and Nearest in / Lanczos3 out"""
    fam, mode, tile, c = case
    for (xf, sf) in FILTER_PAIRS:
        check_case(gpu, cached_case(fam, mode, tile, c, xf, sf), f"{case_id(case)} filters {xf}/{sf}")


@pytest.mark.parametrize("mode", [SHRINK_BY, DIRECTIONAL])
def test_values_and_sizes_only(gpu, mode):
    case = cached_case("A", mode, (32, 32), 4, LANCZOS3, LANCZOS3)
    got, flags, status = reshrink(gpu, case, upload_tiles(case.inputs), want_pixels=False)
    exp = cat_expected(case.expected)
    assert status == 0 and (flags == 0).all()
    assert (got[0].view(np.uint32) == exp[0].view(np.uint32)).all() and (got[1] == exp[1]).all() and (got[2] == exp[2]).all()


@pytest.mark.parametrize("mode", [SHRINK_BY, DIRECTIONAL])
@pytest.mark.parametrize("c", [3, 4])
def test_in_place_equals_out_of_place(gpu, mode, c):
    """the outputs alias the inputs: a tile's inputs are in LDS before its block stores anything"""
    case = cached_case("A", mode, (37, 61), c, LANCZOS3, LANCZOS3)
    apart, _, _ = reshrink(gpu, case, upload_tiles(case.inputs))
    together, flags, status = reshrink(gpu, case, upload_tiles(case.inputs), in_place=True)
    assert status == 0 and (flags == 0).all()
    assert_tiles_equal(together, apart, c, "in place against out of place")
    assert_tiles_equal(together, cat_expected(case.expected), c, "in place against the oracle")


# ---- tiny odd blocks ------------------------------------------------------------------------------------------------------

TINY = [((3, 5), 4, (7, 11), SHRINK_BY), ((5, 3), 3, (23, 11), SHRINK_BY), ((5, 3), 3, (23, 11), DIRECTIONAL), ((3, 3), 4, (7, 7), SHRINK_BY)]


def check_drawn(gpu, oracle, case, factors, what):
    """drawn tiles at every factor of the list against the oracle composition; some tile of the batch must be expanded"""
    fw, fh = case.cat(case.full, 0), case.cat(case.full, 1)
    tw, th = case.cat(case.inputs, 1), case.cat(case.inputs, 2)
    assert ((tw < fw) | (th < fh)).any(), f"{what}: every tile is stored at its full size"
    dev = upload_tiles(case.inputs)
    for f, exp in zip(factors, oracle_rungs(oracle, case, factors)):
        got, flags, status = reshrink(gpu, case, dev, factor=f)
        assert status == 0 and (flags == 0).all(), f"{what} factor {f}: status {status}, flags {flags}"
        assert_tiles_equal(got, exp, case.c, f"{what} factor {f} against the oracle")
        valid = got[1].astype(np.int64) * got[2] * case.c
        beyond = np.arange(got[3].shape[1])[None, :] >= valid[:, None]
        assert (got[3][beyond] == POISON).all(), f"{what} factor {f}: bytes beyond the stored tiles were written"


@pytest.mark.parametrize("tile,c,size,mode", TINY, ids=lambda v: str(v).replace(" ", ""))
def test_tiny_odd_blocks(gpu, oracle, tile, c, size, mode):
    """blocks of a few pixels whose rows are no multiple of a dword, noise tiles stored at mixed sizes: the expand reads RGB
    pixels at every byte alignment, and the planes are smaller than the detector's.  (The 1-px edge tiles of
    7x11 and 7x7 are for shrink_by only: the directional detector refuses them.)"""
    for (xf, sf) in [(LANCZOS3, LANCZOS3), (NEAREST, TRIANGLE), (TRIANGLE, NEAREST)]:
        case = drawn_case(oracle, [size, size], tile, c, mode, xf, sf, [None, None], seed=tile[0] * 100 + tile[1] * 10 + c)
        check_drawn(gpu, oracle, case, FACTORS[mode], f"{tile} c{c} in {size} mode {mode} filters {xf}/{sf}")


def test_slots_of_45_bytes_meet_every_alignment(gpu, oracle):
    """3x5 RGB: slot t starts at a multiple of 45 bytes, so the expand's loads and the store meet every alignment of a slot"""
    case = drawn_case(oracle, [(7, 11), (6, 10)], (3, 5), 3, SHRINK_BY, LANCZOS3, LANCZOS3, [None, None], seed=45)
    T = sum(x[1].size for x in case.inputs)
    assert {(t * 45) % 4 for t in range(T)} == {0, 1, 2, 3}
    check_drawn(gpu, oracle, case, FACTORS[SHRINK_BY], "45-byte slots")


# ---- the tile loop --------------------------------------------------------------------------------------------------------

def test_more_tiles_than_blocks(gpu, oracle):
    """2500 tiles of one image: more than the largest grid (8 blocks on each of 256 CUs), so blocks walk the grid-stride loop"""
    case = Case(oracle, "A", SHRINK_BY, (16, 16), 4, LANCZOS3, LANCZOS3, sizes=[(800, 800)])
    assert sum(x[1].size for x in case.inputs) == 2500 > 8 * 256
    k = case.counts()
    assert k["in_full"] * 10 >= k["n"] and k["changed"] * 3 >= k["n"], k
    check_case(gpu, case, "800x800 at 16x16")


def test_forty_one_tile_images(gpu, oracle):
    """the owner search: every tile belongs to another image"""
    sizes = [(1 + (7 * i) % 16, 1 + (5 * i) % 16) for i in range(40)]
    case = Case(oracle, "B", SHRINK_BY, (16, 16), 3, LANCZOS3, LANCZOS3, sizes=sizes)
    assert all(x[1].size == 1 for x in case.inputs)
    check_case(gpu, case, "40 one-tile images")


# ---- the limit ------------------------------------------------------------------------------------------------------------

def limit_case(oracle, tile):
    """one image a pixel or two past the block on both axes, drawn tiles of every class (Lanczos3, shrink_by, RGBA: the largest
    footprint)"""
    case = Case.__new__(Case)
    bw, bh = tile
    w, h = bw + 2, bh + 1
    rng = np.random.default_rng(77)
    vals, tw, th, slots, _ = draw_tiles(rng, w, h, bw, bh, 4, np.array([ANY, FULL, HALVED, ANY]))
    case.family, case.mode, case.bw, case.bh, case.c, case.expand_filter, case.filt, case.factor = "B", SHRINK_BY, bw, bh, 4, LANCZOS3, LANCZOS3, 0.05
    case.sizes = [(w, h)]
    case.inputs = [(vals, tw, th, slots)]
    img = oracle.expand_image(w, h, bw, bh, 4, LANCZOS3, tw, th, slots)
    case.expected = [oracle.shrink_image(img, bw, bh, SHRINK_BY, LANCZOS3, case.factor)]
    case.full = [full_sizes(w, h, bw, bh)]
    return case


def test_largest_block(gpu, oracle):
    case = limit_case(oracle, LIMIT_BLOCK)
    assert case.sizes == [(130, 129)]
    k = case.counts()
    assert k["in_full"] >= 1 and k["both"] >= 1 and k["in_full"] < k["n"], k  # the big tile is expanded and resampled, not only cloned
    assert int(case.inputs[0][1][0]) != 128 or int(case.inputs[0][2][0]) != 128
    check_case(gpu, case, "130x129 at 128x128 RGBA")


@pytest.mark.parametrize("tile", [(128, 129), (129, 128)], ids=lambda t: f"{t[0]}x{t[1]}")
def test_one_step_beyond_the_limit_is_refused(gpu, product, tile):
    import torch
    bw, bh = tile
    sizes = [(130, 130)]
    T = (-(-130 // bw)) * (-(-130 // bh))
    tw = torch.ones(T, dtype=torch.int32, device="cuda")
    slots = torch.zeros((T, bw * bh * 4), dtype=torch.uint8, device="cuda")
    out, flags = poisoned(T, bw * bh * 4, 1)
    with pytest.raises(product.PxzError) as e:
        gpu.reshrink_varied_frames_device(sizes, 4, bw, bh, SHRINK_BY, LANCZOS3, 1.0, LANCZOS3, tw, tw.clone(), slots, out=out, image_flags=flags)
    assert e.value.code == UNSUPPORTED and "65536" in str(e.value)
    torch.cuda.synchronize()
    assert_still_poisoned(out, flags)


def assert_still_poisoned(out, flags):
    vals, ow, oh, slots = out
    assert (vals.cpu().numpy().view(np.uint32) == VAL_POISON).all()
    assert (ow.cpu().numpy().view(np.uint32) == SIZE_POISON).all() and (oh.cpu().numpy().view(np.uint32) == SIZE_POISON).all()
    assert (slots.cpu().numpy() == POISON).all()
    assert (flags.cpu().numpy().view(np.uint32) == SIZE_POISON).all()


# ---- flagged tiles --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", [3, 4])
def test_flagged_tiles(gpu, product, c):
    """two tiles of one image carry stored sizes that cannot be: 0x0, and one pixel wider than the tile's place"""
    case = cached_case("B", SHRINK_BY, (32, 32), c, LANCZOS3, LANCZOS3)
    clean, flags, status = reshrink(gpu, case, upload_tiles(case.inputs))
    assert status == 0 and (flags == 0).all()
    to = product.varied_layout([(w, h, w * c, 0) for (w, h) in case.sizes], 32, 32)
    victim = max(range(len(case.sizes)), key=lambda i: int(to[i + 1] - to[i]))
    a, b = int(to[victim]), int(to[victim + 1])
    assert b - a >= 3
    tw, th, slots = upload_tiles(case.inputs)
    fw = np.concatenate([f[0] for f in case.full])
    tw[a] = 0
    th[a] = 0
    tw[b - 1] = int(fw[b - 1]) + 1
    got, flags, status = reshrink(gpu, case, (tw, th, slots))
    assert status == 1
    assert [int(f) for f in flags] == [1 if i == victim else 0 for i in range(len(case.sizes))]
    for t in (a, b - 1):
        assert got[1][t] == 0 and got[2][t] == 0 and got[0].view(np.uint32)[t] == 0
        assert (got[3][t] == POISON).all()
    keep = np.ones(got[1].size, bool)
    keep[[a, b - 1]] = False
    assert_tiles_equal(tuple(x[keep] for x in got), tuple(x[keep] for x in clean), c, "tiles beside the flagged ones")
    # and the next clean call starts from a clean status
    again, flags, status = reshrink(gpu, case, upload_tiles(case.inputs))
    assert status == 0 and (flags == 0).all()
    assert_tiles_equal(again, clean, c, "the clean run after a flagged one")


# ---- validation -----------------------------------------------------------------------------------------------------------

def raw_call(gpu, product, sizes, c, bw, bh, mode, filt, factor, xf, tw, th, slots, out, flags, n_images=None, null=None, params=True):
    vals, ow, oh, ns = out
    geoms = [(w, h, w * c, 0) for (w, h) in sizes]
    pd = product.binding.Params(bw, bh, mode, filt, factor, 0)
    ptr = {"descs": C.cast(product.image_descs(geoms), C.c_void_p), "tw": C.c_void_p(tw.data_ptr()), "th": C.c_void_p(th.data_ptr()),
           "slots": C.c_void_p(slots.data_ptr()), "vals": C.c_void_p(vals.data_ptr()), "ow": C.c_void_p(ow.data_ptr()),
           "oh": C.c_void_p(oh.data_ptr())}
    if null:
        ptr[null] = None
    rc = gpu._L.pxz_reshrink_varied_frames_device(gpu._h, ptr["descs"], len(geoms) if n_images is None else n_images, c,
                                                  C.byref(pd) if params else None, xf, ptr["tw"], ptr["th"], ptr["slots"], ptr["vals"],
                                                  ptr["ow"], ptr["oh"], C.c_void_p(ns.data_ptr()), C.c_void_p(flags.data_ptr()))
    return rc, (gpu._L.pxz_last_error(gpu._h) or b"").decode()


def test_validation_runs_before_anything_is_written(gpu, product):
    import torch
    bw, bh, c = 32, 32, 4
    sizes = [(40, 40), (33, 64), (64, 64)]  # image 1 has a 1-px edge column
    T = 4 + 4 + 4
    tw = torch.ones(T, dtype=torch.int32, device="cuda")
    th = torch.ones(T, dtype=torch.int32, device="cuda")
    slots = torch.zeros((T, bw * bh * c), dtype=torch.uint8, device="cuda")
    out, flags = poisoned(T, bw * bh * c, len(sizes))
    base = dict(sizes=sizes, c=c, bw=bw, bh=bh, mode=SHRINK_BY, filt=LANCZOS3, factor=1.0, xf=LANCZOS3, tw=tw, th=th, slots=slots, out=out,
                flags=flags)

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
    expect(INVALID_ARG, "expand_filter", xf=5)
    expect(INVALID_ARG, "filter must be 0..4", filt=5)
    expect(INVALID_ARG, "channels must be 3 or 4", c=5)
    expect(INVALID_ARG, "factor must be finite", factor=float("nan"))
    expect(INVALID_ARG, "image 1: empty image", sizes=[(40, 40), (0, 7), (64, 64)])
    expect(TILE_TOO_SMALL, "image 1: directional detector needs tiles of at least 2x2 px", mode=DIRECTIONAL)
    # the same batch is fine for shrink_by
    rc, err = raw_call(gpu, product, **base)
    assert rc == 0, err
    torch.cuda.synchronize()
    assert (out[1].cpu().numpy() == 1).all() and (flags.cpu().numpy() == 0).all()


# ---- host form ------------------------------------------------------------------------------------------------------------

def oracle_files(oracle, case, bw, bh, filter_byte):
    """the oracle composition's files at block bw x bh"""
    files = []
    for raw, (w, h) in zip(case.files, case.sizes):
        d = oracle.decode_container(raw)
        slots = np.ascontiguousarray(d["slots"][:, : case.bw * case.bh * case.c])
        img = oracle.expand_image(w, h, case.bw, case.bh, case.c, case.expand_filter, d["tw"], d["th"], slots)
        vals, ow, oh, ns = oracle.shrink_image(img, bw, bh, case.mode, case.filt, case.factor)
        files.append(oracle.encode_container(w, h, bw, bh, case.c, filter_byte, vals, None, ow, oh, ns))
    return files


@pytest.mark.parametrize("mode", [SHRINK_BY, DIRECTIONAL])
@pytest.mark.parametrize("c", [3, 4])
def test_files_in_files_out_same_block(gpu, product, oracle, mode, c):
    case = cached_case("A", mode, (32, 32), c, NEAREST, LANCZOS3)
    assert len(case.files) == 6
    exp = oracle_files(oracle, case, 32, 32, 4)
    got = gpu.transcode_varied_files(case.files, 32, 32, mode, case.filt, case.factor, case.expand_filter, filter_byte=4)
    assert [len(f) for f in got] == [len(f) for f in exp]
    assert got == exp
    total = sum(len(f) for f in exp)
    # the size query, and a buffer one byte short: the size comes back, nothing is written
    with pytest.raises(product.PxzError) as e:
        gpu.transcode_varied_files(case.files, 32, 32, mode, case.filt, case.factor, case.expand_filter, filter_byte=4, out=np.empty(0, np.uint8))
    assert e.value.code == BUFFER_TOO_SMALL and e.value.needed == total
    short = np.full(total - 1, POISON, np.uint8)
    with pytest.raises(product.PxzError) as e:
        gpu.transcode_varied_files(case.files, 32, 32, mode, case.filt, case.factor, case.expand_filter, filter_byte=4, out=short)
    assert e.value.code == BUFFER_TOO_SMALL and e.value.needed == total and (short == POISON).all()
    exact = np.full(total, POISON, np.uint8)
    assert gpu.transcode_varied_files(case.files, 32, 32, mode, case.filt, case.factor, case.expand_filter, filter_byte=4, out=exact) == exp


def test_files_in_a_truncated_file_stops_the_call(gpu, product, oracle):
    case = cached_case("A", SHRINK_BY, (32, 32), 4, NEAREST, LANCZOS3)
    files = list(case.files)
    files[4] = files[4][: len(files[4]) - 9]
    out = np.full(sum(len(f) for f in files) * 2, POISON, np.uint8)
    with pytest.raises(product.PxzError) as e:
        gpu.transcode_varied_files(files, 32, 32, SHRINK_BY, case.filt, case.factor, case.expand_filter, out=out)
    assert e.value.code == INVALID_ARG and "image 4" in str(e.value)
    assert (out == POISON).all()
    # files that do not share a block size or channels are refused by their headers
    other = cached_case("A", SHRINK_BY, (16, 16), 4, LANCZOS3, LANCZOS3).files[0]
    with pytest.raises(product.PxzError) as e:
        gpu.transcode_varied_files([case.files[0], case.files[1], other], 32, 32, SHRINK_BY, case.filt, case.factor, case.expand_filter, out=out)
    assert e.value.code == INVALID_ARG and "image 2" in str(e.value) and (out == POISON).all()
    rgb = cached_case("A", SHRINK_BY, (32, 32), 3, NEAREST, LANCZOS3).files[0]
    with pytest.raises(product.PxzError) as e:
        gpu.transcode_varied_files([case.files[0], rgb], 32, 32, SHRINK_BY, case.filt, case.factor, case.expand_filter, out=out)
    assert e.value.code == INVALID_ARG and "image 1" in str(e.value) and (out == POISON).all()
    # and the handle still works
    assert gpu.transcode_varied_files(case.files, 32, 32, SHRINK_BY, case.filt, case.factor, case.expand_filter) == oracle_files(oracle, case, 32, 32, 0)


@pytest.mark.parametrize("tile", [(48, 20), (64, 64)], ids=lambda t: f"{t[0]}x{t[1]}")
@pytest.mark.parametrize("mode", [SHRINK_BY, DIRECTIONAL])
def test_files_in_files_out_other_block(gpu, oracle, mode, tile):
    """the CLI's -b on a .pix input: files at 32x32 come back at another block size"""
    case = cached_case("A", mode, (32, 32), 4, LANCZOS3, LANCZOS3)
    bw, bh = tile
    got = gpu.transcode_varied_files(case.files, bw, bh, mode, case.filt, case.factor, case.expand_filter, filter_byte=2)
    assert got == oracle_files(oracle, case, bw, bh, 2)


# ---- handle hygiene -------------------------------------------------------------------------------------------------------

def test_single_geometry_state_is_left_alone(gpu):
    """a single-geometry 32x32 shrink before and after a re-shrink on the same handle: the same results, the same handle state"""
    import torch
    frames = gpu.synth_frames_device(3, 96, 160, 4)

    def single():
        out = gpu.shrink_frames_device(frames, 32, 32, SHRINK_BY, LANCZOS3, 1.0)
        torch.cuda.synchronize()
        return [x.cpu().numpy().copy() for x in out], gpu.state()

    single()  # (the first launch on a handle has no statistics of a launch before it)
    before, state_before = single()
    case = cached_case("A", SHRINK_BY, (32, 32), 4, LANCZOS3, LANCZOS3)
    for in_place in (False, True):
        got, flags, status = reshrink(gpu, case, upload_tiles(case.inputs), in_place=in_place)
        assert status == 0
    after, state_after = single()
    assert state_after == state_before
    assert (before[1] == after[1]).all() and (before[2] == after[2]).all()
    assert (before[0].view(np.uint32) == after[0].view(np.uint32)).all()
    valid = before[1].astype(np.int64) * before[2] * 4
    idx = np.arange(before[3].shape[-1])[None, None, :] < valid[..., None]
    assert (before[3][idx] == after[3][idx]).all()
