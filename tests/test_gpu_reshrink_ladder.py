"""Re-shrink ladder on the device (pxz_reshrink_varied_ladder_frames_device, pxz_transcode_varied_ladder_files): every rung's
value bits, sizes and valid slot bytes equal pxz_reshrink_varied_frames_device at that rung's factor and the oracle composition

    oracle.decode_container -> oracle.expand_image(expand_filter) -> oracle.shrink_image(mode, filter, factors[r]) -> oracle.encode_container

Every output is poisoned before each call, and one guard rung behind the last must come back untouched.  The batches and what
they must exercise are those of tests/test_reshrink_ladder_host.py, which holds them against their conditions without a GPU."""
import numpy as np
import pytest

from test_gpu_reshrink import SIZE_POISON, TINY, VAL_POISON, assert_still_poisoned, drawn_case, reshrink, to_host, upload_tiles
from test_gpu_varied_decode import POISON, assert_tiles_equal, poisoned
from test_reshrink_host import CASES, DIRECTIONAL, FILTER_PAIRS, LANCZOS3, NEAREST, SHRINK_BY, TRIANGLE, Case, cached_case, case_id
from test_reshrink_ladder_host import FACTORS, cached_ladder, oracle_rungs
from test_varied_decode_host import ANY, FULL, HALVED

pytestmark = pytest.mark.gpu

INVALID_ARG, UNSUPPORTED, BUFFER_TOO_SMALL = -1, -5, -7
MODES = [SHRINK_BY, DIRECTIONAL]


@pytest.fixture(scope="module")
def gpu(product):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    h = product.Handle(0)
    yield h
    h.close()


# ---- helpers --------------------------------------------------------------------------------------------------------------

def ladder(gpu, case, dev_tiles, factors, want_pixels=True, in_place=False):
    """one ladder call into poisoned outputs of len(factors) rungs and a guard rung, which is checked here
    -> ([(values, w, h, slots) per rung, on the host], per-image flags, pxz_decode_status)"""
    import torch
    tw, th, slots = dev_tiles
    K, T, slot = len(factors), tw.numel(), case.bw * case.bh * case.c
    out, flags = poisoned((K + 1) * T, slot, len(case.sizes))
    if in_place:  # the inputs are rung 0 of the outputs
        out[1][:T], out[2][:T], out[3][:T] = tw, th, slots
        tw, th, slots = out[1], out[2], out[3]
    gpu.reshrink_varied_ladder_frames_device(case.sizes, case.c, case.bw, case.bh, case.mode, case.filt, factors, case.expand_filter, tw, th, slots,
                                             out=out if want_pixels else (out[0], out[1], out[2], None), image_flags=flags)
    status = gpu.decode_status()
    torch.cuda.synchronize()
    vals, ow, oh, px = to_host(out)
    assert (vals[K * T:].view(np.uint32) == VAL_POISON).all() and (ow[K * T:] == SIZE_POISON).all() and (oh[K * T:] == SIZE_POISON).all(), \
        "the guard rung's values or sizes were written"
    assert (px[K * T:] == POISON).all(), "the guard rung's slots were written"
    if not want_pixels:
        assert (px == POISON).all(), "slots were written by a call that was given none"
    rungs = [tuple(x[r * T:(r + 1) * T] for x in (vals, ow, oh, px)) for r in range(K)]
    return rungs, flags.cpu().numpy(), status


def assert_rung(got, exp, c, what, slots_were_poisoned=True):
    assert_tiles_equal(got, exp, c, what)
    if slots_were_poisoned:  # nothing beyond a tile's valid bytes is written
        valid = got[1].astype(np.int64) * got[2] * c
        beyond = np.arange(got[3].shape[1])[None, :] >= valid[:, None]
        assert (got[3][beyond] == POISON).all(), f"{what}: bytes beyond the stored tiles were written"


def check_ladder(gpu, case, factors, expected, what, against_single=True):
    """expected: per rung the oracle composition's tiles"""
    dev = upload_tiles(case.inputs)
    rungs, flags, status = ladder(gpu, case, dev, factors)
    assert status == 0 and (flags == 0).all(), f"{what}: status {status}, flags {flags}"
    for r, f in enumerate(factors):
        assert_rung(rungs[r], expected[r], case.c, f"{what} rung {r} (factor {f}) against the oracle")
        if against_single:
            single, _, _ = reshrink(gpu, case, dev, factor=f)
            assert_rung(rungs[r], single, case.c, f"{what} rung {r} (factor {f}) against the one-factor re-shrink")
    return rungs


def mixed_rungs(case, expected):
    """tiles that are stored reduced, and tiles with a clone rung beside a reduced one, among the expected rungs"""
    fw, fh = case.cat(case.full, 0), case.cat(case.full, 1)
    tw, th = case.cat(case.inputs, 1), case.cat(case.inputs, 2)
    clone = np.stack([(e[1] == fw) & (e[2] == fh) for e in expected])
    return int(((tw != fw) | (th != fh)).sum()), int((clone.any(axis=0) & (~clone).any(axis=0)).sum())


# ---- 1. parity ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_every_rung_equals_the_single_call_and_the_oracle(gpu, case):
    """every tile size, channel count, mode and family; the five filters on both sides and Nearest in / Lanczos3 out"""
    fam, mode, tile, c = case
    for (xf, sf) in FILTER_PAIRS:
        lad = cached_ladder(fam, mode, tile, c, xf, sf)
        check_ladder(gpu, lad.case, lad.factors, lad.rungs, f"{case_id(case)} filters {xf}/{sf}")


# ---- 2. tiny odd blocks ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tile,c,size,mode", TINY, ids=lambda v: str(v).replace(" ", ""))
def test_tiny_odd_blocks(gpu, oracle, tile, c, size, mode):
    """blocks whose resampled images do not fit the plane the expand leaves free (3x5 RGBA: 80 bytes beside a plane of 64) and
    whose rows are no multiple of a dword; noise tiles stored at mixed sizes.  (The 1-px edge tiles of 7x11 and 7x7 are for
    shrink_by only: the directional detector refuses them.)"""
    for (xf, sf) in [(LANCZOS3, LANCZOS3), (NEAREST, TRIANGLE), (TRIANGLE, NEAREST)]:
        case = drawn_case(oracle, [size, size], tile, c, mode, xf, sf, [None, None], seed=tile[0] * 100 + tile[1] * 10 + c)
        expected = oracle_rungs(oracle, case, FACTORS[mode])
        reduced_in, mixed = mixed_rungs(case, expected)
        assert reduced_in >= 2 and mixed >= 2, (reduced_in, mixed)
        check_ladder(gpu, case, FACTORS[mode], expected, f"{tile} c{c} in {size} mode {mode} filters {xf}/{sf}")


# ---- 3. the limit ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", [4, 3])
@pytest.mark.parametrize("mode", MODES)
def test_largest_block(gpu, oracle, mode, c):
    """128x128: two planes of 64 KB, the Oklab tables and the windows; I and F lie in the free plane"""
    size = (130, 130) if mode == SHRINK_BY else (128, 130)
    classes = [ANY, FULL, HALVED, ANY] if mode == SHRINK_BY else [ANY, HALVED]
    case = drawn_case(oracle, [size], (128, 128), c, mode, LANCZOS3, LANCZOS3, [classes], seed=77 + c)
    assert int(case.inputs[0][1][0]) != 128 or int(case.inputs[0][2][0]) != 128  # the big tile is expanded, not cloned in
    expected = oracle_rungs(oracle, case, FACTORS[mode])
    assert len({(int(e[1][0]), int(e[2][0])) for e in expected}) >= 3  # and resampled at several sizes
    check_ladder(gpu, case, FACTORS[mode], expected, f"{size} at 128x128 c{c} mode {mode}")


def test_one_step_beyond_the_limit_is_refused(gpu, product):
    import torch
    bw, bh, K = 129, 128, 3
    T = 4
    tw = torch.ones(T, dtype=torch.int32, device="cuda")
    slots = torch.zeros((T, bw * bh * 4), dtype=torch.uint8, device="cuda")
    out, flags = poisoned(K * T, bw * bh * 4, 1)
    with pytest.raises(product.PxzError) as e:
        gpu.reshrink_varied_ladder_frames_device([(130, 130)], 4, bw, bh, SHRINK_BY, LANCZOS3, [1.0, 0.5, 0.25], LANCZOS3, tw, tw.clone(), slots,
                                                 out=out, image_flags=flags)
    assert e.value.code == UNSUPPORTED and "65536" in str(e.value)
    torch.cuda.synchronize()
    assert_still_poisoned(out, flags)


# ---- 4. factor handling ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("c", [3, 4])
def test_one_rung_thirty_two_rungs_repeats_and_order(gpu, mode, c):
    lad = cached_ladder("B", mode, (32, 32), c, LANCZOS3, LANCZOS3)
    for r in (0, 5):  # K = 1
        check_ladder(gpu, lad.case, [lad.factors[r]], [lad.rungs[r]], f"K = 1, factor {lad.factors[r]}")
    pick = [int(i) % 8 for i in np.random.default_rng(5).permutation(32)]  # K = 32: every factor four times, in no order
    check_ladder(gpu, lad.case, [lad.factors[i] for i in pick], [lad.rungs[i] for i in pick], "K = 32", against_single=False)
    pick = [7, 7, 0, 7, 3, 0]  # repeats side by side and apart, the last rung a repeat of the first-met key
    check_ladder(gpu, lad.case, [lad.factors[i] for i in pick], [lad.rungs[i] for i in pick], "repeated factors", against_single=False)


@pytest.mark.parametrize("mode", MODES)
def test_values_and_sizes_only(gpu, mode):
    lad = cached_ladder("A", mode, (32, 32), 4, LANCZOS3, LANCZOS3)
    rungs, flags, status = ladder(gpu, lad.case, upload_tiles(lad.case.inputs), lad.factors, want_pixels=False)
    assert status == 0 and (flags == 0).all()
    for got, exp in zip(rungs, lad.rungs):
        assert (got[0].view(np.uint32) == exp[0].view(np.uint32)).all() and (got[1] == exp[1]).all() and (got[2] == exp[2]).all()


def test_slots_of_45_bytes_put_rungs_on_every_alignment(gpu, oracle):
    """3x5 RGB: slot (r * tiles + t) starts at a multiple of 45 bytes, so the store meets every alignment of a slot"""
    case = drawn_case(oracle, [(7, 11), (6, 10)], (3, 5), 3, SHRINK_BY, LANCZOS3, LANCZOS3, [None, None], seed=45)
    T = sum(x[1].size for x in case.inputs)
    assert {((r * T + t) * 45) % 4 for r in range(8) for t in range(T)} == {0, 1, 2, 3}
    expected = oracle_rungs(oracle, case, FACTORS[SHRINK_BY])
    assert mixed_rungs(case, expected)[1] >= 2
    check_ladder(gpu, case, FACTORS[SHRINK_BY], expected, "45-byte slots")


# ---- 5. in place ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("c", [3, 4])
def test_in_place_on_rung_0_equals_out_of_place(gpu, mode, c):
    """rung 0 of the outputs are the input arrays: a tile's inputs are in LDS before its block stores anything, and the rungs
    from 1 on lie beyond the inputs"""
    lad = cached_ladder("A", mode, (37, 61), c, LANCZOS3, LANCZOS3)
    apart, _, _ = ladder(gpu, lad.case, upload_tiles(lad.case.inputs), lad.factors)
    together, flags, status = ladder(gpu, lad.case, upload_tiles(lad.case.inputs), lad.factors, in_place=True)
    assert status == 0 and (flags == 0).all()
    for r in range(len(lad.factors)):
        assert_rung(together[r], apart[r], c, f"in place against out of place, rung {r}", slots_were_poisoned=r > 0)
        assert_tiles_equal(together[r], lad.rungs[r], c, f"in place against the oracle, rung {r}")


# ---- 6. flagged tiles -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", [3, 4])
def test_flagged_tiles(gpu, product, c):
    """two tiles of one image carry stored sizes that cannot be: 0x0, and one pixel wider than the tile's place.  Every rung of
    them is empty and its slot untouched; the other tiles, the other images included, are complete"""
    lad = cached_ladder("B", SHRINK_BY, (32, 32), c, LANCZOS3, LANCZOS3)
    case, K = lad.case, len(lad.factors)
    to = product.varied_layout([(w, h, w * c, 0) for (w, h) in case.sizes], 32, 32)
    victim = max(range(len(case.sizes)), key=lambda i: int(to[i + 1] - to[i]))
    a, b = int(to[victim]), int(to[victim + 1])
    assert b - a >= 3
    tw, th, slots = upload_tiles(case.inputs)
    fw = np.concatenate([f[0] for f in case.full])
    tw[a] = 0
    th[a] = 0
    tw[b - 1] = int(fw[b - 1]) + 1
    rungs, flags, status = ladder(gpu, case, (tw, th, slots), lad.factors)
    assert status == 1
    assert [int(f) for f in flags] == [1 if i == victim else 0 for i in range(len(case.sizes))]
    keep = np.ones(rungs[0][1].size, bool)
    keep[[a, b - 1]] = False
    for r in range(K):
        got = rungs[r]
        for t in (a, b - 1):
            assert got[1][t] == 0 and got[2][t] == 0 and got[0].view(np.uint32)[t] == 0, (r, t)
            assert (got[3][t] == POISON).all(), (r, t)
        assert_rung(tuple(x[keep] for x in got), tuple(x[keep] for x in lad.rungs[r]), c, f"tiles beside the flagged ones, rung {r}")
    # and the next clean call starts from a clean status
    rungs, flags, status = ladder(gpu, case, upload_tiles(case.inputs), lad.factors)
    assert status == 0 and (flags == 0).all()
    for r in range(K):
        assert_rung(rungs[r], lad.rungs[r], c, f"the clean run after a flagged one, rung {r}")


# ---- 7. tile counts -------------------------------------------------------------------------------------------------------

def test_more_tiles_than_blocks(gpu, oracle):
    """2500 tiles of one image: more than the largest grid (8 blocks on each of 256 CUs), so blocks walk the grid-stride loop,
    and rung r's outputs start 2500 tiles behind rung r - 1's"""
    case = Case(oracle, "A", SHRINK_BY, (8, 8), 4, LANCZOS3, LANCZOS3, sizes=[(400, 400)])
    assert sum(x[1].size for x in case.inputs) == 2500 > 8 * 256
    factors = [1.0, 0.05, 2.0, 0.25]
    expected = oracle_rungs(oracle, case, factors)
    reduced_in, mixed = mixed_rungs(case, expected)
    assert reduced_in * 10 >= 2500 and mixed * 10 >= 2500, (reduced_in, mixed)
    check_ladder(gpu, case, factors, expected, "400x400 at 8x8")


def test_forty_one_tile_images(gpu, oracle):
    """the owner search: every tile belongs to another image"""
    sizes = [(1 + (7 * i) % 16, 1 + (5 * i) % 16) for i in range(40)]
    case = Case(oracle, "B", SHRINK_BY, (16, 16), 3, LANCZOS3, LANCZOS3, sizes=sizes)
    assert all(x[1].size == 1 for x in case.inputs)
    check_ladder(gpu, case, FACTORS[SHRINK_BY], oracle_rungs(oracle, case, FACTORS[SHRINK_BY]), "40 one-tile images")


# ---- 8. the host form -----------------------------------------------------------------------------------------------------

def oracle_ladder_files(oracle, case, factors, bw, bh, filter_byte):
    """per rung the oracle composition's files at block bw x bh"""
    rungs = [[] for _ in factors]
    for raw, (w, h) in zip(case.files, case.sizes):
        d = oracle.decode_container(raw)
        slots = np.ascontiguousarray(d["slots"][:, : case.bw * case.bh * case.c])
        img = oracle.expand_image(w, h, case.bw, case.bh, case.c, case.expand_filter, d["tw"], d["th"], slots)
        for r, f in enumerate(factors):
            vals, ow, oh, ns = oracle.shrink_image(img, bw, bh, case.mode, case.filt, f)
            rungs[r].append(oracle.encode_container(w, h, bw, bh, case.c, filter_byte, vals, None, ow, oh, ns))
    return rungs


@pytest.mark.parametrize("mode,c", [(SHRINK_BY, 4), (SHRINK_BY, 3), (DIRECTIONAL, 4)])
def test_files_in_files_out_same_block(gpu, product, oracle, mode, c):
    case = cached_case("A", mode, (32, 32), c, NEAREST, LANCZOS3)
    factors = FACTORS[mode]
    exp = oracle_ladder_files(oracle, case, factors, 32, 32, 4)
    got = gpu.transcode_varied_ladder_files(case.files, 32, 32, mode, case.filt, factors, case.expand_filter, filter_byte=4)
    assert [[len(f) for f in rung] for rung in got] == [[len(f) for f in rung] for rung in exp]
    assert got == exp
    # the size query is the rate table: the offsets are the real ones and no file is kept
    table = gpu.transcode_varied_ladder_files(case.files, 32, 32, mode, case.filt, factors, case.expand_filter, filter_byte=4, sizes_only=True)
    assert table.shape == (len(factors), len(case.files)) and table.tolist() == [[len(f) for f in rung] for rung in exp]
    total = int(table.sum())
    short = np.full(total - 1, POISON, np.uint8)
    with pytest.raises(product.PxzError) as e:
        gpu.transcode_varied_ladder_files(case.files, 32, 32, mode, case.filt, factors, case.expand_filter, filter_byte=4, out=short)
    assert e.value.code == BUFFER_TOO_SMALL and e.value.needed == total and (short == POISON).all()
    assert np.diff(e.value.offsets.astype(np.int64)).reshape(table.shape).tolist() == table.tolist()
    exact = np.full(total, POISON, np.uint8)
    assert gpu.transcode_varied_ladder_files(case.files, 32, 32, mode, case.filt, factors, case.expand_filter, filter_byte=4, out=exact) == exp
    # and a rung is the one-factor host form's answer
    assert gpu.transcode_varied_files(case.files, 32, 32, mode, case.filt, factors[3], case.expand_filter, filter_byte=4) == got[3]


@pytest.mark.parametrize("mode", MODES)
def test_files_in_files_out_other_block(gpu, oracle, mode):
    """files at 32x32 come back at 48x20: reader, expand-varied, the varied ladder, writer"""
    case = cached_case("A", mode, (32, 32), 4, LANCZOS3, LANCZOS3)
    factors = FACTORS[mode][:5]
    got = gpu.transcode_varied_ladder_files(case.files, 48, 20, mode, case.filt, factors, case.expand_filter, filter_byte=2)
    assert got == oracle_ladder_files(oracle, case, factors, 48, 20, 2)


def test_a_malformed_file_writes_nothing(gpu, product, oracle):
    case = cached_case("A", SHRINK_BY, (32, 32), 4, NEAREST, LANCZOS3)
    factors = [1.0, 0.25]
    files = list(case.files)
    files[4] = files[4][: len(files[4]) - 9]
    out = np.full(sum(len(f) for f in files) * 4, POISON, np.uint8)
    with pytest.raises(product.PxzError) as e:
        gpu.transcode_varied_ladder_files(files, 32, 32, SHRINK_BY, case.filt, factors, case.expand_filter, out=out)
    assert e.value.code == INVALID_ARG and "image 4" in str(e.value)
    assert (out == POISON).all() and (e.value.offsets == 0).all()
    for bad in ([], [1.0] * 33, [1.0, float("inf")]):
        with pytest.raises(product.PxzError) as e:
            gpu.transcode_varied_ladder_files(case.files, 32, 32, SHRINK_BY, case.filt, bad, case.expand_filter, out=out)
        assert e.value.code == INVALID_ARG and (out == POISON).all()
    # and the handle still works
    assert gpu.transcode_varied_ladder_files(case.files, 32, 32, SHRINK_BY, case.filt, factors, case.expand_filter) == \
        oracle_ladder_files(oracle, case, factors, 32, 32, 0)


# ---- 9. handle hygiene ----------------------------------------------------------------------------------------------------

def test_one_handle_against_fresh_handles(gpu, product):
    """single -> re-shrink ladder -> varied ladder -> re-shrink -> trim -> re-shrink ladder -> single on one handle: every step
    gives what a fresh handle gives, and the single-geometry state is what it was"""
    import torch
    lad = cached_ladder("A", SHRINK_BY, (32, 32), 4, LANCZOS3, LANCZOS3)
    case = lad.case
    images = [torch.from_numpy(np.random.default_rng(9 + i).integers(0, 256, (h, w, 4), dtype=np.uint8)).cuda() for i, (w, h) in enumerate([(70, 41), (33, 97)])]

    def single(h):
        frames = h.synth_frames_device(3, 96, 160, 4)
        out = h.shrink_frames_device(frames, 32, 32, SHRINK_BY, LANCZOS3, 1.0)
        torch.cuda.synchronize()
        return [tuple(x.cpu().numpy().reshape((-1,) + x.shape[2:]) for x in out)]

    def reshrink_ladder(h):
        return ladder(h, case, upload_tiles(case.inputs), lad.factors)[0]

    def varied_ladder(h):
        _, vals, ow, oh, slots = h.shrink_varied_ladder_frames_device(images, 32, 32, SHRINK_BY, LANCZOS3, lad.factors)
        torch.cuda.synchronize()
        return [tuple(x.cpu().numpy().reshape((-1,) + x.shape[2:]) for x in (vals, ow, oh, slots))]

    def reshrink_once(h):
        return [reshrink(h, case, upload_tiles(case.inputs))[0]]

    def trim(h):
        h.trim()
        return []

    states = []
    for k, step in enumerate([single, single, reshrink_ladder, varied_ladder, reshrink_once, trim, reshrink_ladder, single]):
        got = step(gpu)
        fresh = product.Handle(0)
        try:
            if step is single:
                step(fresh)  # (the first launch on a handle has no statistics of a launch before it)
            exp = step(fresh)
        finally:
            fresh.close()
        assert len(got) == len(exp)
        for r, (g, e) in enumerate(zip(got, exp)):
            assert_tiles_equal(g, e, 4, f"step {k} ({step.__name__}), set {r}")
        if step is reshrink_ladder:
            for r, g in enumerate(got):
                assert_tiles_equal(g, lad.rungs[r], 4, f"step {k}, rung {r} against the oracle")
        if step is single and k > 0:
            states.append(gpu.state())
    assert len(states) == 2 and states[0] == states[1]


# ---- 10. validation -------------------------------------------------------------------------------------------------------

def test_validation_runs_before_anything_is_written(gpu, product):
    import torch
    bw, bh, c, K = 32, 32, 4, 3
    sizes = [(40, 40), (33, 64), (64, 64)]
    T = 4 + 4 + 4
    tw = torch.ones(T, dtype=torch.int32, device="cuda")
    th = torch.ones(T, dtype=torch.int32, device="cuda")
    slots = torch.zeros((T, bw * bh * c), dtype=torch.uint8, device="cuda")
    out, flags = poisoned(33 * T, bw * bh * c, len(sizes))
    base = dict(sizes=sizes, channels=c, bw=bw, bh=bh, mode=SHRINK_BY, filt=LANCZOS3, factors=[1.0, 0.5, 0.25], expand_filter=LANCZOS3)

    def expect(code, text, n_factors=None, **change):
        with pytest.raises(product.PxzError) as e:
            gpu.reshrink_varied_ladder_frames_device(ow=tw, oh=th, slots=slots, out=out, image_flags=flags, n_factors=n_factors, **{**base, **change})
        assert e.value.code == code and text in str(e.value), (str(e.value), change)
        torch.cuda.synchronize()
        assert_still_poisoned(out, flags)

    expect(INVALID_ARG, "null factors", factors=None, n_factors=3)
    expect(INVALID_ARG, "n_factors must be 1..32", factors=[1.0], n_factors=0)
    expect(INVALID_ARG, "n_factors must be 1..32", factors=[1.0] * 33)
    expect(INVALID_ARG, "factor 1 must be finite", factors=[1.0, float("nan"), 0.5])
    expect(INVALID_ARG, "expand_filter", expand_filter=5)
    expect(INVALID_ARG, "filter must be 0..4", filt=5)
    expect(INVALID_ARG, "channels must be 3 or 4", channels=5)
    expect(INVALID_ARG, "image 1: empty image", sizes=[(40, 40), (0, 7), (64, 64)])
    expect(-4, "image 1: directional detector needs tiles of at least 2x2 px", mode=DIRECTIONAL)
    # the same batch is fine for shrink_by, and params->factor is ignored (the binding passes 0)
    gpu.reshrink_varied_ladder_frames_device(ow=tw, oh=th, slots=slots, out=out, image_flags=flags, **base)
    torch.cuda.synchronize()
    assert (out[1].cpu().numpy()[: K * T] == 1).all() and (flags.cpu().numpy() == 0).all()
    assert (out[1].cpu().numpy()[K * T:].view(np.uint32) == SIZE_POISON).all()
