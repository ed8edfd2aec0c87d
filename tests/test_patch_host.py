"""The patch of pixel windows without a GPU: pxz_patch_check against the Python of tests/patch_model.py, and the footing of that
model on the fixtures the GPU tests use (tests/test_gpu_patch.py): a hull's tiles are the whole patched image's tiles, the
oracle's writer is canonical over what its reader reads, a whole-image window gives the plain encode of its pixels, and every
fixture has covered tiles stored at full size and covered tiles stored small."""
import ctypes as C

import numpy as np
import pytest

import patch_model as pm

INVALID_ARG, UNSUPPORTED = -1, -5
NAMES = ("pxz_patch_check", "pxz_patch_windows_device", "pxz_splice_windows_device", "pxz_patch_windows_files")


def win(image, x, y, w, h):
    return (image, x, y, w, h, 0, 0)


def test_library_exports_the_patch_calls(product):
    L = product.load_library()
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in product.EXPORTED_SYMBOLS, name
    for name in ("patch_windows_device", "splice_windows_device", "patch_windows_files"):
        assert callable(getattr(product.Handle, name)), name
    assert callable(product.patch_check) and product.NO_WINDOW == 0xffffffff


# 100x70 in 32x32 blocks: a 4x3 grid.  name: (windows, the first offending window or None)
CHECKS = {
    "disjoint": ([win(0, 0, 0, 10, 10), win(0, 40, 40, 10, 10)], None),
    "touching at a tile border": ([win(0, 0, 0, 32, 32), win(0, 32, 0, 32, 32), win(0, 0, 32, 64, 32)], None),
    "two inside one tile": ([win(0, 1, 1, 5, 5), win(0, 20, 20, 5, 5)], 1),
    "pixels apart, one tile shared": ([win(0, 0, 0, 33, 10), win(0, 70, 0, 5, 5), win(0, 60, 20, 3, 3)], 2),
    "different tiles of one tile row": ([win(0, 1, 33, 5, 5), win(0, 40, 40, 5, 5), win(0, 97, 50, 2, 2)], None),
    "the same tile of different images": ([win(0, 1, 1, 5, 5), win(1, 1, 1, 5, 5), win(2, 2, 2, 5, 5)], None),
    "the third meets the first": ([win(0, 0, 0, 10, 10), win(1, 0, 0, 10, 10), win(0, 31, 31, 2, 2)], 2),
    "the whole image and a pixel": ([win(0, 0, 0, 100, 70), win(0, 99, 69, 1, 1)], 1),
}


@pytest.mark.parametrize("name", sorted(CHECKS))
def test_check_equals_the_model(product, name):
    windows, bad = CHECKS[name]
    sizes = [(100, 70)] * 3
    assert pm.first_overlap(windows, 32, 32) == bad  # the model, against the answer made by hand
    if bad is None:
        got = product.patch_check(sizes, windows, 32, 32)
        assert got.tolist() == pm.layout(windows, 32, 32) == product.window_layout(sizes, windows, 32, 32).tolist()
    else:
        with pytest.raises(product.PxzError) as e:
            product.patch_check(sizes, windows, 32, 32)
        assert e.value.code == INVALID_ARG and e.value.window == bad


def test_check_on_random_windows(product):
    rng = np.random.default_rng(11)
    sizes = [(45, 40), (97, 61), (200, 136)]
    seen = set()
    for bw, bh in ((48, 20), (16, 16), (32, 32)):
        for _ in range(60):
            windows = []
            for _ in range(int(rng.integers(1, 6))):
                i = int(rng.integers(0, 3))
                x, y = int(rng.integers(0, sizes[i][0])), int(rng.integers(0, sizes[i][1]))
                windows.append(win(i, x, y, int(rng.integers(1, min(40, sizes[i][0] - x) + 1)), int(rng.integers(1, min(30, sizes[i][1] - y) + 1))))
            bad = pm.first_overlap(windows, bw, bh)
            seen.add(bad is None)
            if bad is None:
                assert product.patch_check(sizes, windows, bw, bh).tolist() == pm.layout(windows, bw, bh)
            else:
                with pytest.raises(product.PxzError) as e:
                    product.patch_check(sizes, windows, bw, bh)
                assert e.value.code == INVALID_ARG and e.value.window == bad
    assert seen == {True, False}


def test_check_refuses_what_the_layout_refuses(product):
    L = product.load_library()
    descs = C.cast(product.image_descs([(100, 70, 0, 0)]), C.c_void_p)
    one = C.cast(product.window_descs([win(0, 0, 0, 10, 10)]), C.c_void_p)
    out = np.zeros(4, np.uint64)
    po, bad = C.c_void_p(out.ctypes.data), C.c_uint32(7)
    assert L.pxz_patch_check(descs, 1, one, 1, 32, 32, po, C.byref(bad)) == 0 and bad.value == product.NO_WINDOW
    assert L.pxz_patch_check(descs, 1, one, 1, 32, 32, po, None) == 0  # (the out parameter is optional)
    for args in ((None, 1, one, 1, 32, 32, po), (descs, 1, None, 1, 32, 32, po), (descs, 1, one, 1, 32, 32, None), (descs, 1, one, 0, 32, 32, po),
                 (descs, 0, one, 1, 32, 32, po), (descs, 1, one, 1, 0, 32, po), (descs, 1, one, 1, 32, 0, po)):
        bad.value = 7
        assert L.pxz_patch_check(*args, C.byref(bad)) == INVALID_ARG and bad.value == product.NO_WINDOW, args
    refused = {
        "image index out of range": win(1, 0, 0, 10, 10),
        "empty width": win(0, 5, 5, 0, 10),
        "empty height": win(0, 5, 5, 10, 0),
        "leaves the image on the right": win(0, 91, 0, 10, 10),
        "leaves the image below": win(0, 0, 61, 10, 10),
        "starts outside": win(0, 100, 0, 1, 1),
        "x + width wraps 32 bits": win(0, 0xfffffff0, 0, 0x20, 1),
    }
    for what, w in refused.items():
        for check in (product.patch_check, product.window_layout):
            with pytest.raises(product.PxzError) as e:
                check([(100, 70)], [win(0, 0, 0, 1, 1), w], 32, 32)
            assert e.value.code == INVALID_ARG, what
    for what, geom, code in (("zero side", (0, 70, 0, 0), INVALID_ARG), ("reserved field", (100, 70, 0, 0, 1), INVALID_ARG),
                             ("side above 2^24", ((1 << 24) + 1, 70, 0, 0), UNSUPPORTED)):
        d = C.cast(product.image_descs([geom]), C.c_void_p)
        assert L.pxz_patch_check(d, 1, C.cast(product.window_descs([win(0, 0, 0, 1, 1)]), C.c_void_p), 1, 32, 32, po, None) == code, what
    side = 1 << 24  # more than 2^32-1 covered tiles: the layout's answer comes before the look at what the windows share
    w = win(0, 0, 0, side, 255)
    assert product.patch_check([(side, 255)], [w], 1, 1).tolist() == [0, 255 * side]
    with pytest.raises(product.PxzError) as e:
        product.patch_check([(side, 255)], [w, w], 1, 1)
    assert e.value.code == UNSUPPORTED and e.value.window == product.NO_WINDOW


# ---- the model's footing ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(pm.FIXTURES))
def test_writer_is_canonical_over_the_reader(oracle, name):
    f = pm.fixture(oracle, name)
    d = pm.decoded(oracle, f.raw, f.c)
    again = oracle.encode_container(f.w, f.h, f.bw, f.bh, f.c, d["filter"], d["values"], None, d["tw"], d["th"], d["slots"])
    assert again == f.raw


@pytest.mark.parametrize("name", sorted(pm.FIXTURES))
def test_hull_tiles_are_the_whole_images_tiles(oracle, name):
    """a tile's shrink result depends only on its own pixels: value bits, sizes and slot bytes"""
    f = pm.fixture(oracle, name)
    d = pm.decoded(oracle, f.raw, f.c)
    for case, rects in f.windows().items():
        patches = [(r, pm.new_pixels(r, f.c, 1)) for r in rects]
        img = pm.patched_image(oracle, d, f.c, f.p.expand_filter, patches)
        wv, ww, wh, ws = oracle.shrink_image(img, f.bw, f.bh, f.p.mode, f.p.filt, f.p.factor)
        for r in rects:
            hv, hw, hh, hs = pm.hull_tiles(oracle, img, r, f.bw, f.bh, f.p)
            tiles = pm.covered_tiles(r, f.size, f.bw, f.bh)
            assert len(tiles) == len(hv), case
            for q, t in enumerate(tiles):
                n = int(hw[q]) * int(hh[q]) * f.c
                assert hv[q:q + 1].view(np.uint32)[0] == wv[t:t + 1].view(np.uint32)[0], (case, t)
                assert (hw[q], hh[q]) == (ww[t], wh[t]) and (hs[q, :n] == ws[t, :n]).all(), (case, t)


@pytest.mark.parametrize("name", sorted(pm.FIXTURES))
def test_a_whole_image_window_is_the_plain_encode(oracle, name):
    f = pm.fixture(oracle, name)
    rect = f.windows()["whole"][0]
    px = pm.new_pixels(rect, f.c, 2)
    new, _ = pm.patched_file(oracle, f.raw, f.c, f.p, [(rect, px)])
    v, tw, th, slots = oracle.shrink_image(px, f.bw, f.bh, f.p.mode, f.p.filt, f.p.factor)
    assert new == oracle.encode_container(f.w, f.h, f.bw, f.bh, f.c, 0, v, None, tw, th, slots)


@pytest.mark.parametrize("name", sorted(pm.FIXTURES))
def test_fixtures_cover_tiles_stored_whole_and_tiles_stored_small(oracle, name):
    """both paths of the tile image -- the clone-in and the expand -- under the windows: among the covered tiles of the windows that
    are not the whole image, under the 2x2 corner alone, and among the tiles the one-tile windows patch.  (Noise at factors of
    0.3-0.5 came out small on every 32x32 tile: the fixtures alternate noise with ramps, and their factors were picked per mode.
    The 2 px wide edge tiles of the 130x130 fixtures have no interior for the directional detector and are stored as 1x1.)"""
    f = pm.fixture(oracle, name)
    single, partial = set(), set()
    for case, rects in f.windows().items():
        tiles = [t for r in rects for t in pm.covered_tiles(r, f.size, f.bw, f.bh)]
        kinds = {f.stored_full(t) for t in tiles}
        print(name, case, "covered", len(tiles), "stored whole", sum(f.stored_full(t) for t in tiles))
        if case == "corner":
            assert kinds == {True, False}, [(int(f.tw[t]), int(f.th[t])) for t in tiles]
        if len(tiles) == 1:
            single |= kinds
        if case != "whole":
            partial |= kinds
    assert single == {True, False} and partial == {True, False}
