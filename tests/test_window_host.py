"""Pixel windows of files without a GPU: pxz_window_layout against the formula of the header -- window k covers tile columns
x/bw .. (x+width-1)/bw and tile rows y/bh .. (y+height-1)/bh of its image, its covered tiles are numbered from the sum of the
covered tiles of the windows before it -- its error codes, and the four exported names.  (The header parsing of
pxz_decode_windows_files is reachable only with a handle: tests/test_gpu_windows.py.)"""
import ctypes as C

import numpy as np
import pytest

INVALID_ARG, UNSUPPORTED = -1, -5
NAMES = ("pxz_window_layout", "pxz_decode_windows_device", "pxz_expand_windows_device", "pxz_decode_windows_files")


def covered(window, bw, bh):
    """the formula, in Python: (first column, first row, columns, rows) of the tile grid a window covers"""
    _, x, y, w, h = window[:5]
    c0, r0 = x // bw, y // bh
    return c0, r0, (x + w - 1) // bw - c0 + 1, (y + h - 1) // bh - r0 + 1


def expected_offsets(windows, bw, bh):
    offs = [0]
    for w in windows:
        _, _, cc, cr = covered(w, bw, bh)
        offs.append(offs[-1] + cc * cr)
    return offs


def win(image, x, y, w, h):
    return (image, x, y, w, h, 0, 0)


def test_library_exports_the_window_calls(product):
    L = product.load_library()
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in product.EXPORTED_SYMBOLS, name
    for name in ("decode_windows_device", "expand_windows_device", "decode_windows_files"):
        assert callable(getattr(product.Handle, name)), name
    assert C.sizeof(product.Window) == 32  # six dwords and the 64-bit offset


# 100x70 in 32x32 blocks: a 4x3 grid whose edge tiles are 4 px wide and 6 px high
CASES = {
    "one tile": ([win(0, 33, 34, 20, 10)], [1]),
    "a tile exactly": ([win(0, 32, 32, 32, 32)], [1]),
    "straddles four tiles": ([win(0, 31, 31, 2, 2)], [4]),
    "touches the edge tile": ([win(0, 90, 60, 10, 10)], [4]),
    "inside the edge tile": ([win(0, 97, 65, 2, 3)], [1]),
    "the image": ([win(0, 0, 0, 100, 70)], [12]),
    "one pixel row": ([win(0, 0, 63, 100, 1)], [4]),
    "one pixel column": ([win(0, 64, 0, 1, 70)], [3]),
    "two windows of one image": ([win(0, 0, 0, 33, 33), win(0, 20, 20, 50, 20)], [4, 6]),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_layout_equals_the_formula(product, name):
    windows, counts = CASES[name]
    want = expected_offsets(windows, 32, 32)
    assert [b - a for a, b in zip(want, want[1:])] == counts  # the formula itself, against counts made by hand
    got = product.window_layout([(100, 70)], windows, 32, 32)
    assert got.dtype == np.uint64 and got.tolist() == want


def test_layout_over_several_images_and_odd_blocks(product):
    """windows of three differently sized images in any order, blocks that are not square; random rectangles"""
    rng = np.random.default_rng(7)
    sizes = [(1, 1), (45, 40), (97, 61)]
    for bw, bh in ((48, 20), (16, 16), (7, 64)):
        windows = []
        for _ in range(40):
            i = int(rng.integers(0, 3))
            x, y = int(rng.integers(0, sizes[i][0])), int(rng.integers(0, sizes[i][1]))
            windows.append(win(i, x, y, int(rng.integers(1, sizes[i][0] - x + 1)), int(rng.integers(1, sizes[i][1] - y + 1))))
        assert product.window_layout(sizes, windows, bw, bh).tolist() == expected_offsets(windows, bw, bh)


def raw_layout(product, descs, n_images, windows, n_windows, bw, bh, out):
    return product.load_library().pxz_window_layout(descs, n_images, windows, n_windows, bw, bh, out)


def test_layout_error_codes(product):
    descs = C.cast(product.image_descs([(100, 70, 0, 0)]), C.c_void_p)
    one = C.cast(product.window_descs([win(0, 0, 0, 10, 10)]), C.c_void_p)
    out = np.zeros(4, np.uint64)
    po = C.c_void_p(out.ctypes.data)
    assert raw_layout(product, descs, 1, one, 1, 32, 32, po) == 0
    assert raw_layout(product, None, 1, one, 1, 32, 32, po) == INVALID_ARG
    assert raw_layout(product, descs, 1, None, 1, 32, 32, po) == INVALID_ARG
    assert raw_layout(product, descs, 1, one, 1, 32, 32, None) == INVALID_ARG
    assert raw_layout(product, descs, 1, one, 0, 32, 32, po) == INVALID_ARG
    assert raw_layout(product, descs, 0, one, 1, 32, 32, po) == INVALID_ARG
    assert raw_layout(product, descs, 1, one, 1, 0, 32, po) == INVALID_ARG
    bad = {
        "image index out of range": win(1, 0, 0, 10, 10),
        "empty width": win(0, 5, 5, 0, 10),
        "empty height": win(0, 5, 5, 10, 0),
        "leaves the image on the right": win(0, 91, 0, 10, 10),
        "leaves the image below": win(0, 0, 61, 10, 10),
        "starts outside": win(0, 100, 0, 1, 1),
        "x + width wraps 32 bits": win(0, 0xfffffff0, 0, 0x20, 1),
    }
    for what, w in bad.items():
        with pytest.raises(product.PxzError) as e:
            product.window_layout([(100, 70)], [win(0, 0, 0, 1, 1), w], 32, 32)
        assert e.value.code == INVALID_ARG, what
    # what pxz_varied_layout refuses for the descriptors
    for what, geom, code in (("zero side", (0, 70, 0, 0), INVALID_ARG), ("reserved field", (100, 70, 0, 0, 1), INVALID_ARG),
                             ("side above 2^24", ((1 << 24) + 1, 70, 0, 0), UNSUPPORTED)):
        d = C.cast(product.image_descs([geom]), C.c_void_p)
        assert raw_layout(product, d, 1, C.cast(product.window_descs([win(0, 0, 0, 1, 1)]), C.c_void_p), 1, 32, 32, po) == code, what


def test_more_than_2_32_covered_tiles_are_unsupported(product):
    """one image of 2^24 x 256 px in 1x1 blocks has exactly 2^32 tiles, which pxz_varied_layout refuses; 2^24 x 255 passes it, and
    two whole-image windows of that one then cover 2 * 255 * 2^24 > 2^32 - 1 tiles"""
    side = 1 << 24
    w = win(0, 0, 0, side, 255)
    assert product.window_layout([(side, 255)], [w], 1, 1).tolist() == [0, 255 * side]
    with pytest.raises(product.PxzError) as e:
        product.window_layout([(side, 255)], [w, w], 1, 1)
    assert e.value.code == UNSUPPORTED
