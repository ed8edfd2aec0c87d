"""Distortion of re-shrunk tiles against the archive's own (pxz_reshrink_distortion_varied_device and the two host forms over it),
the part that needs no GPU: the symbols, and the size query -- the footprint of a one-wave block from the layout function the
launch uses, held against a count made here by hand (three planes of a dword per pixel, the windows of both axes at the wider
of the two filters' strides, the images' first tiles), at the limit it reports and one step on either side of it."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pixlzr_hip.h")
LDS_PER_CU = 160 * 1024
FIRST_TILES = 8192  # the first tiles of at most 2048 images, kept in LDS beside the waves' images
BLOCKS = [(16, 16), (32, 32), (64, 64), (37, 61)]
NAMES = ["pxz_reshrink_distortion_varied_device", "pxz_reshrink_distortion_lds_bytes", "pxz_rate_distortion_varied_files",
         "pxz_transcode_varied_files_fit"]
INVALID_ARG = -1
# the largest square block the header states, and the filter pair (Nearest on both sides: the narrowest windows) that goes one further
LIMIT, LIMIT_NEAREST = 112, 113


_widest = {}


def widest_window(product, side, filt):
    """taps of the widest window among the up-scaling tables stored size -> side (Nearest picks one sample)"""
    if filt == 0 or side == 1:
        return 1
    if (side, filt) not in _widest:
        _widest[(side, filt)] = max(product.axis_table(s, side, filt)[2].shape[1] for s in range(1, side))
    return _widest[(side, filt)]


def by_hand(product, bw, bh, expand_filter, filter_up):
    """the footprint counted here: first tiles + 4 * (3 planes + (bw + bh) windows of 1 + ceil(taps / 2) dwords), in whole 16 bytes"""
    taps = max(widest_window(product, side, f) for side in {bw, bh} for f in (expand_filter, filter_up))
    wdw = 1 + (taps + 1) // 2
    return FIRST_TILES + 4 * ((3 * bw * bh + wdw * (bw + bh) + 3) & ~3)


def test_symbols_are_exported_and_declared(product):
    """fails before the feature exists"""
    lib = product.load_library()
    text = open(HEADER).read()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert f"int {name}(" in text, name
        assert name in product.EXPORTED_SYMBOLS, name
    out = subprocess.run(["nm", "-D", "--defined-only", product.library_path()], capture_output=True, text=True, check=True).stdout
    for name in NAMES:
        assert f" T {name}" in out, name
    for method in ("reshrink_distortion_varied_device", "rate_distortion_varied_files", "transcode_varied_files_fit"):
        assert hasattr(product.Handle, method), method
    assert hasattr(product, "reshrink_distortion_lds_bytes")
    assert len(set(product.EXPORTED_SYMBOLS)) == len(product.EXPORTED_SYMBOLS)


@pytest.mark.parametrize("c", [3, 4])
@pytest.mark.parametrize("block", BLOCKS, ids=lambda b: f"{b[0]}x{b[1]}")
def test_footprint_equals_the_count_by_hand(product, block, c):
    """every pair of filters; the planes hold a dword per pixel, so the channel count does not enter"""
    bw, bh = block
    for xf in range(5):
        for uf in range(5):
            got = product.reshrink_distortion_lds_bytes(bw, bh, c, xf, uf)
            assert got == by_hand(product, bw, bh, xf, uf), (block, c, xf, uf, got)
            assert got <= LDS_PER_CU and got % 16 == 0
            assert got == product.reshrink_distortion_lds_bytes(bw, bh, c, uf, xf)  # the wider of the two strides, whichever side has it
    # three planes against the re-shrink's two: above it by a plane, less what the detector's tables take there
    assert product.reshrink_distortion_lds_bytes(bw, bh, c, 4, 4) > 3 * 4 * bw * bh
    if block == (64, 64):
        assert product.reshrink_distortion_lds_bytes(64, 64, c, 4, 4) <= (LDS_PER_CU - FIRST_TILES) // 3 + FIRST_TILES  # three waves to a block


@pytest.mark.parametrize("c", [3, 4])
def test_one_step_on_either_side_of_the_limit(product, c):
    for xf in range(5):
        for uf in range(5):
            n = LIMIT_NEAREST if (xf, uf) == (0, 0) else LIMIT
            at = product.reshrink_distortion_lds_bytes(n, n, c, xf, uf)
            assert at <= LDS_PER_CU and at == by_hand(product, n, n, xf, uf), (xf, uf, at)
            for (w, h) in [(n + 1, n + 1), (n + 2, n), (n, n + 2)]:
                assert product.reshrink_distortion_lds_bytes(w, h, c, xf, uf) > LDS_PER_CU, (xf, uf, w, h)
    # the re-shrink's own limit is not this call's; nor is anything near the range of the arguments
    for (w, h) in [(128, 128), (256, 64), (1, 16385), (65536, 65536), (2 ** 32 - 1, 2 ** 32 - 1)]:
        assert product.reshrink_distortion_lds_bytes(w, h, c, 4, 4) > LDS_PER_CU, (w, h)
    # non-square blocks fit as well (their windows take more: bw + bh of them), and small ones by far
    for (w, h) in [(200, 56), (56, 200), (1, 1), (5, 3), (3, 5)]:
        assert product.reshrink_distortion_lds_bytes(w, h, c, 4, 4) <= LDS_PER_CU, (w, h)
    assert f"{LIMIT}x{LIMIT}" in open(HEADER).read(), "the header does not state the limit the function gives"


def test_bad_arguments_leave_the_output_as_it_was(product):
    L = product.load_library()
    for args in [(0, 16, 4, 0, 0), (16, 0, 4, 0, 0), (16, 16, 2, 0, 0), (16, 16, 5, 0, 0), (16, 16, 0, 0, 0), (16, 16, 4, 5, 0), (16, 16, 4, 0, 5),
                 (16, 16, 4, 2 ** 32 - 1, 0), (0, 0, 0, 9, 9)]:
        out = C.c_uint32(0xDEADBEEF)
        with pytest.raises(product.PxzError) as e:
            product.reshrink_distortion_lds_bytes(*args, out=out)
        assert e.value.code == INVALID_ARG and out.value == 0xDEADBEEF, args
    assert L.pxz_reshrink_distortion_lds_bytes(16, 16, 4, 0, 0, None) == INVALID_ARG
    # the calls with a handle refuse a null one before they read anything else
    assert L.pxz_reshrink_distortion_varied_device(None, None, 0, 4, None, 0, 1, *([None] * 9)) == INVALID_ARG
    assert L.pxz_rate_distortion_varied_files(None, None, None, 0, None, 0, 0, None, 0, None, None) == INVALID_ARG
    assert L.pxz_transcode_varied_files_fit(None, None, None, 0, None, 0, 0, None, 0, 0, None, 0, None, 0, *([None] * 5)) == INVALID_ARG
