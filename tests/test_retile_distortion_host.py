"""Distortion of re-tiled tiles against the archive they came from (pxz_retile_distortion_varied_device, its size query and the
three host forms over it), the part that needs no GPU: the symbols, the LDS footprint of the kernel against a hand count of the
layout the header describes, its limit, and the argument errors of the size query."""
import ctypes as C
import os
import re
import subprocess

import pytest

from test_retile_ladder_host import window_dwords

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pixlzr_hip.h")
LDS_PER_CU = 160 * 1024
LANCZOS3 = 4
NAMES = ["pxz_retile_distortion_varied_device", "pxz_retile_distortion_lds_bytes", "pxz_rate_distortion_retile_files",
         "pxz_retile_varied_files_fit", "pxz_retile_varied_files_fit_tiles"]
BLOCKS = [(16, 16), (32, 32), (64, 64), (48, 20), (37, 61)]
PAIRS = [(s, d) for s in BLOCKS for d in BLOCKS]  # every pair, both directions, equal blocks included


# ---- 1. symbols -----------------------------------------------------------------------------------------------------------

def test_symbols_are_exported_declared_and_bound(product):
    """fails before the archive fit at a new block size exists"""
    lib = product.load_library()
    text = open(HEADER).read()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert f"int {name}(" in text, name
        assert name in product.EXPORTED_SYMBOLS, name
    out = subprocess.run(["nm", "-D", "--defined-only", product.library_path()], capture_output=True, text=True, check=True).stdout
    for name in NAMES:
        assert f" T {name}" in out, name
    for method in ("retile_distortion_varied_device", "rate_distortion_retile_files", "retile_varied_files_fit", "retile_varied_files_fit_tiles"):
        assert hasattr(product.Handle, method), method
    assert hasattr(product, "retile_distortion_lds_bytes")
    assert len(set(product.EXPORTED_SYMBOLS)) == len(product.EXPORTED_SYMBOLS)


# ---- 2. footprint ---------------------------------------------------------------------------------------------------------

def up16(v):
    return (v + 15) & ~15


def staging(src, dst, wdw):
    """what retile_assemble stages for parts of a dst tile out of src tiles whose windows take wdw dwords: the stored pixels the
    part's windows read (pw x ph dwords), the horizontal pass's intermediate (cw x ph), the windows of both source axes"""
    (sw, sh), (dw, dh) = src, dst
    cw, ch = min(sw, dw), min(sh, dh)
    pw, ph = min(sw, cw + 2 * (wdw - 1) + 2), min(sh, ch + 2 * (wdw - 1) + 2)
    return up16(pw * ph * 4) + up16(cw * ph * 4) + (((sw + sh) * wdw + 3) & ~3) * 4


def restated_footprint(src, dst, wdw_src, wdw_set):
    """the layout of retile_distortion_lds, said again: [R: D] [E: D] [S = max(source side, set side)]"""
    d = up16(dst[0] * dst[1] * 4)
    if d > 65536 or src[0] * src[1] * 4 > 65536:
        return 0xffffffff
    return 2 * d + max(staging(src, dst, wdw_src), staging(dst, dst, wdw_set))


def expected_query(product, src, dst, xf, uf):
    want = restated_footprint(src, dst, 1, 1)  # (a pair beyond the CU with windows of one dword is reported as that)
    if want <= LDS_PER_CU:
        want = restated_footprint(src, dst, window_dwords(product, src, xf), window_dwords(product, dst, uf))
    return want


@pytest.mark.parametrize("xf", range(5))
@pytest.mark.parametrize("uf", range(5))
def test_lds_footprint_equals_the_restated_layout_and_the_promised_pairs_fit(product, xf, uf):
    for (src, dst) in PAIRS:
        for c in (3, 4):
            got = product.retile_distortion_lds_bytes(*src, *dst, c, xf, uf)
            assert got == expected_query(product, src, dst, xf, uf), (src, dst, c)
            assert got <= LDS_PER_CU, (src, dst, c, got)
    # pairs around and beyond the limit, tiny blocks, one-row blocks
    for (src, dst) in [((3, 5), (3, 5)), ((1, 1), (1, 1)), ((1, 7), (7, 1)), ((128, 128), (16, 16)), ((16, 16), (128, 128)), ((128, 128), (128, 127)),
                       ((256, 16), (16, 256)), ((61, 37), (48, 20)), ((99, 99), (99, 99)), ((100, 100), (100, 100)), ((101, 101), (101, 101))]:
        assert product.retile_distortion_lds_bytes(*src, *dst, 4, xf, uf) == expected_query(product, src, dst, xf, uf), (src, dst)
    # seven blocks per CU at 32x32 destination blocks and two at 64x64, whatever the source block up to 64x64
    for src in BLOCKS:
        assert product.retile_distortion_lds_bytes(*src, 32, 32, 4, xf, uf) <= LDS_PER_CU // 7, src
        assert product.retile_distortion_lds_bytes(*src, 64, 64, 4, xf, uf) <= LDS_PER_CU // 2, src


def test_a_hand_count():
    # 64x64 -> 32x32 with windows of 5 dwords on both sides (Lanczos3): D = 32*32*4 = 4096 twice; the source side stages
    # min(64, 32 + 8 + 2) = 42 x 42 dwords (7056), an intermediate of 32 x 42 (5376) and 128 windows of 5 dwords (2560): 14992; the
    # set side a whole 32x32 tile (4096), as large an intermediate (4096) and 64 windows (1280): 9472
    assert staging((64, 64), (32, 32), 5) == 7056 + 5376 + 2560
    assert staging((32, 32), (32, 32), 5) == 4096 + 4096 + 1280
    assert restated_footprint((64, 64), (32, 32), 5, 5) == 8192 + 14992
    # 32x32 -> 64x64: the set side decides: 16384 + 16384 + 2560
    assert restated_footprint((32, 32), (64, 64), 5, 5) == 32768 + 35328


def test_the_largest_equal_square_pair_is_the_one_the_header_states(product):
    n = 1
    while product.retile_distortion_lds_bytes(n + 1, n + 1, n + 1, n + 1, 4, LANCZOS3, LANCZOS3) <= LDS_PER_CU:
        n += 1
    assert product.retile_distortion_lds_bytes(n, n, n, n, 4, LANCZOS3, LANCZOS3) <= LDS_PER_CU
    assert product.retile_distortion_lds_bytes(n + 1, n + 1, n + 1, n + 1, 4, LANCZOS3, LANCZOS3) > LDS_PER_CU
    for m in range(n + 1, 129):  # nothing larger fits either
        assert product.retile_distortion_lds_bytes(m, m, m, m, 3, LANCZOS3, LANCZOS3) > LDS_PER_CU, m
    text = " ".join(open(HEADER).read().split())
    said = re.search(r"With Lanczos3 on both sides the largest admitted equal square pair is (\d+)x(\d+) <-> (\d+)x(\d+)", text)
    assert said, "the header does not state the largest equal square pair"
    assert {int(g) for g in said.groups()} == {n}, (said.group(0), n)
    assert n * n * 65025 < 2 ** 32  # what the u32 accumulation must hold


def test_a_plane_above_64_kb_on_either_side(product):
    for c in (3, 4):
        assert product.retile_distortion_lds_bytes(129, 128, 16, 16, c, 2, 3) == 0xffffffff
        assert product.retile_distortion_lds_bytes(16, 16, 129, 128, c, 2, 3) == 0xffffffff
        assert product.retile_distortion_lds_bytes(128, 128, 16, 16, c, 2, 3) != 0xffffffff


def test_lds_query_refuses_bad_arguments(product):
    for args in [(0, 16, 16, 16, 4, 0, 0), (16, 0, 16, 16, 4, 0, 0), (16, 16, 0, 16, 4, 0, 0), (16, 16, 16, 0, 4, 0, 0), (16, 16, 16, 16, 2, 0, 0),
                 (16, 16, 16, 16, 5, 0, 0), (16, 16, 16, 16, 4, 5, 0), (16, 16, 16, 16, 4, 0, 5)]:
        out = C.c_uint32(0x5A5A5A5A)
        with pytest.raises(product.PxzError) as e:
            product.retile_distortion_lds_bytes(*args, out=out)
        assert e.value.code == -1 and out.value == 0x5A5A5A5A, args
    assert product.load_library().pxz_retile_distortion_lds_bytes(16, 16, 16, 16, 4, 0, 0, None) == -1


def test_device_and_host_forms_refuse_a_null_handle(product):
    L = product.load_library()
    assert L.pxz_retile_distortion_varied_device(None, None, 0, 4, 16, 16, None, 0, 1, *([None] * 9)) == -1
    assert L.pxz_rate_distortion_retile_files(None, None, None, 0, None, 0, 0, None, 0, None, None) == -1
    assert L.pxz_retile_varied_files_fit(None, None, None, 0, None, 0, 0, None, 0, 0, None, 0, None, 0, *([None] * 5)) == -1
    assert L.pxz_retile_varied_files_fit_tiles(None, None, None, 0, None, 0, 0, None, 0, 0, None, 0, None, 0, None, 0, *([None] * 6)) == -1
