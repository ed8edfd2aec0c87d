"""Decode at reduced scale, without a GPU: the model against the oracle at scale 0, the host-only entry points (pxz_scaled_size,
pxz_scaled_axis_table, pxz_expand_scaled_lds_bytes), the exported symbols, and the coverage of the stored sizes that
tests/test_gpu_scaled_decode.py deals.  Every comparison is exact."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import scaled_model as sm

INVALID_ARG, UNSUPPORTED = -1, -5
NAMES = ("pxz_scaled_size", "pxz_scaled_axis_table", "pxz_expand_scaled_lds_bytes", "pxz_expand_varied_scaled_frames_device",
         "pxz_expand_windows_scaled_device", "pxz_decode_varied_files_scaled", "pxz_decode_windows_files_scaled")
CONVOLUTIONS = (1, 2, 3, 4)


def test_library_exports_declares_and_binds_the_scaled_calls(product):
    lib = product.load_library()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "pixlzr_hip.h")).read()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in product.EXPORTED_SYMBOLS, name
        assert re.search(r"\bint " + name + r"\(", header), name
        assert getattr(lib, name).argtypes is not None, name
    for method in ("expand_varied_scaled_frames_device", "expand_windows_scaled_device", "decode_varied_files_scaled",
                   "decode_windows_files_scaled"):
        assert hasattr(product.Handle, method), method


# ---- the model ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", (3, 4))
@pytest.mark.parametrize("geom", sm.GEOMS, ids=lambda g: f"{g[0]}x{g[1]}-{g[2]}x{g[3]}")
def test_model_at_scale_0_is_the_oracles_expand(oracle, geom, c):
    bw, bh, w, h, _ = geom
    f = sm.files_of(oracle, bw, bh, w, h, c, 0)[0]
    d = oracle.decode_container(f.raw)
    for filt in range(5):
        exp = oracle.expand_image(w, h, bw, bh, c, filt, d["tw"], d["th"], d["slots"])
        assert (f.image(filt, 0) == exp).all(), filt


# ---- pxz_scaled_size and the s | block rule -------------------------------------------------------------------------------

def test_scaled_size_is_the_sum_of_a_rows_tile_targets(product):
    for bw, bh, w, h, scales in sm.GEOMS:
        for k in scales:
            sw, sh = product.scaled_size(w, h, bw, bh, k)
            assert (sw, sh) == (sm.ceil_div(w, 1 << k), sm.ceil_div(h, 1 << k))
            rects = sm.tile_rects(w, h, bw, bh)
            cols = sm.ceil_div(w, bw)
            assert sw == sum(sm.target_of(r[2], r[3], k)[0] for r in rects[:cols])
            assert sh == sum(sm.target_of(r[2], r[3], k)[1] for r in rects[::cols])
            # ... and every tile's origin is exact
            assert all(r[0] % (1 << k) == 0 and r[1] % (1 << k) == 0 for r in rects)


def raw_size(product, *args):
    w, h = C.c_uint32(7), C.c_uint32(7)
    return product.load_library().pxz_scaled_size(*args, C.byref(w), C.byref(h)), w.value, h.value


def test_scaled_size_error_codes(product):
    L = product.load_library()
    assert raw_size(product, 100, 37, 48, 20, 2) == (0, 25, 10)
    assert raw_size(product, 100, 37, 48, 20, 3)[0] == INVALID_ARG   # 8 does not divide 20
    assert raw_size(product, 100, 70, 32, 32, 6)[0] == INVALID_ARG   # 64 does not divide 32
    assert raw_size(product, 100, 70, 32, 48, 5)[0] == INVALID_ARG   # ... nor 48
    assert raw_size(product, 100, 70, 32, 32, 32)[0] == INVALID_ARG
    assert raw_size(product, 0, 70, 32, 32, 0)[0] == INVALID_ARG
    assert raw_size(product, 100, 70, 0, 32, 0)[0] == INVALID_ARG
    assert raw_size(product, (1 << 24) + 1, 70, 32, 32, 0)[0] == UNSUPPORTED
    assert raw_size(product, 1 << 24, 1, 32, 32, 5) == (0, 1 << 19, 1)
    w = C.c_uint32()
    assert L.pxz_scaled_size(100, 70, 32, 32, 0, None, C.byref(w)) == INVALID_ARG
    assert L.pxz_scaled_size(100, 70, 32, 32, 0, C.byref(w), None) == INVALID_ARG


def test_window_alignment_rule_is_what_makes_a_window_a_crop(product):
    """x, y multiples of s and x + w a multiple of s or the image's width: then the scaled rectangle of the window is made of whole
    scaled pixels, and scaled_window_size is the size of that crop of the scaled image"""
    w, h = 100, 70
    for k in range(4):
        s = 1 << k
        for rect in ((0, 0, w, h), (s, 2 * s, 3 * s, s), (w - w % s - s if w % s else w - s, 0, w - (w - w % s - s if w % s else w - s), s)):
            x0, y0, x1, y1 = sm.scaled_rect(rect, k)
            assert product.scaled_window_size((0,) + rect, k) == (x1 - x0, y1 - y0)
            assert x1 <= sm.ceil_div(w, s) and y1 <= sm.ceil_div(h, s)
            assert rect[0] % s == 0 and ((rect[0] + rect[2]) % s == 0 or rect[0] + rect[2] == w)


# ---- pxz_scaled_axis_table ------------------------------------------------------------------------------------------------

PAIRS = [(8, 32), (32, 8), (64, 32), (64, 8), (64, 1), (33, 16), (17, 9), (5, 3), (20, 24), (48, 10), (2, 1), (1, 1), (7, 7), (13, 64), (64, 13)]


def test_axis_table_equals_fir_where_fir_defines_the_same_table(product, oracle):
    """the oracle's table of an axis is built with the flag `out > in`: the same table wherever the axis itself grows, or nothing
    grows"""
    for filt in CONVOLUTIONS:
        for i, o in PAIRS:
            es, en, ek, ep = oracle.fir_coeffs(i, o, filt)
            for grows in ((False, True) if o > i else (False,)):
                s, n, k, p = product.scaled_axis_table(i, o, filt, grows)
                assert p == ep and (s == es).all() and (n == en).all() and k.shape == ek.shape and (k == ek).all(), (filt, i, o, grows)
            # without the flag it is pxz_axis_table
            a = product.axis_table(i, o, filt)
            b = product.scaled_axis_table(i, o, filt, False)
            assert all((np.asarray(x) == np.asarray(y)).all() for x, y in zip(a, b)), (filt, i, o)
    # Nearest: the f64 index formula
    for i, o in PAIRS:
        s, n, k, p = product.scaled_axis_table(i, o, 0)
        assert (s == np.minimum((i / o * 0.5 + i / o * np.arange(o)).astype(np.int64), i - 1)).all() and (n == 1).all()


def test_only_triangle_depends_on_the_other_axis(product):
    for filt in CONVOLUTIONS:
        for i, o in ((64, 8), (8, 7), (33, 16)):
            a = product.scaled_axis_table(i, o, filt, False)
            b = product.scaled_axis_table(i, o, filt, True)
            same = a[3] == b[3] and all(x.shape == y.shape and (x == y).all() for x, y in zip(a[:3], b[:3]))
            assert same == (filt != 1), (filt, i, o)


def fir_premultiply(px):
    """fir's mul_div_255 on the colours of RGBA pixels"""
    out = px.copy()
    al = px[..., 3:4].astype(np.uint32)
    t = px[..., :3].astype(np.uint32) * al + 128
    out[..., :3] = ((t + (t >> 8)) >> 8).astype(np.uint8)
    return out


def fir_unpremultiply(px):
    """fir's reciprocal-table division"""
    out = px.copy()
    al = px[..., 3].astype(np.uint32)
    recip = np.where(al == 0, 0, ((255 * 512) // np.maximum(al, 1) + 1) >> 1)
    v = (px[..., :3].astype(np.uint32) * recip[..., None] + 128) >> 8
    out[..., :3] = np.minimum(v, 255).astype(np.uint8)
    return out


def pass_along(img, table, axis):
    """one convolution pass of fir over axis 0 (rows) or 1 (columns) of a [h, w, c] uint8 image with an exported table"""
    starts, sizes, k, prec = table
    src = np.moveaxis(img, axis, 0).astype(np.int64)
    out = np.empty((len(starts),) + src.shape[1:], np.uint8)
    for o in range(len(starts)):
        a, n = int(starts[o]), int(sizes[o])
        acc = (1 << (prec - 1)) + np.tensordot(k[o, :n].astype(np.int64), src[a:a + n], axes=(0, 0))
        out[o] = np.clip(acc >> prec, 0, 255).astype(np.uint8)
    return np.moveaxis(out, 0, axis)


def two_pass(product, tile, nw, nh, filt):
    """PixlzrBlock::resize restated over the exported tables: one flag for both axes, horizontal first, u8 between the passes"""
    th, tw, c = tile.shape
    grows = nw > tw or nh > th
    cur = fir_premultiply(tile) if c == 4 else tile
    if nw != tw:
        cur = pass_along(cur, product.scaled_axis_table(tw, nw, filt, grows), 1)
    if nh != th:
        cur = pass_along(cur, product.scaled_axis_table(th, nh, filt, grows), 0)
    return fir_unpremultiply(cur) if c == 4 else cur


MIXED = [((64, 8), (32, 32)), ((8, 64), (32, 32)), ((20, 48), (24, 10)), ((5, 17), (9, 3))]


@pytest.mark.parametrize("c", (3, 4))
@pytest.mark.parametrize("filt", CONVOLUTIONS)
def test_mixed_pairs_over_the_exported_tables_equal_the_oracle(product, oracle, filt, c):
    """an axis that shrinks while the other grows: the only place where the Triangle variant is pinned without a GPU"""
    rng = np.random.default_rng(50 + 10 * filt + c)
    for (tw, th), (nw, nh) in MIXED + [((64, 64), (8, 8)), ((64, 64), (1, 1)), ((33, 64), (16, 32)), ((8, 8), (32, 32))]:
        tiles = [rng.integers(0, 256, (th, tw, c), dtype=np.uint8)]
        sat = np.where(rng.integers(0, 2, (th, tw, c)) == 1, 255, 0).astype(np.uint8)  # saturated: 0 / 255 in every channel
        tiles.append(sat)
        checker = np.zeros((th, tw, c), np.uint8)
        checker[(np.add.outer(np.arange(th), np.arange(tw)) & 1) == 1] = 255
        if c == 4:
            checker[..., 3] = 255
        tiles.append(checker)
        for t in tiles:
            exp = oracle.resize(t, nw, nh, filt)
            got = two_pass(product, t, nw, nh, filt)
            assert (got == exp).all(), f"filter {filt} C{c} {tw}x{th} -> {nw}x{nh}: {int((got != exp).sum())} bytes differ"


# ---- pxz_expand_scaled_lds_bytes ------------------------------------------------------------------------------------------

def test_lds_bytes_grow_with_the_block_and_refuse_beyond_160_kb(product):
    last = 0
    for side in (16, 32, 64, 96, 128):
        b = product.expand_scaled_lds_bytes(side, side, 4, 4, 3)
        assert b > last and b >= 8 * side * side and b + 8192 <= 160 * 1024
        last = b
    # the windows are sized by the largest scale, not by the block times the widest window
    assert product.expand_scaled_lds_bytes(64, 64, 4, 4, 6) - 8 * 64 * 64 < 4 * (2 * 64 * (1 + 4) + 64 + 4) + 1
    assert product.expand_scaled_lds_bytes(64, 64, 4, 0, 6) < product.expand_scaled_lds_bytes(64, 64, 4, 4, 6)
    with pytest.raises(product.PxzError) as e:   # 144 x 144 RGB: two planes of 81 KB
        product.expand_scaled_lds_bytes(144, 144, 3, 4, 4)
    assert e.value.code == UNSUPPORTED and e.value.lds_bytes > 160 * 1024 - 8192
    with pytest.raises(product.PxzError) as e:   # RGBA tiles above 65536 bytes
        product.expand_scaled_lds_bytes(136, 136, 4, 4, 3)
    assert e.value.code == UNSUPPORTED
    with pytest.raises(product.PxzError) as e:
        product.expand_scaled_lds_bytes(48, 20, 4, 4, 3)
    assert e.value.code == INVALID_ARG
    with pytest.raises(product.PxzError) as e:
        product.expand_scaled_lds_bytes(32, 32, 5, 4, 0)
    assert e.value.code == INVALID_ARG


# ---- what the GPU module deals --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("geom", sm.GEOMS, ids=lambda g: f"{g[0]}x{g[1]}-{g[2]}x{g[3]}")
def test_dealt_stored_sizes_meet_every_class_that_can_occur(geom):
    """for every (geometry, scale) the GPU module runs -- the geometry itself and the block's second one (scaled_model.EXTRA)"""
    bw, bh, _, _, scales = geom
    everywhere = set()
    for (w, h) in (geom[2:4], sm.EXTRA[(bw, bh)]):
        for k in scales:
            rects = sm.tile_rects(w, h, bw, bh)
            met, can = set(), sm.feasible_classes(w, h, bw, bh, k)
            for tw, th in sm.deal_sizes(w, h, bw, bh, k):  # (the files the GPU module decodes at this scale)
                assert all(1 <= a <= r[2] and 1 <= b <= r[3] for r, a, b in zip(rects, tw, th))
                met |= sm.met_classes(w, h, bw, bh, k, tw, th)
            assert met == can, f"{bw}x{bh} {w}x{h} k={k}: not met: {sorted(can - met)}"
            everywhere |= met
            # what cannot occur at k = 0, and why: the target is the full place, which no stored size exceeds, and nothing is
            # narrower than s = 1 (a target of 1x1 needs a tile within s x s)
            if k == 0:
                assert not can & {"edge narrower than s", "both down", "one axis down", "mixed wider/lower", "mixed narrower/higher"}
            assert {"clone", "stored 1x1"} <= can
    assert everywhere == set(sm.CLASSES)
    # the block refuses the next scale
    assert bw % (2 << scales[-1]) or bh % (2 << scales[-1])
