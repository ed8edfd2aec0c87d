"""Decode at reduced scale (pxz_expand_varied_scaled_frames_device, pxz_expand_windows_scaled_device and their host forms).  The
files are built on the CPU: stored sizes dealt per (geometry, scale) so that every resize class that can occur there does
(tests/scaled_model.py; tests/test_scaled_host.py asserts it), random stored bytes, written by the oracle's writer and read by the
library's unchanged readers.  The expected pixels are the model's: oracle.resize of every stored tile to ceil(full / s), placed at
(x0 / s, y0 / s).  Every comparison is exact.  The outputs are pre-filled, and every byte that belongs to no image or window must
still hold the pattern afterwards."""
import numpy as np
import pytest

import scaled_model as sm
import stored_patterns as sp
from test_gpu_varied_decode import decode_varied, expand_varied, upload_files, poisoned

pytestmark = pytest.mark.gpu

POISON = sm.POISON
FILTERS = (0, 1, 2, 3, 4)
INVALID_ARG, UNSUPPORTED = -1, -5
GUARD = 64
IDS = [f"{g[0]}x{g[1]}-{g[2]}x{g[3]}" for g in sm.GEOMS]


@pytest.fixture(scope="module")
def gpu(product):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    h = product.Handle(0)
    yield h
    h.close()


# ---- batches, places and what to expect -----------------------------------------------------------------------------------

def batch_of(oracle, geom, c):
    """the files of one block: the geometry's and the second geometry's, dealt for every scale -> (files, their scales)"""
    bw, bh, w, h, scales = geom
    files = [f for (gw, gh) in ((w, h), sm.EXTRA[(bw, bh)]) for k in scales for f in sm.files_of(oracle, bw, bh, gw, gh, c, k)]
    return files, [f.k for f in files]


def place(shapes, c, flip=0):
    """outputs of (width, height) pixels each in one buffer, GUARD bytes before, between and behind them.  RGBA: every other one
    (flip picks which) on dwords with a pitch of a multiple of 4, the others at an odd address with an odd pitch; RGB: all at odd
    offsets with pitches that are no multiple of 4.  -> ([(pitch, offset)], bytes)"""
    out, at = [], GUARD
    for k, (w, h) in enumerate(shapes):
        if c == 4 and (k + flip) % 2 == 0:
            at = (at + 3) & ~3
            pitch = w * 4 + 8
        else:
            at |= 1
            pitch = w * c + 5
            while pitch % 4 == 0:
                pitch += 1
        out.append((pitch, at))
        at += pitch * h + GUARD
    return out, at


def view(buf, shape, where, c):
    (w, h), (pitch, off) = shape, where
    return np.lib.stride_tricks.as_strided(buf[off:], (h, w, c), (pitch, c, 1))


def outside(total, shapes, places, c):
    m = np.ones(total, bool)
    for (w, h), (pitch, off) in zip(shapes, places):
        for y in range(h):
            m[off + y * pitch: off + y * pitch + w * c] = False
    return m


def read_files(gpu, product, files):
    f0 = files[0]
    to, host, flags, status, dev = decode_varied(gpu, product, [f.raw for f in files], [(f.w, f.h) for f in files], f0.c, f0.bw, f0.bh)
    assert status == 0 and (flags == 0).all()
    return to, host, dev


def expand_scaled(gpu, files, scales, places, total, filt, dev):
    """-> (the pre-filled buffer after the call as a host array, per-image flags, status)"""
    import torch
    f0 = files[0]
    out = torch.full((total,), POISON, dtype=torch.uint8, device="cuda")
    flags = torch.full((len(files),), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    descs = [(f.w, f.h, p, o) for f, (p, o) in zip(files, places)]
    gpu.expand_varied_scaled_frames_device(descs, f0.c, f0.bw, f0.bh, filt, scales, dev[1], dev[2], dev[3], out, image_flags=flags)
    status = gpu.decode_status()
    torch.cuda.synchronize()
    return out.cpu().numpy(), flags.cpu().numpy(), status


def scaled_shapes(files, scales):
    return [(sm.ceil_div(f.w, 1 << k), sm.ceil_div(f.h, 1 << k)) for f, k in zip(files, scales)]


# ---- whole images ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", (3, 4), ids=("rgb", "alpha"))
@pytest.mark.parametrize("geom", sm.GEOMS, ids=IDS)
def test_batches_of_mixed_geometries_and_scales_equal_the_model(gpu, product, oracle, geom, c):
    files, scales = batch_of(oracle, geom, c)
    assert len({(f.w, f.h) for f in files}) == 2 and set(scales) == set(geom[4])
    to, host, dev = read_files(gpu, product, files)
    shapes = scaled_shapes(files, scales)
    for filt in FILTERS:
        places, total = place(shapes, c, flip=filt % 2)
        if c == 3:
            assert all(o % 2 == 1 and p % 4 != 0 for p, o in places)
        else:
            assert any(o % 4 == 0 and p % 4 == 0 for p, o in places) and any(o % 2 == 1 for p, o in places)
        buf, flags, status = expand_scaled(gpu, files, scales, places, total, filt, dev)
        assert status == 0 and (flags == 0).all(), f"filter {filt}: status {status}, flags {flags}"
        for i, f in enumerate(files):
            got, exp = view(buf, shapes[i], places[i], c), f.image(filt)
            bad = (got != exp).any(axis=2)
            assert not bad.any(), f"filter {filt} image {i} ({f.w}x{f.h} at 1/{1 << f.k}): {int(bad.sum())} of {bad.size} pixels differ from the model"
        assert (buf[outside(total, shapes, places, c)] == POISON).all(), f"filter {filt}: bytes outside the images were written"


@pytest.mark.parametrize("c", (3, 4), ids=("rgb", "alpha"))
@pytest.mark.parametrize("geom", sm.GEOMS, ids=IDS)
def test_scale_0_equals_the_unscaled_call(gpu, product, oracle, geom, c):
    files, _ = batch_of(oracle, geom, c)
    to, host, dev = read_files(gpu, product, files)
    shapes = [(f.w, f.h) for f in files]
    places, total = place(shapes, c)
    bw, bh = geom[:2]
    for filt in FILTERS:
        buf, flags, status = expand_scaled(gpu, files, [0] * len(files), places, total, filt, dev)
        descs = [(f.w, f.h, p, o) for f, (p, o) in zip(files, places)]
        ref, rflags, rstatus = expand_varied(gpu, descs, total, c, bw, bh, filt, dev)
        assert status == rstatus == 0 and (flags == rflags).all()
        assert (buf == ref).all(), f"filter {filt}: {int((buf != ref).sum())} bytes differ from pxz_expand_varied_frames_device"


def test_the_48x20_block_refuses_scale_3_and_names_the_image(gpu, product, oracle):
    import torch
    geom = sm.GEOMS[3]
    files, scales = batch_of(oracle, geom, 4)
    to, host, dev = read_files(gpu, product, files)
    shapes = [(f.w, f.h) for f in files]
    places, total = place(shapes, 4)
    out = torch.full((total,), POISON, dtype=torch.uint8, device="cuda")
    descs = [(f.w, f.h, p, o) for f, (p, o) in zip(files, places)]
    bad = [0] * len(files)
    bad[2] = 3
    with pytest.raises(product.PxzError) as e:
        gpu.expand_varied_scaled_frames_device(descs, 4, 48, 20, 4, bad, dev[1], dev[2], dev[3], out)
    assert e.value.code == INVALID_ARG and "image 2" in str(e.value)
    # a pitch below the scaled row, and only that: the full-resolution row's pitch is not asked for
    ok = [1] * len(files)
    small = list(descs)
    small[1] = (descs[1][0], descs[1][1], sm.ceil_div(descs[1][0], 2) * 4 - 1, descs[1][3])
    with pytest.raises(product.PxzError) as e:
        gpu.expand_varied_scaled_frames_device(small, 4, 48, 20, 4, ok, dev[1], dev[2], dev[3], out)
    assert e.value.code == INVALID_ARG and "image 1" in str(e.value)
    small[1] = (descs[1][0], descs[1][1], sm.ceil_div(descs[1][0], 2) * 4, descs[1][3])
    gpu.expand_varied_scaled_frames_device(small, 4, 48, 20, 4, ok, dev[1], dev[2], dev[3], out)
    torch.cuda.synchronize()


# ---- windows --------------------------------------------------------------------------------------------------------------

def rects_at(f, k):
    """aligned rectangles of one image at scale k: corners on multiples of s, or on the image's right and lower edge"""
    s = 1 << k
    bw, bh, w, h = f.bw, f.bh, f.w, f.h

    def rect(x0, y0, x1, y1):
        x1, y1 = min(x1, w), min(y1, h)
        return (x0, y0, x1 - x0, y1 - y0) if 0 <= x0 < x1 and 0 <= y0 < y1 else None

    lx, ly = (w - 1) // s * s, (h - 1) // s * s        # where the last scaled column and row begin
    rects = [rect(0, 0, w, h),                           # the whole image
             rect(bw - s, bh - s, bw + s, bh + s),       # across a four-tile corner (the tile seams, where they exist)
             rect(max(lx - s, 0), 0, w, 2 * s),          # to the ragged right edge
             rect(lx, ly, w, h),                         # one scaled pixel: the lower right corner
             rect(0, ly, s, h),                          # ... and the lower left one
             rect(bw + s, s, 2 * bw - s, bh - s),        # starts and ends inside one tile
             rect(s, bh - 2 * s, lx, bh + s)]            # starts and ends inside tiles, across every column seam
    return list(dict.fromkeys(r for r in rects if r is not None))


def windows_of(files, per_file_scales, c):
    """-> (windows with the places of their scaled crops, their scales, shapes, places, bytes)"""
    rects, scales = [], []
    for i, (f, ks) in enumerate(zip(files, per_file_scales)):
        for k in ks:
            for r in rects_at(f, k):
                rects.append((i,) + r)
                scales.append(k)
    shapes = [(x1 - x0, y1 - y0) for (x0, y0, x1, y1) in (sm.scaled_rect(r[1:], k) for r, k in zip(rects, scales))]
    places, total = place(shapes, c)
    windows = [r + (p, o) for r, (p, o) in zip(rects, places)]
    return windows, scales, shapes, places, total


def run_windows(gpu, product, files, windows, scales, total, filt):
    import torch
    f0 = files[0]
    sizes = [(f.w, f.h) for f in files]
    buf, offs = upload_files([f.raw for f in files], 3)
    to = product.window_layout(sizes, windows, f0.bw, f0.bh)
    tiles, rflags = poisoned(int(to[-1]), f0.bw * f0.bh * f0.c, len(windows))
    gpu.decode_windows_device(buf, offs, sizes, windows, f0.c, f0.bw, f0.bh, out=tiles, window_flags=rflags)
    assert gpu.decode_status() == 0
    out = torch.full((total,), POISON, dtype=torch.uint8, device="cuda")
    flags = torch.full((len(windows),), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    gpu.expand_windows_scaled_device(sizes, windows, f0.c, f0.bw, f0.bh, filt, scales, tiles[1], tiles[2], tiles[3], out, window_flags=flags)
    status = gpu.decode_status()
    torch.cuda.synchronize()
    return out.cpu().numpy(), flags.cpu().numpy(), status, tiles


@pytest.mark.parametrize("c", (3, 4), ids=("rgb", "alpha"))
@pytest.mark.parametrize("geom", sm.GEOMS, ids=IDS)
def test_windows_equal_the_crops_of_the_scaled_images(gpu, product, oracle, geom, c):
    bw, bh, w, h, all_scales = geom
    # two files; the first is read through windows at every scale of the geometry at once
    files = [sm.files_of(oracle, bw, bh, w, h, c, all_scales[1])[0], sm.files_of(oracle, bw, bh, *sm.EXTRA[(bw, bh)], c, all_scales[-1])[0]]
    windows, scales, shapes, places, total = windows_of(files, [all_scales, all_scales[:2]], c)
    assert len({k for win, k in zip(windows, scales) if win[0] == 0}) == len(all_scales) > 1
    for win, k in zip(windows, scales):
        s, f = 1 << k, files[win[0]]
        assert win[1] % s == 0 and win[2] % s == 0 and ((win[1] + win[3]) % s == 0 or win[1] + win[3] == f.w)
        assert (win[2] + win[4]) % s == 0 or win[2] + win[4] == f.h
    assert any((win[1] + win[3]) % (1 << k) for win, k in zip(windows, scales))  # the ragged edge
    for filt in FILTERS:
        buf, flags, status, _ = run_windows(gpu, product, files, windows, scales, total, filt)
        assert status == 0 and (flags == 0).all(), f"filter {filt}: status {status}, flags {flags}"
        for j, (win, k) in enumerate(zip(windows, scales)):
            x0, y0, x1, y1 = sm.scaled_rect(win[1:5], k)
            exp = files[win[0]].image(filt, k)[y0:y1, x0:x1]
            got = view(buf, shapes[j], places[j], c)
            bad = (got != exp).any(axis=2)
            assert not bad.any(), f"filter {filt} window {j} {win[:5]} at 1/{1 << k}: {int(bad.sum())} of {bad.size} pixels differ from the crop"
        assert (buf[outside(total, shapes, places, c)] == POISON).all(), f"filter {filt}: bytes outside the windows were written"


def test_windows_off_the_scales_grid_are_refused(gpu, product, oracle):
    import torch
    bw, bh, w, h, _ = sm.GEOMS[0]
    f = sm.files_of(oracle, bw, bh, w, h, 4, 1)[0]
    good = [(0, 4, 8, 16, 12), (0, 96, 64, 4, 6)]          # the second ends on the image's edge: 100 and 70
    windows, scales, shapes, places, total = [g + (64, 4096 * i) for i, g in enumerate(good)], [2, 2], None, None, 16384
    sizes = [(w, h)]
    to = product.window_layout(sizes, windows, bw, bh)
    T = int(to[-1])
    ow = torch.ones(T, dtype=torch.int32, device="cuda")
    slots = torch.zeros((T, bw * bh * 4), dtype=torch.uint8, device="cuda")
    out = torch.full((total,), POISON, dtype=torch.uint8, device="cuda")
    gpu.expand_windows_scaled_device(sizes, windows, 4, bw, bh, 4, scales, ow, ow, slots, out)
    torch.cuda.synchronize()
    out.fill_(POISON)
    for bad, scale in (((0, 2, 8, 16, 12), 2), ((0, 4, 6, 16, 12), 2), ((0, 4, 8, 15, 12), 2), ((0, 4, 8, 16, 13), 2), ((0, 4, 8, 16, 12), 3),
                       ((0, 0, 0, 32, 32), 6)):
        with pytest.raises(product.PxzError) as e:
            gpu.expand_windows_scaled_device(sizes, [windows[0], bad + (64, 4096)], 4, bw, bh, 4, [2, scale], ow, ow, slots, out)
        assert e.value.code == INVALID_ARG and "window 1" in str(e.value), bad
    with pytest.raises(product.PxzError) as e:   # the pitch is held against the scaled row: 4 pixels
        gpu.expand_windows_scaled_device(sizes, [(0, 4, 8, 16, 12, 15, 0)], 4, bw, bh, 4, [2], ow, ow, slots, out)
    assert e.value.code == INVALID_ARG and "window 0" in str(e.value)
    torch.cuda.synchronize()
    assert (out == POISON).all()


# ---- the ends of the value domain -----------------------------------------------------------------------------------------

PATTERNS = sp.OVERSHOOT + ("alpha 1..3", "alpha extremes", "alpha checker 254/255", "alpha checker 0/255", "white alpha 0", "white alpha 1")


def pattern_file(oracle, bw, bh):
    """the overshoot patterns, alpha 0..3, alpha 254/255 and the lone non-opaque pixels, drawn at their stored sizes"""
    pairs = [(bw, bh), (bw // 2, bh // 2), (bw // 4, bh), (bw, bh // 4), (bw - 1, bh // 2), (3, 8), (bw // 8, bh // 8), (1, 1)]
    items = []
    for tw, th in pairs:
        ones = sp.one_pixel_names(tw, th)
        lone = tuple(n for kind in sp.ONE_PIXEL_KINDS for n in [m for m in ones if m.startswith(kind)][:1] + [m for m in ones if m.startswith(kind)][-1:])
        items += [(n, tw, th) for n in dict.fromkeys(PATTERNS + lone) if n in sp.names(tw, th, 4)]
    w, h, tw, th, slots, names = sp.layout(items, bw, bh, 4)
    raw = oracle.encode_container(w, h, bw, bh, 4, 0, np.zeros(tw.size, np.float32), None, tw, th, slots)
    return raw, w, h, names


@pytest.mark.parametrize("block", (64, 32))
def test_pattern_tiles_at_scales_1_and_2(gpu, product, oracle, block):
    raw, w, h, names = pattern_file(oracle, block, block)
    assert any("one 254" in n for n in names) and any("lone opaque" in n for n in names) and any("alpha 1..3" in n for n in names)
    f = type("F", (), dict(raw=raw, w=w, h=h, c=4, bw=block, bh=block))
    files, scales = [f, f], [1, 2]
    to, host, dev = read_files(gpu, product, files)
    shapes = scaled_shapes(files, scales)
    places, total = place(shapes, 4)
    for filt in (4, 2):
        buf, flags, status = expand_scaled(gpu, files, scales, places, total, filt, dev)
        assert status == 0 and (flags == 0).all()
        for i, k in enumerate(scales):
            exp = sm.scaled_image(oracle, raw, 4, filt, k)
            got = view(buf, shapes[i], places[i], 4)
            bad = (got != exp).any(axis=2)
            if bad.any():
                ys, xs = np.nonzero(bad)
                t = (ys[0] << k) // block * sm.ceil_div(w, block) + (xs[0] << k) // block
                raise AssertionError(f"filter {filt} at 1/{1 << k}: {int(bad.sum())} pixels differ, first in tile {t} ({names[t]})")
        assert (buf[outside(total, shapes, places, 4)] == POISON).all()


# ---- flags ----------------------------------------------------------------------------------------------------------------

def test_impossible_stored_sizes_flag_their_owner_and_leave_its_pixels(gpu, product, oracle):
    import torch
    bw, bh, w, h, _ = sm.GEOMS[0]
    c, k, filt = 4, 2, 4
    f = sm.files_of(oracle, bw, bh, w, h, c, k)[0]
    files, scales = [f, f, f], [k, k, k]
    to, host, dev = read_files(gpu, product, files)
    T = int(to[1])
    cols = sm.ceil_div(w, bw)
    ow, oh = dev[1].clone(), dev[2].clone()
    # image 0: a stored width of zero; image 1: the 4-wide edge tile stored 5 wide (above its FULL place); image 2: a full tile
    # stored at its full size, far above its 8x8 target -- ordinary
    ow[1] = 0
    ow[T + cols - 1] = 5
    ow[2 * T], oh[2 * T] = bw, bh
    tw, th = host[1].copy(), host[2].copy()
    tw[1], tw[T + cols - 1] = 0, 5
    tw[2 * T], th[2 * T] = bw, bh
    assert bw > sm.target_of(bw, bh, k)[0] and sm.tile_rects(w, h, bw, bh)[cols - 1][2] == 4
    shapes = scaled_shapes(files, scales)
    places, total = place(shapes, c)
    buf, flags, status = expand_scaled(gpu, files, scales, places, total, filt, (dev[0], ow, oh, dev[3]))
    assert status == 1 and flags.tolist() == [1, 1, 0]
    for i in range(3):
        a, b = int(to[i]), int(to[i + 1])
        exp = sm.scaled_tiles_image(oracle, w, h, bw, bh, c, filt, k, tw[a:b], th[a:b], host[3][a:b], base=POISON)
        assert (view(buf, shapes[i], places[i], c) == exp).all(), i
    assert (view(buf, shapes[0], places[0], c)[:bh >> k, bw >> k:2 * bw >> k] == POISON).all()
    assert (buf[outside(total, shapes, places, c)] == POISON).all()

    # the same through windows: the windows that cover the tile are flagged, the one beside it is not
    windows, wscales, wshapes, wplaces, wtotal = windows_of([f], [[k]], c)
    sizes = [(w, h)]
    raw, offs = upload_files([f.raw], 3)
    wto = product.window_layout(sizes, windows, bw, bh)
    tiles, rflags = poisoned(int(wto[-1]), bw * bh * c, len(windows))
    gpu.decode_windows_device(raw, offs, sizes, windows, c, bw, bh, out=tiles, window_flags=rflags)
    wow = tiles[1].clone()
    covers = []
    for j, win in enumerate(windows):
        c0, r0 = win[1] // bw, win[2] // bh
        cc = (win[1] + win[3] - 1) // bw - c0 + 1
        hit = c0 <= 1 < c0 + cc and r0 == 0
        covers.append(int(hit))
        if hit:
            wow[int(wto[j]) + 1 - c0] = 0
    assert 0 < sum(covers) < len(covers)
    out = torch.full((wtotal,), POISON, dtype=torch.uint8, device="cuda")
    wflags = torch.full((len(windows),), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    gpu.expand_windows_scaled_device(sizes, windows, c, bw, bh, filt, wscales, wow, tiles[2], tiles[3], out, window_flags=wflags)
    assert gpu.decode_status() == 1
    torch.cuda.synchronize()
    assert wflags.cpu().numpy().tolist() == covers
    got = out.cpu().numpy()
    whole = sm.scaled_tiles_image(oracle, w, h, bw, bh, c, filt, k, tw[:T], th[:T], host[3][:T], base=POISON)  # (tile 1 missing)
    for j, win in enumerate(windows):
        x0, y0, x1, y1 = sm.scaled_rect(win[1:5], k)
        assert (view(got, wshapes[j], wplaces[j], c) == whole[y0:y1, x0:x1]).all(), j
    assert (got[outside(wtotal, wshapes, wplaces, c)] == POISON).all()


# ---- host forms -----------------------------------------------------------------------------------------------------------

def test_host_forms_equal_the_device_composition(gpu, product, oracle):
    geom = sm.GEOMS[0]
    bw, bh = geom[:2]
    for c, filt in ((4, 4), (3, 1)):
        files, scales = batch_of(oracle, geom, c)
        files, scales = files[:7], scales[:7]
        raws = [f.raw for f in files]
        to, host, dev = read_files(gpu, product, files)
        shapes = scaled_shapes(files, scales)
        places, total = place(shapes, c)
        dev_buf, _, _ = expand_scaled(gpu, files, scales, places, total, filt, dev)
        descs = [(f.w, f.h, p, o) for f, (p, o) in zip(files, places)]
        out = np.full(total, POISON, np.uint8)
        _, flags = gpu.decode_varied_files_scaled(raws, c, bw, bh, filt, scales, out=out, descs=descs)
        assert (flags == 0).all() and (out == dev_buf).all()
        images, _ = gpu.decode_varied_files_scaled(raws, c, bw, bh, filt, scales)
        assert all((img == f.image(filt)).all() for img, f in zip(images, files))
        # a header that disagrees with its descriptor names the file and writes nothing
        wrong = list(descs)
        wrong[4] = (descs[4][0] + 1,) + descs[4][1:]
        out[:] = POISON
        with pytest.raises(product.PxzError) as e:
            gpu.decode_varied_files_scaled(raws, c, bw, bh, filt, scales, out=out, descs=wrong)
        assert e.value.code == INVALID_ARG and "image 4" in str(e.value) and (out == POISON).all()
        # a file broken past its header flags only itself; the others are complete, the gaps untouched
        broken = list(raws)
        broken[2] = broken[2][:-9]
        with pytest.raises(product.PxzError) as e:
            gpu.decode_varied_files_scaled(broken, c, bw, bh, filt, scales, out=out, descs=descs)
        assert e.value.code == INVALID_ARG and "image 2" in str(e.value)
        assert [int(x != 0) for x in e.value.flags] == [int(i == 2) for i in range(len(files))] and e.value.flags[2] & 2
        for i, f in enumerate(files):
            if i != 2:
                assert (view(out, shapes[i], places[i], c) == f.image(filt)).all(), i
        assert (out[outside(total, shapes, places, c)] == POISON).all()

        # windows
        two = [files[1], files[3]]
        windows, wscales, wshapes, wplaces, wtotal = windows_of(two, [[0, 1, 2], [3]], c)
        dev_buf, wflags, status, _ = run_windows(gpu, product, two, windows, wscales, wtotal, filt)
        assert status == 0
        out = np.full(wtotal, POISON, np.uint8)
        _, flags = gpu.decode_windows_files_scaled([f.raw for f in two], windows, c, bw, bh, filt, wscales, out=out)
        assert (flags == 0).all() and (out == dev_buf).all()
        crops, _ = gpu.decode_windows_files_scaled([f.raw for f in two], [win[:5] for win in windows], c, bw, bh, filt, wscales)
        for crop, win, k in zip(crops, windows, wscales):
            x0, y0, x1, y1 = sm.scaled_rect(win[1:5], k)
            assert (crop == two[win[0]].image(filt, k)[y0:y1, x0:x1]).all()
        out[:] = POISON
        with pytest.raises(product.PxzError) as e:
            gpu.decode_windows_files_scaled([two[0].raw, two[1].raw[:20]], windows, c, bw, bh, filt, wscales, sizes=[(f.w, f.h) for f in two], out=out)
        assert "image 1" in str(e.value) and (out == POISON).all()
        with pytest.raises(product.PxzError) as e:
            gpu.decode_windows_files_scaled([two[0].raw, two[1].raw[:-9]], windows, c, bw, bh, filt, wscales, sizes=[(f.w, f.h) for f in two], out=out)
        assert e.value.code == INVALID_ARG
        assert [int(x != 0) for x in e.value.flags] == [int(win[0] == 1) for win in windows]
        for j, (win, k) in enumerate(zip(windows, wscales)):
            if win[0] == 0:
                x0, y0, x1, y1 = sm.scaled_rect(win[1:5], k)
                assert (view(out, wshapes[j], wplaces[j], c) == two[0].image(filt, k)[y0:y1, x0:x1]).all(), j
        assert (out[outside(wtotal, wshapes, wplaces, c)] == POISON).all()
