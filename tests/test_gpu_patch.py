"""Pixel windows patched into .pixlzr files on the device (pxz_patch_windows_device, pxz_splice_windows_device,
pxz_patch_windows_files).  The fixtures are tests/patch_model.py's -- 200x136 px in 32x32 tiles, 130x130 in 64x64, 150x70 in 48x20:
the smallest grids with interior tiles and ragged right and bottom tiles; RGB and RGBA, both modes, Lanczos3 and one Nearest -- and
the files are written by pxz_encode_varied_images.  Step 1 (tiles to tiles) is held against the composition of calls that existed
before it (window expand of the hull, overlay, varied shrink of the hulls) and against the model; step 2 (the splice) and the host
form against the model's file, byte for byte.  Every comparison is exact."""
import numpy as np
import pytest

import patch_model as pm
from test_gpu_varied_decode import upload_files, poisoned

pytestmark = pytest.mark.gpu

POISON = 0xA5
GUARD = 64
INVALID_ARG, TILE_TOO_SMALL, BUFFER_TOO_SMALL = -1, -4, -7
CASES = ("pixel", "inside", "inside a whole tile", "tile", "corner", "edge", "whole", "two")


@pytest.fixture(scope="module")
def gpu(product):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    h = product.Handle(0)
    yield h
    h.close()


# ---- the chain and what it is held against -----------------------------------------------------------------------------------

class Source:
    """one file of a call: its bytes and geometry"""

    def __init__(self, raw, w, h):
        self.raw, self.w, self.h = raw, w, h


def place_patches(rects, patches, c):
    """the windows' new pixels in one buffer, each at an odd address with a pitch that is no multiple of 4 -- every other RGBA one on
    dwords -- GUARD bytes around them -> (windows with pitch and offset, host buffer)"""
    windows, at = [], GUARD
    for k, ((i, x, y, w, h), px) in enumerate(zip(rects, patches)):
        if c == 4 and k % 2 == 1:
            at = (at + 3) & ~3
            pitch = w * 4 + 8
        else:
            at |= 1
            pitch = w * c + 5
            while pitch % 4 == 0:
                pitch += 1
        windows.append((i, x, y, w, h, pitch, at))
        at += pitch * h + GUARD
    buf = np.full(at, POISON, np.uint8)
    for (_, _, _, w, h, pitch, off), px in zip(windows, patches):
        np.lib.stride_tricks.as_strided(buf[off:], (h, w, c), (pitch, c, 1))[...] = px
    return windows, buf


def tiles_to_host(t):
    vals, ow, oh, slots = t
    return (vals.cpu().numpy(), ow.cpu().numpy().astype(np.uint32), oh.cpu().numpy().astype(np.uint32), None if slots is None else slots.cpu().numpy())


def same_tiles(got, want, c, what):
    gv, gw, gh, gs = got
    wv, ww, wh, ws = want
    assert len(gv) == len(wv), what
    assert (gw == ww).all() and (gh == wh).all(), (what, list(zip(gw, gh)), list(zip(ww, wh)))
    assert (gv.view(np.uint32) == wv.view(np.uint32)).all(), what
    for t in range(len(gv)):
        n = int(gw[t]) * int(gh[t]) * c
        assert (gs[t, :n] == ws[t, :n]).all(), (what, t)


class Chain:
    """reader of the windows -> patch -> splice over `sources` (one channel count and block size), everything kept.  lead: the files
    start that many bytes into their allocation; out: (file offsets, bytes) of the splice, the bytes any view of the caller's (or
    None, the size query); placement: (windows with pitch and offset, host buffer) made by the caller in place of place_patches'"""

    def __init__(self, gpu, product, sources, c, bw, bh, p, rects, patches, in_place=False, out=None, lead=3, break_tile=None,
                 placement=None):
        import torch
        self.sizes = [(s.w, s.h) for s in sources]
        plain = [(i, x, y, w, h, 0, 0) for (i, x, y, w, h) in rects]
        self.files, self.offs = upload_files([s.raw for s in sources], lead)
        to = product.patch_check(self.sizes, plain, bw, bh)
        self.T = int(to[-1])
        self.old, self.rflags = poisoned(self.T, bw * bh * c, len(rects))
        gpu.decode_windows_device(self.files, self.offs, self.sizes, plain, c, bw, bh, out=self.old, window_flags=self.rflags)
        if break_tile is not None:  # a stored size that cannot be
            self.old[1][break_tile] = 0
        self.old_host = tiles_to_host(self.old)
        self.windows, self.host_patch = place_patches(rects, patches, c) if placement is None else placement
        self.patch = torch.from_numpy(self.host_patch).cuda()
        self.pflags = torch.full((len(rects),), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        if in_place:
            vals = torch.full((self.T,), 0x7F7F7F7F, dtype=torch.int32, device="cuda").view(torch.float32)
            target = (vals, self.old[1], self.old[2], self.old[3])
        else:
            target, _ = poisoned(self.T, bw * bh * c, 1)
        self.new = gpu.patch_windows_device(self.sizes, self.windows, c, bw, bh, p.mode, p.filt, p.factor, p.expand_filter, self.patch,
                                            self.old[1], self.old[2], self.old[3], out=target, window_flags=self.pflags)
        self.status = gpu.decode_status()
        self.iflags = torch.full((len(sources),), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        self.out_offs, self.out = gpu.splice_windows_device(self.files, self.offs, self.sizes, plain, c, bw, bh, *self.new, reader_flags=self.rflags,
                                                            patch_flags=self.pflags, out=out, image_flags=self.iflags)
        torch.cuda.synchronize()
        self.new_host = tiles_to_host(self.new)
        self.o = self.out_offs.cpu().numpy()

    def file(self, i):
        return self.out[int(self.o[i]):int(self.o[i + 1])].cpu().numpy().tobytes()


def composition(gpu, product, chain, c, bw, bh, p, rects, patches):
    """what the patch must equal, from calls that existed before it: pxz_expand_windows_device of each window's hull into a packed
    image, the new pixels over it, pxz_shrink_varied_frames_device over the hulls as a varied batch"""
    import torch
    hulls, descs, at = [], [], 0
    for (i, x, y, w, h) in rects:
        hx, hy, hw, hh = pm.hull((x, y, w, h), chain.sizes[i], bw, bh)
        hulls.append((i, hx, hy, hw, hh, hw * c, at))
        descs.append((hw, hh, hw * c, at))
        at += hw * hh * c
    img = torch.full((at,), POISON, dtype=torch.uint8, device="cuda")
    gpu.expand_windows_device(chain.sizes, hulls, c, bw, bh, p.expand_filter, chain.old[1], chain.old[2], chain.old[3], img)
    for (i, x, y, w, h), (_, hx, hy, hw, hh, _, off), px in zip(rects, hulls, patches):
        view = img[off:off + hw * hh * c].view(hh, hw, c)
        view[y - hy:y - hy + h, x - hx:x - hx + w] = torch.from_numpy(np.ascontiguousarray(px)).cuda()
    _, vals, ow, oh, slots = gpu.shrink_varied_frames_device(img, bw, bh, p.mode, p.filt, p.factor, descs=descs, channels=c)
    torch.cuda.synchronize()
    return tiles_to_host((vals, ow, oh, slots))


def model(oracle, sources, c, p, rects, patches):
    """-> (the expected files, the expected covered tiles in the call's window order)"""
    files, tiles = [], [None] * len(rects)
    for i, s in enumerate(sources):
        mine = [k for k, r in enumerate(rects) if r[0] == i]
        if not mine:
            files.append(s.raw)
            continue
        new, per_window = pm.patched_file(oracle, s.raw, c, p, [(rects[k][1:], patches[k]) for k in mine])
        files.append(new)
        for k, t in zip(mine, per_window):
            tiles[k] = t
    cat = tuple(np.concatenate([t[j] for t in tiles]) for j in range(4))
    return files, cat


def host_form(gpu, sources, f_bw, f_bh, p, rects, patches, out=None):
    return gpu.patch_windows_files([s.raw for s in sources], rects, patches, f_bw, f_bh, p.mode, p.filt, p.factor, p.expand_filter, out=out)


def product_file(gpu, image, f):
    return gpu.encode_varied_images([image], f.bw, f.bh, f.p.mode, f.p.filt, f.p.factor)[0]


# ---- the cases -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(pm.FIXTURES))
def test_fixture_files_are_the_writers(gpu, oracle, name):
    """the file the host tests reason about is the file pxz_encode_varied_images writes"""
    f = pm.fixture(oracle, name)
    assert product_file(gpu, f.image, f) == f.raw


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("name", sorted(pm.FIXTURES))
def test_patch_equals_composition_and_model(gpu, product, oracle, name, case):
    f = pm.fixture(oracle, name)
    src = [Source(product_file(gpu, f.image, f), f.w, f.h)]
    rects = [(0,) + r for r in f.windows()[case]]
    patches = [pm.new_pixels(r[1:], f.c, 3) for r in rects]
    ch = Chain(gpu, product, src, f.c, f.bw, f.bh, f.p, rects, patches)
    assert ch.status == 0 and (ch.rflags.cpu().numpy() == 0).all() and (ch.pflags.cpu().numpy() == 0).all()
    want_files, want_tiles = model(oracle, src, f.c, f.p, rects, patches)
    same_tiles(ch.new_host, composition(gpu, product, ch, f.c, f.bw, f.bh, f.p, rects, patches), f.c, "composition")
    same_tiles(ch.new_host, want_tiles, f.c, "model")
    assert (ch.iflags.cpu().numpy() == 0).all()
    assert ch.file(0) == want_files[0]
    assert host_form(gpu, src, f.bw, f.bh, f.p, [r for r in rects], patches) == want_files
    if case == "whole":
        assert ch.file(0) == product_file(gpu, patches[0], f)


def small_sources(oracle, f, sizes):
    out = []
    for k, (w, h) in enumerate(sizes):
        img = pm.picture(w, h, f.c, f.bw, f.bh, 100 + k)
        v, tw, th, slots = oracle.shrink_image(img, f.bw, f.bh, f.p.mode, f.p.filt, f.p.factor)
        out.append(Source(oracle.encode_container(w, h, f.bw, f.bh, f.c, 7, v, None, tw, th, slots), w, h))  # (a filter byte that must stay)
    return out


@pytest.mark.parametrize("name", ("rgba-32-directional", "rgb-48x20-by"))
def test_three_files_one_without_a_window(gpu, product, oracle, name):
    """windows of the third file, then two in one tile row of the first; the second file has none and passes through"""
    f = pm.fixture(oracle, name)
    src = small_sources(oracle, f, [(f.w, f.h), (2 * f.bw + 6, f.bh + 8), (3 * f.bw + 4, 2 * f.bh + 5)])
    rects = [(2, f.bw - 2, f.bh - 3, 7, 5)] + [(0,) + r for r in f.windows()["two"]] + [(2, 2 * f.bw + 1, 1, 3, 3)]
    patches = [pm.new_pixels(r[1:], f.c, 4) for r in rects]
    ch = Chain(gpu, product, src, f.c, f.bw, f.bh, f.p, rects, patches, lead=1)
    want_files, want_tiles = model(oracle, src, f.c, f.p, rects, patches)
    same_tiles(ch.new_host, want_tiles, f.c, "model")
    assert [ch.file(i) for i in range(3)] == want_files
    assert ch.file(1) == src[1].raw and want_files[0][9] == 7
    assert (ch.iflags.cpu().numpy() == 0).all()
    assert host_form(gpu, src, f.bw, f.bh, f.p, rects, patches) == want_files


# ---- directed streams ----------------------------------------------------------------------------------------------------------

def records(raw):
    """[(first byte, bytes)] of every record of a file, and the first byte behind its line table"""
    w, h, bw, bh = (int.from_bytes(raw[o:o + 4], "big") for o in (10, 14, 18, 22))
    cols, rows = -(-w // bw), -(-h // bh)
    pos, out = 26 + 4 * rows, []
    for _ in range(cols * rows):
        n = 13 + int.from_bytes(raw[pos + 9:pos + 13], "big")
        out.append((pos, n))
        pos += n
    assert pos == len(raw)
    return out


def test_damage_outside_the_windows_arrives_verbatim(gpu, product, oracle):
    """a record right of the window in its tile row with garbage under a correct length field, and a tile row the window does not
    touch damaged throughout: neither is read, both are copied, the window is not flagged"""
    f = pm.fixture(oracle, "rgba-32-directional")
    recs = records(f.raw)
    bad = bytearray(f.raw)
    right = 1 * f.cols + 3  # tile (3, 1): the window covers (1, 1)
    pos, n = recs[right]
    bad[pos + 13:pos + n] = bytes((37 * k + 11) & 255 for k in range(n - 13))
    a, b = recs[3 * f.cols][0], recs[4 * f.cols][0]  # tile row 3
    bad[a + 2:b - 1] = bytes((91 * k + 5) & 255 for k in range(b - a - 3))
    src = [Source(bytes(bad), f.w, f.h)]
    rects = [(0,) + f.windows()["inside"][0]]
    patches = [pm.new_pixels(rects[0][1:], f.c, 5)]
    clean, _ = model(oracle, [Source(f.raw, f.w, f.h)], f.c, f.p, rects, patches)
    want = bytearray(clean[0])
    new_recs = records(clean[0])
    covered = set(pm.covered_tiles(rects[0][1:], f.size, f.bw, f.bh))
    for t, ((po, no), (pn, nn)) in enumerate(zip(recs, new_recs)):
        if t not in covered:
            assert no == nn
            want[pn:pn + nn] = bad[po:po + no]
    ch = Chain(gpu, product, src, f.c, f.bw, f.bh, f.p, rects, patches)
    assert (ch.rflags.cpu().numpy() == 0).all() and (ch.pflags.cpu().numpy() == 0).all() and (ch.iflags.cpu().numpy() == 0).all()
    assert ch.file(0) == bytes(want) and bytes(want) != clean[0]
    assert host_form(gpu, src, f.bw, f.bh, f.p, rects, patches) == [bytes(want)]


def test_a_broken_record_left_of_the_window_flags_it(gpu, product, oracle):
    f = pm.fixture(oracle, "rgb-32-by")
    recs = records(f.raw)
    bad = bytearray(f.raw)
    bad[recs[1 * f.cols][0] + 1] ^= 0x20  # "block" of tile (0, 1); the window covers (1, 1)
    src = [Source(bytes(bad), f.w, f.h), Source(f.raw, f.w, f.h)]
    rects = [(0,) + f.windows()["inside"][0], (1,) + f.windows()["inside"][0]]
    patches = [pm.new_pixels(r[1:], f.c, 6) for r in rects]
    ch = Chain(gpu, product, src, f.c, f.bw, f.bh, f.p, rects, patches)
    assert ch.rflags.cpu().numpy().tolist() == [2, 0]
    want, _ = model(oracle, [src[1]], f.c, f.p, [(0,) + rects[1][1:]], patches[1:])
    assert ch.file(0) == b"" and ch.file(1) == want[0]
    assert ch.iflags.cpu().numpy().tolist() == [2 | int(ch.pflags[0].item()), 0] and int(ch.pflags[1].item()) == 0
    out = np.full(len(f.raw) * 3, POISON, np.uint8)
    with pytest.raises(product.PxzError) as e:
        host_form(gpu, src, f.bw, f.bh, f.p, rects, patches, out=out)
    assert e.value.code == INVALID_ARG and "window 0" in str(e.value)
    assert (out == POISON).all() and (e.value.offsets == 0).all()


def test_a_stored_size_that_cannot_be_flags_a_wholly_covered_tile(gpu, product, oracle):
    """one rule for the splice: the tile is flagged and emptied as in the re-shrink although none of its stored pixels is needed"""
    f = pm.fixture(oracle, "rgba-64-by")
    src = [Source(f.raw, f.w, f.h)]
    rects = [(0,) + f.windows()["corner"][0]]
    patches = [pm.new_pixels(rects[0][1:], f.c, 7)]
    whole = [(0,) + f.windows()["tile"][0]]
    ch = Chain(gpu, product, src, f.c, f.bw, f.bh, f.p, whole, [pm.new_pixels(whole[0][1:], f.c, 7)], break_tile=0)
    assert ch.status == 1 and ch.pflags.cpu().numpy().tolist() == [1] and ch.iflags.cpu().numpy().tolist() == [1]
    v, w, h, s = ch.new_host
    assert (int(w[0]), int(h[0]), int(v.view(np.uint32)[0])) == (0, 0, 0) and (s[0] == POISON).all()
    assert ch.o.tolist() == [0, 0]
    ch = Chain(gpu, product, src, f.c, f.bw, f.bh, f.p, rects, patches, break_tile=2)  # one of four; the others are done
    v, w, h, s = ch.new_host
    _, want = model(oracle, src, f.c, f.p, rects, patches)
    assert (int(w[2]), int(h[2])) == (0, 0) and ch.pflags.cpu().numpy().tolist() == [1] and ch.o.tolist() == [0, 0]
    keep = [0, 1, 3]
    same_tiles(tuple(a[keep] for a in ch.new_host), tuple(a[keep] for a in want), f.c, "the other tiles")


# ---- capacity, in place, reuse, validation -------------------------------------------------------------------------------------

def test_capacity_and_size_query(gpu, product, oracle):
    import torch
    f = pm.fixture(oracle, "rgb-48x20-by")
    src = small_sources(oracle, f, [(f.w, f.h), (f.bw + 3, f.bh + 2)])
    rects = [(0,) + f.windows()["corner"][0]]
    patches = [pm.new_pixels(rects[0][1:], f.c, 8)]
    want, _ = model(oracle, src, f.c, f.p, rects, patches)
    total = sum(len(w) for w in want)
    exact = [0, len(want[0]), total]
    offs = torch.full((3,), -1, dtype=torch.int64, device="cuda")
    ch = Chain(gpu, product, src, f.c, f.bw, f.bh, f.p, rects, patches, out=(offs, None))  # the size query
    assert ch.o.tolist() == exact
    whole = torch.full((total + GUARD,), POISON, dtype=torch.uint8, device="cuda")
    ch = Chain(gpu, product, src, f.c, f.bw, f.bh, f.p, rects, patches, out=(offs, whole[:total - 1]))  # one byte short
    got = whole.cpu().numpy()
    assert ch.o.tolist() == exact and (got[total - 1:] == POISON).all()
    assert got[:total - 1].tobytes() == b"".join(want)[:total - 1]
    ch = Chain(gpu, product, src, f.c, f.bw, f.bh, f.p, rects, patches, out=(offs, whole[:total]))
    assert whole.cpu().numpy()[:total].tobytes() == b"".join(want) and (whole.cpu().numpy()[total:] == POISON).all()
    # the host form's protocol
    for room in (0, total - 1):
        out = np.full(room + GUARD, POISON, np.uint8)
        with pytest.raises(product.PxzError) as e:
            host_form(gpu, src, f.bw, f.bh, f.p, rects, patches, out=out[:room])
        assert e.value.code == BUFFER_TOO_SMALL and e.value.needed == total and e.value.offsets.tolist() == exact and (out == POISON).all()
    out = np.full(total + GUARD, POISON, np.uint8)
    assert host_form(gpu, src, f.bw, f.bh, f.p, rects, patches, out=out[:total]) == want and (out[total:] == POISON).all()


@pytest.mark.parametrize("name", ("rgba-32-directional", "rgb-64-directional"))
def test_in_place(gpu, product, oracle, name):
    f = pm.fixture(oracle, name)
    src = [Source(f.raw, f.w, f.h)]
    rects = [(0,) + f.windows()["edge"][0]]
    patches = [pm.new_pixels(rects[0][1:], f.c, 9)]
    want_files, want_tiles = model(oracle, src, f.c, f.p, rects, patches)
    ch = Chain(gpu, product, src, f.c, f.bw, f.bh, f.p, rects, patches, in_place=True)
    assert ch.new[1].data_ptr() == ch.old[1].data_ptr() and ch.new[3].data_ptr() == ch.old[3].data_ptr()
    same_tiles(ch.new_host, want_tiles, f.c, "in place")
    assert ch.file(0) == want_files[0]


def test_handle_reuse_across_geometries(gpu, product, oracle):
    """two geometries in turn on one handle, the scratch given back between the second and the third call"""
    for k, name in enumerate(("rgba-64-by", "rgb-48x20-by", "rgba-64-by")):
        f = pm.fixture(oracle, name)
        src = [Source(f.raw, f.w, f.h)]
        rects = [(0,) + r for r in f.windows()["two"]]
        patches = [pm.new_pixels(r[1:], f.c, 10 + k) for r in rects]
        want_files, want_tiles = model(oracle, src, f.c, f.p, rects, patches)
        ch = Chain(gpu, product, src, f.c, f.bw, f.bh, f.p, rects, patches)
        same_tiles(ch.new_host, want_tiles, f.c, name)
        assert ch.file(0) == want_files[0]
        assert host_form(gpu, src, f.bw, f.bh, f.p, rects, patches) == want_files
        if k == 1:
            gpu.trim()


def test_validation_runs_before_any_launch(gpu, product, oracle):
    import torch
    f = pm.fixture(oracle, "rgba-32-directional")
    src = [Source(f.raw, f.w, f.h)]
    sizes = [f.size]
    one = [(0, 1, 1, 5, 5, 20, 0)]
    T = 4
    (vals, ow, oh, slots), flags = poisoned(T, f.bw * f.bh * f.c, 2)
    patch = torch.zeros(4096, dtype=torch.uint8, device="cuda")

    def call(windows, mode=f.p.mode, sizes=sizes, expand_filter=4):
        return gpu.patch_windows_device(sizes, windows, f.c, f.bw, f.bh, mode, 4, 1.0, expand_filter, patch, ow, oh, slots,
                                        out=(vals, ow, oh, slots), window_flags=flags)
    for what, windows, code, text in (
            ("two windows in one tile", one + [(0, 20, 20, 3, 3, 12, 512)], INVALID_ARG, "window 1"),
            ("a pitch below a row", [(0, 1, 1, 5, 5, 19, 0)], INVALID_ARG, "window 0"),
            ("a rectangle that leaves the image", [(0, 190, 1, 20, 5, 80, 0)], INVALID_ARG, "window 0")):
        with pytest.raises(product.PxzError) as e:
            call(windows)
        assert e.value.code == code and text in str(e.value), what
    with pytest.raises(product.PxzError) as e:
        call(one, expand_filter=5)
    assert e.value.code == INVALID_ARG
    # shrink_directionally needs tiles of 2x2: judged on the covered tiles of a 65 px wide image, whose last column is 1 px wide
    narrow = [(65, 40)]
    with pytest.raises(product.PxzError) as e:
        call([(0, 60, 1, 5, 5, 20, 0)], mode=pm.DIRECTIONAL, sizes=narrow)
    assert e.value.code == TILE_TOO_SMALL and "window 0" in str(e.value)
    torch.cuda.synchronize()
    assert (flags.cpu().numpy() == 0x5A5A5A5A).all() and (ow.cpu().numpy() == 0x5A5A5A5A).all()  # nothing was written
    # ... and away from that edge the same image is patched
    img = pm.picture(65, 40, f.c, f.bw, f.bh, 77)
    v, tw, th, s = oracle.shrink_image(img, f.bw, f.bh, pm.SHRINK_BY, 4, 0.3)
    raw = oracle.encode_container(65, 40, f.bw, f.bh, f.c, 0, v, None, tw, th, s)
    rects = [(0, 30, 3, 9, 7)]
    patches = [pm.new_pixels(rects[0][1:], f.c, 12)]
    ch = Chain(gpu, product, [Source(raw, 65, 40)], f.c, f.bw, f.bh, f.p, rects, patches)
    want_files, want_tiles = model(oracle, [Source(raw, 65, 40)], f.c, f.p, rects, patches)
    same_tiles(ch.new_host, want_tiles, f.c, "away from the narrow edge")
    assert ch.file(0) == want_files[0]
    # the splice without the reader's scratch of these windows on a fresh handle
    h2 = product.Handle(0)
    try:
        with pytest.raises(product.PxzError) as e:
            h2.splice_windows_device(ch.files, ch.offs, [(65, 40)], [r + (0, 0) for r in rects], f.c, f.bw, f.bh, *ch.new)
        assert e.value.code == INVALID_ARG
    finally:
        h2.close()
