"""The expand kernels on the ends of the pixel-value domain: the stored-tile patterns of tests/stored_patterns.py -- 0/255 tiles whose
way up overshoots in both passes, alpha in 0..3 / 127, 128 / 254, 255, tiles whose only non-opaque (or only opaque) pixel sits at a
chosen stored index -- through every decode-side kernel text: the 32x32 matrix-core form and its one-row shortcut, the 2x2 groups of
16x16 tiles, the 64x64 RGBA and RGB instances, the general form (LDS and HBM image), the varied expand, the windows, the distortion
sums and the archive kernels' own expands.  Every comparison is equality with oracle.expand_image, every byte of every image (for
the sums and the archive kernels: with the composition built on it), into outputs that were poisoned where the binding takes them.
What the patterns make the oracle do (which clamps fire, where un-premultiply saturates or meets alpha 0, that a stored side of 1
always takes the one-row shortcuts) is asserted without a GPU in tests/test_expand_domain_host.py."""
import collections
import functools
import types

import numpy as np
import pytest

import stored_patterns as sp
from test_gpu_value_domain import same_tiles

pytestmark = pytest.mark.gpu

NEAREST, TRIANGLE, CATMULLROM, GAUSSIAN, LANCZOS3 = range(5)
FILTERS = [NEAREST, TRIANGLE, CATMULLROM, GAUSSIAN, LANCZOS3]
POISON = 0xA5
POISON64 = 0x5A5A5A5A5A5A5A5A
ALL = ("pow2", "one pass", "odd", "clone")


@pytest.fixture(scope="module")
def gpu(product):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    h = product.Handle(0)
    yield h
    h.close()


# ---- frames and references: made once, shared by every test, never written to -------------------------------------------------------

def frozen(width, height, tile_w, tile_h, slots, names):
    for a in (tile_w, tile_h, slots):
        a.setflags(write=False)
    return types.SimpleNamespace(W=width, H=height, tw=tile_w, th=tile_h, slots=slots, names=tuple(names))


@functools.lru_cache(maxsize=None)
def frame(bw, bh, channels, classes=ALL, patterns=None, rotate=0, cols=None):
    """the items of sp.items(bw, bh, channels, classes, patterns), started `rotate` items in, as one frame"""
    items = sp.items(bw, bh, channels, classes, patterns)
    return frozen(*sp.layout(items[rotate:] + items[:rotate], bw, bh, channels, cols))


_expected = {}


def expected(oracle, key, lay, bw, bh, channels, filt):
    """oracle.expand_image of a frame, once per (frame, filter)"""
    key = (key, bw, bh, channels, filt)
    if key not in _expected:
        img = oracle.expand_image(lay.W, lay.H, bw, bh, channels, filt, lay.tw, lay.th, lay.slots)
        img.setflags(write=False)
        _expected[key] = img
    return _expected[key]


def same_image(got, exp, lay, bw, bh, what):
    """every byte; on a difference the pattern and stored size of the tiles that differ"""
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    bad = (got != exp).any(axis=2)
    if bad.any():
        cols = -(-lay.W // bw)
        ys, xs = np.nonzero(bad)
        tiles = sorted(set(((ys // bh) * cols + xs // bw).tolist()))
        shown = ", ".join(f"{lay.names[t]} (tile {t})" for t in tiles[:12])
        count = lambda part: dict(collections.Counter(part(lay.names[t]) for t in tiles).most_common())  # noqa: E731
        raise AssertionError(f"{what}: {int(bad.sum())} pixels differ in {len(tiles)} of {len(lay.names)} tiles: {shown}\n"
                             f"  by stored size: {count(lambda n: n.rsplit(' ', 1)[1])}\n"
                             f"  by pattern: {count(lambda n: n.rsplit(' ', 1)[0].split(' @')[0])}")


def on_device(lays):
    """frames of one grid -> (w[N,T], h[N,T], slots[N,T,S]) on the device"""
    import torch
    i32 = lambda a: torch.from_numpy(np.stack(a).astype(np.int32)).cuda()  # noqa: E731
    return i32([l.tw for l in lays]), i32([l.th for l in lays]), torch.from_numpy(np.stack([l.slots for l in lays])).cuda()


def expand_frames(gpu, lays, bw, bh, channels, filt, dev=None):
    """pxz_expand_frames_device into a poisoned batch -> host [N, H, W, C]"""
    import torch
    dev = dev if dev is not None else on_device(lays)
    out = torch.full((len(lays), lays[0].H, lays[0].W, channels), POISON, dtype=torch.uint8, device="cuda")
    gpu.expand_frames_device(tuple(out.shape), bw, bh, filt, *dev, out=out)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def check_both_forms(gpu, oracle, bw, bh, channels, filt, key_a, a, key_b, b, what):
    """the host form on frame a; the device form on (a, b) in one batch, so that a wave's next tile comes from another frame"""
    exp_a, exp_b = expected(oracle, key_a, a, bw, bh, channels, filt), expected(oracle, key_b, b, bw, bh, channels, filt)
    got = gpu.expand_image(a.W, a.H, channels, bw, bh, filt, a.tw, a.th, a.slots)
    assert gpu.decode_status() == 0, what
    same_image(got, exp_a, a, bw, bh, f"{what}, host form")
    assert (a.W, a.H) == (b.W, b.H) and len(a.names) == len(b.names)
    both = expand_frames(gpu, (a, b), bw, bh, channels, filt)
    assert gpu.decode_status() == 0, what
    same_image(both[0], exp_a, a, bw, bh, f"{what}, device form, frame 0")
    same_image(both[1], exp_b, b, bw, bh, f"{what}, device form, frame 1")


def status_bit_0_still_works(gpu, lay, bw, bh, channels, filt):
    """behind the patterns, on the same handle: a stored width above its place is flagged, and the next valid call clears it"""
    tw, th, slots = on_device((lay,))
    bad = tw.clone()
    bad[0, 0] = bw + 1
    expand_frames(gpu, (lay,), bw, bh, channels, filt, dev=(bad, th, slots))
    assert gpu.decode_status() == 1
    expand_frames(gpu, (lay,), bw, bh, channels, filt, dev=(tw, th, slots))
    assert gpu.decode_status() == 0


def pair_of_frames(bw, bh, channels, classes=ALL, patterns=None):
    n = len(sp.items(bw, bh, channels, classes, patterns))
    return frame(bw, bh, channels, classes, patterns), frame(bw, bh, channels, classes, patterns, rotate=n // 2 + 1)


# ---- 32x32 RGBA: expand_kernel<4, true> ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("filt", FILTERS)
def test_32x32_every_power_of_two_pair_and_pattern(gpu, oracle, filt):
    """every pair of {1, 2, 4, 8, 16}^2 with every pattern: expand_tile_mfma (signed-byte products, the bias row, clamp_fixed against
    the run-time top, the SDWA byte pack, the staging gate round by round, the un-premultiply gate) for the four convolutions,
    expand_tile_nearest_pow2 for Nearest; the n x 1 pairs take the matrix-core form's one-row shortcut.  The ragged tiles (7 px
    wide, 5 px high) carry the same patterns through the general form."""
    a, b = pair_of_frames(32, 32, 4, ("pow2",))
    assert {(int(w), int(h)) for w, h in zip(a.tw, a.th)} >= {(x, y) for x in (1, 2, 4, 8, 16) for y in (1, 2, 4, 8, 16)}
    check_both_forms(gpu, oracle, 32, 32, 4, filt, "32 pow2 a", a, "32 pow2 b", b, f"32x32 powers of two, filter {filt}")
    status_bit_0_still_works(gpu, a, 32, 32, 4, filt)


@pytest.mark.parametrize("filt", FILTERS)
def test_32x32_one_pass_odd_sizes_and_clones(gpu, oracle, filt):
    """32 x n and n x 32 (one pass), 3x8, 8x5, 31x16, 12x12 and the ragged edge through the general vector form inside the 32x32
    instance; tiles stored at 32x32 through expand_tile_clone32 -- each with every pattern"""
    a, b = pair_of_frames(32, 32, 4, ("one pass", "odd", "clone"))
    check_both_forms(gpu, oracle, 32, 32, 4, filt, "32 rest a", a, "32 rest b", b, f"32x32 one pass / odd / clone, filter {filt}")


@functools.lru_cache(maxsize=None)
def one_row_frame(rotate):
    items = [(n, w, 1) for w in sp.ONE_ROW_WIDTHS for n in sp.ALPHA + sp.one_pixel_names(w, 1)]
    return frozen(*sp.layout(items[rotate:] + items[:rotate], 32, 32, 4))


@pytest.mark.parametrize("filt", [TRIANGLE, CATMULLROM, GAUSSIAN, LANCZOS3])
def test_32x32_one_stored_row_low_alpha_and_one_pixel(gpu, oracle, filt):
    """stored rows 1, 2, 4, 8, 16 wide (the matrix-core form's "copied" shortcut: the row is un-premultiplied once and written 32
    times) and 32, 31, 12, 3 wide (the general form's one_row shortcut, with and without a horizontal pass before it), each as
    every alpha pattern and every one-pixel tile.  tests/test_expand_domain_host.py: a stored side of 1 is always the single
    full-weight tap, so every one of these takes its shortcut -- there is no n x 1 tile that goes the long way."""
    a, b = one_row_frame(0), one_row_frame(37)
    check_both_forms(gpu, oracle, 32, 32, 4, filt, "one row a", a, "one row b", b, f"32x32 one stored row, filter {filt}")


# ---- 16x16 RGBA: expand16_kernel and its LIST launch ------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def groups_frame(which):
    """2x2 groups with exactly one alpha or one-pixel tile (eligible for the group form: both sides in {1, 2, 4, 8}) among three
    opaque ones; the opaque ones go through every stored pair, so groups mix sizes, and eligible tiles with listed ones and clones"""
    special = [i for i in sp.items(16, 16, 4, ("pow2",)) if i[0] not in sp.OPAQUE]
    fillers = sp.items(16, 16, 4, ALL, sp.OPAQUE)
    if which:  # the second frame: other groups, other neighbours
        special, fillers = special[::-1], fillers[5:] + fillers[:5]
    return frozen(*sp.layout(sp.group_items(special, fillers, 24), 16, 16, 4, cols=24))


@pytest.mark.parametrize("filt", FILTERS)
def test_16x16_groups_with_one_alpha_tile_among_three_opaque(gpu, oracle, filt):
    """expand16_kernel: the premultiply decision is one ballot for the whole group and un-premultiply one per channel set, so a
    group is driven with exactly ONE tile that is not opaque, in each of its four positions, next to opaque tiles of other stored
    sizes (the block-diagonal weights, the zeroed columns of the other tile), to listed ones (16 x n, odd sizes) and to clones.
    25 columns of tiles: the last full column has no partner and goes to the list with the ragged one."""
    a, b = groups_frame(0), groups_frame(1)
    cols = -(-a.W // 16)
    assert cols % 2 == 1
    seen = set()
    for r in range(0, a.H // 16 - 1, 2):
        for c in range(0, cols - 2, 2):
            group = [a.names[(r + dr) * cols + c + dc] for dr in (0, 1) for dc in (0, 1)]
            special = [k for k, n in enumerate(group) if n.rsplit(" ", 1)[0] not in sp.OPAQUE]
            if len(special) == 1:
                seen.add(special[0])
            assert len(special) <= 1, group
    assert seen == {0, 1, 2, 3}
    check_both_forms(gpu, oracle, 16, 16, 4, filt, "16 groups a", a, "16 groups b", b, f"16x16 groups, filter {filt}")


@pytest.mark.parametrize("filt", FILTERS)
def test_16x16_every_pair_and_pattern(gpu, oracle, filt):
    """every pattern at every stored pair, row-major: groups of four alpha tiles, of mixed stored sizes, 16 x n and odd sizes and
    the partial groups of an odd column count through the LIST launch of the general form"""
    a, b = pair_of_frames(16, 16, 4)
    assert (-(-a.W // 16)) % 2 == 1 or (-(-a.H // 16)) % 2 == 1
    check_both_forms(gpu, oracle, 16, 16, 4, filt, "16 all a", a, "16 all b", b, f"16x16 every pair, filter {filt}")
    status_bit_0_still_works(gpu, a, 16, 16, 4, filt)


# ---- 64x64 RGBA and RGB: expand64_kernel<4>, <3> -----------------------------------------------------------------------------------

@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("channels", [4, 3])
def test_64x64_every_pair_and_pattern(gpu, oracle, channels, filt):
    """stored heights 1..8, 16 and 32 (expand64_conv<1>, <2>, <4>), 64 x n (expand64_vonly) and n x 64 (expand64_honly), clones,
    Nearest, and 3x8, 8x5, 63x32, 12x12 with the ragged edge as listed leftovers.  RGBA: every pattern, both staging forms (a
    pixel per lane below 4 px of width or 64 px in all, else four).  RGB: the opaque patterns; the frame is 64 k + 7 px wide, so
    its rows start at every byte alignment mod 4, and the twelve-byte pack of x64_store_quadrant<3> gets saturated inputs."""
    a, b = pair_of_frames(64, 64, channels)
    assert a.W % 64 == 7 and (channels == 4 or {(r * a.W * 3) % 4 for r in range(4)} == {0, 1, 2, 3})
    heights = {int(h) for w, h in zip(a.tw, a.th) if w < 64 and h < 64}
    assert heights >= {1, 2, 4, 8, 16, 32}
    check_both_forms(gpu, oracle, 64, 64, channels, filt, "64 a", a, "64 b", b, f"64x64 c{channels}, filter {filt}")
    if filt == LANCZOS3:
        status_bit_0_still_works(gpu, a, 64, 64, channels, filt)


# ---- the general form: expand_kernel<4>, <3> ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("filt", [NEAREST, GAUSSIAN, CATMULLROM, LANCZOS3])
@pytest.mark.parametrize("channels", [4, 3])
@pytest.mark.parametrize("bw,bh", [(48, 20), (24, 24)])
def test_general_form_every_pair_and_pattern(gpu, oracle, bw, bh, channels, filt):
    """tile sizes without a fast path: the level pairs, sides of 1 and 2, the one-pass pairs, 5x3 and a side short of full, the
    clone; the dot2 passes with their clamps, the one_row shortcut, un-premultiply behind its gate; the scalar form on the ragged
    column (7 px: no multiple of four)"""
    a, b = pair_of_frames(bw, bh, channels)
    check_both_forms(gpu, oracle, bw, bh, channels, filt, "general a", a, "general b", b, f"{bw}x{bh} c{channels}, filter {filt}")
    if filt == LANCZOS3:
        status_bit_0_still_works(gpu, a, bw, bh, channels, filt)


@functools.lru_cache(maxsize=None)
def big_frame(start):
    """2x2 full tiles of 192x192 (and the ragged ones): stored sizes from 1x1 up, the patterns dealt over them"""
    pairs = sp.all_pairs(192, 192)
    items = []
    for k in range(4):
        tw, th = pairs[(start + k) % len(pairs)]
        have = sp.names(tw, th, 4)
        want = [n for n in sp.BIG_PATTERNS[(start + k) % len(sp.BIG_PATTERNS):] + sp.BIG_PATTERNS if n in have]
        items.append((want[0], tw, th))
    return frozen(*sp.layout(items, 192, 192, 4, cols=2))


def test_192x192_tiles_with_their_image_in_hbm(gpu, oracle):
    """expand_kernel<4, false, true> (BIG): 192x192 tiles, whose image does not fit LDS, stored from 1x1 up -- four frames of 2x2
    full tiles, two filters with negative lobes and Nearest"""
    starts = (0, 4, 8, 11)
    sizes = {(int(w), int(h)) for s in starts for w, h in zip(big_frame(s).tw, big_frame(s).th)}
    assert sizes >= set(sp.all_pairs(192, 192))
    for filt in (LANCZOS3, CATMULLROM, NEAREST):
        for s in starts:
            lay = big_frame(s)
            got = expand_frames(gpu, (lay,), 192, 192, 4, filt)[0]
            assert gpu.decode_status() == 0
            same_image(got, expected(oracle, ("192", s), lay, 192, 192, 4, filt), lay, 192, 192, f"192x192 frame {s}, filter {filt}")


# ---- the varied expand and the windows (pxz_varied_tile.h) ---------------------------------------------------------------------------

def not_opaque(bw, bh):
    """the names of the alpha and one-pixel tiles of every stored pair of a bw x bh tile, each once"""
    return tuple(dict.fromkeys(n for tw, th in sp.all_pairs(bw, bh) for n in sp.names(tw, th, 4) if n not in sp.OPAQUE))


@functools.lru_cache(maxsize=None)
def three_images(bw, bh, channels):
    """three images of different sizes: the alpha and one-pixel tiles (RGB: the opaque ones) of three classes of stored pairs"""
    other = None if channels == 3 else not_opaque(bw, bh)
    lays = (frame(bw, bh, channels, ("pow2",), other),
            frame(bw, bh, channels, ("one pass", "clone"), sp.OPAQUE[:6] + sp.ALPHA[:3] if channels == 4 else None, cols=6),
            frame(bw, bh, channels, ("odd",), cols=9))
    assert len({(l.W, l.H) for l in lays}) == 3
    return lays


def varied_tiles(lays):
    import torch
    i32 = lambda a: torch.from_numpy(np.concatenate(a).astype(np.int32)).cuda()  # noqa: E731
    return i32([l.tw for l in lays]), i32([l.th for l in lays]), torch.from_numpy(np.concatenate([l.slots for l in lays])).cuda()


@pytest.mark.parametrize("bw,bh,channels", [(32, 32, 4), (32, 32, 3), (64, 64, 4), (48, 20, 4)])
def test_varied_batch_of_three_pattern_images(gpu, oracle, bw, bh, channels):
    """pxz_expand_varied_frames_device (varied_resize_tile): three images of different sizes at odd offsets with padded rows, into a
    poisoned buffer; every image's flag is 0 and nothing outside the images is written"""
    import torch
    from test_gpu_varied_decode import image_of, layout
    lays = three_images(bw, bh, channels)
    descs, total = layout([(l.W, l.H) for l in lays], channels, pad=12, misalign=3)
    dev = varied_tiles(lays)
    for filt in (LANCZOS3, CATMULLROM, TRIANGLE, NEAREST):
        out = torch.full((total,), POISON, dtype=torch.uint8, device="cuda")
        flags = torch.full((3,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        gpu.expand_varied_frames_device(descs, channels, bw, bh, filt, *dev, out, image_flags=flags)
        torch.cuda.synchronize()
        assert gpu.decode_status() == 0 and (flags.cpu().numpy() == 0).all()
        buf = out.cpu().numpy()
        covered = np.zeros(total, bool)
        for i, (lay, d) in enumerate(zip(lays, descs)):
            same_image(image_of(buf, d, channels), expected(oracle, ("varied", i), lay, bw, bh, channels, filt), lay, bw, bh,
                       f"varied {bw}x{bh} c{channels} filter {filt} image {i}")
            for y in range(lay.H):
                covered[d[3] + y * d[2]: d[3] + y * d[2] + lay.W * channels] = True
        assert (buf[~covered] == POISON).all(), "bytes outside the images were written"


@pytest.mark.parametrize("channels", [4, 3])
def test_windows_cut_through_pattern_tiles(gpu, oracle, product, channels):
    """pxz_expand_windows_device at 32x32: crops that start and end inside pattern tiles (and one that covers the ragged corner)
    equal the same rectangle of the oracle's whole-image expansion"""
    import torch
    from test_gpu_windows import GUARD, outside_mask, place, window_view
    from test_gpu_windows import POISON as WPOISON
    lays = three_images(32, 32, channels)
    sizes = [(l.W, l.H) for l in lays]
    rects = []
    for i, l in enumerate(lays):
        rects += [(i, 17, 9, 3 * 32 + 5, 2 * 32 + 11), (i, l.W - 45, l.H - 40, 45, 40), (i, 33, 31, 30, 34), (i, 0, 0, l.W, 7),
                  (i, 5 * 32 + 1, 3, 2, l.H - 3)]
    assert GUARD > 0 and all(x >= 0 and y >= 0 and x + w <= sizes[i][0] and y + h <= sizes[i][1] for i, x, y, w, h in rects)
    windows, total = place(rects, channels)
    to = product.window_layout(sizes, windows, 32, 32)
    # the covered tiles of every window, in the window layout's order
    pick, base = [], np.concatenate([[0], np.cumsum([len(l.names) for l in lays])])
    for (i, x, y, w, h) in rects:
        cols = -(-sizes[i][0] // 32)
        c0, r0, c1, r1 = x // 32, y // 32, (x + w - 1) // 32, (y + h - 1) // 32
        pick += [int(base[i]) + r * cols + c for r in range(r0, r1 + 1) for c in range(c0, c1 + 1)]
    assert len(pick) == int(to[-1])
    tw, th, slots = varied_tiles(lays)
    idx = torch.tensor(pick, dtype=torch.int64, device="cuda")
    dev = (tw[idx].contiguous(), th[idx].contiguous(), slots[idx].contiguous())
    for filt in (LANCZOS3, CATMULLROM, NEAREST):
        out = torch.full((total,), WPOISON, dtype=torch.uint8, device="cuda")
        flags = torch.full((len(windows),), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        gpu.expand_windows_device(sizes, windows, channels, 32, 32, filt, *dev, out, window_flags=flags)
        torch.cuda.synchronize()
        assert gpu.decode_status() == 0 and (flags.cpu().numpy() == 0).all()
        buf = out.cpu().numpy()
        for k, win in enumerate(windows):
            i, x, y, w, h = win[:5]
            exp = expected(oracle, ("varied", i), lays[i], 32, 32, channels, filt)[y:y + h, x:x + w]
            bad = (window_view(buf, win, channels) != exp).any(axis=2)
            assert not bad.any(), f"c{channels} filter {filt} window {k} {win[:5]}: {int(bad.sum())} of {w * h} pixels differ from the oracle's crop"
        assert (buf[outside_mask(buf.size, windows, channels)] == WPOISON).all(), "bytes outside the windows were written"


# ---- distortion ---------------------------------------------------------------------------------------------------------------------

def tile_sums(d, width, height, bw, bh):
    """d [H, W, C] int64 -> per tile and channel its sum, int64 [tiles, C]"""
    return np.array([d[y:y + bh, x:x + bw].sum(axis=(0, 1)) for y in range(0, height, bh) for x in range(0, width, bw)], np.int64)


@pytest.mark.parametrize("bw,bh,channels", [(32, 32, 4), (32, 32, 3), (48, 20, 4)])
def test_distortion_against_a_source_chosen_against_the_expansion(gpu, oracle, bw, bh, channels):
    """pxz_distortion_varied_frames_device: the source is black where the oracle's expansion is 128 or more and white elsewhere, so
    that every difference is large; per tile and channel the sums equal ((source - oracle.expand_image)^2) added up in int64,
    and the images' totals their sums.  A tile stored at its full size counts as its own source: zeros."""
    import torch
    from test_gpu_distortion import odd_layout
    lays = three_images(bw, bh, channels)
    descs, total = odd_layout([(l.W, l.H) for l in lays], channels)
    dev = varied_tiles(lays)
    for filt in (LANCZOS3, CATMULLROM, NEAREST):
        buf = np.full(total, POISON, np.uint8)
        exp_tiles = []
        for i, (lay, (w, h, pitch, off)) in enumerate(zip(lays, descs)):
            exp = expected(oracle, ("varied", i), lay, bw, bh, channels, filt)
            src = np.where(exp >= 128, 0, 255).astype(np.uint8)
            np.lib.stride_tricks.as_strided(buf[off:], (h, w, channels), (pitch, channels, 1))[...] = src
            sums = tile_sums((src.astype(np.int64) - exp.astype(np.int64)) ** 2, w, h, bw, bh)
            cols = -(-w // bw)
            for t in range(len(lay.names)):
                fw, fh = min(bw, w - (t % cols) * bw), min(bh, h - (t // cols) * bh)
                if (lay.tw[t], lay.th[t]) == (fw, fh):
                    sums[t] = 0
            assert sums.max() >= 127 * 127 * 16
            exp_tiles.append(sums)
        exp_tiles = np.concatenate(exp_tiles)
        T = exp_tiles.shape[0]
        tiles = torch.full((T, channels), POISON64, dtype=torch.int64, device="cuda")
        totals = torch.full((3, channels), POISON64, dtype=torch.int64, device="cuda")
        flags = torch.full((3,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        gpu.distortion_varied_frames_device(torch.from_numpy(buf).cuda(), bw, bh, filt, *dev, descs=descs, channels=channels,
                                            out=(tiles, totals), image_flags=flags)
        torch.cuda.synchronize()
        assert gpu.decode_status() == 0 and (flags.cpu().numpy() == 0).all()
        got = tiles.cpu().numpy()
        bad = np.nonzero((got != exp_tiles).any(axis=1))[0]
        names = [n for l in lays for n in l.names]
        assert bad.size == 0, f"{bw}x{bh} c{channels} filter {filt}: {bad.size} tiles differ: " + ", ".join(f"{names[t]} (tile {t}) {got[t].tolist()} != {exp_tiles[t].tolist()}" for t in bad[:6])
        at = np.concatenate([[0], np.cumsum([len(l.names) for l in lays])])
        assert (totals.cpu().numpy() == np.stack([exp_tiles[a:b].sum(axis=0) for a, b in zip(at[:-1], at[1:])])).all()


@pytest.mark.parametrize("channels", [4, 3])
def test_distortion_sums_at_the_largest_block(gpu, product, channels):
    """The largest square block pxz_distortion_varied_frames_device accepts (found from its refusal one step beyond), tiles stored
    1x1 white over a black source: a tile's sum is bw * bh * 255^2 per channel exactly -- what the kernel's uint32 accumulation
    must hold (its comment bounds a tile at 20480 pixels) -- and the first image holds enough tiles for its 64-bit total to pass
    2^32.  Nearest and Lanczos3 (a stored 1x1 is one full-weight tap: the expansion is white either way)."""
    import torch

    def accepted(n):
        src = torch.zeros((channels,), dtype=torch.uint8, device="cuda")
        one = torch.ones((1,), dtype=torch.int32, device="cuda")
        try:
            gpu.distortion_varied_frames_device(src, n, n, LANCZOS3, one, one, torch.zeros((1, n * n * channels), dtype=torch.uint8, device="cuda"),
                                                descs=[(1, 1, channels, 0)], channels=channels)
        except product.PxzError:
            return False
        return True

    lo, hi = 64, 512
    assert accepted(lo) and not accepted(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if accepted(mid) else (lo, mid)
    n = lo
    assert 100 <= n and n * n < 20480 and n * n * 65025 < 2 ** 32, n
    sizes = [(3 * n + 5, 2 * n + 3), (n, n)]
    per_image = [[(min(n, w - x), min(n, h - y)) for y in range(0, h, n) for x in range(0, w, n)] for (w, h) in sizes]
    rects = [r for p in per_image for r in p]
    T = len(rects)
    exp = np.array([[fw * fh * 65025] * channels for fw, fh in rects], np.int64)
    assert exp[: len(per_image[0])].sum(axis=0)[0] > 2 ** 32 and exp.max() == n * n * 65025 > 2 ** 29
    descs, at = [], 3
    for (w, h) in sizes:
        descs.append((w, h, w * channels + 5, at))
        at += (w * channels + 5) * h + 1
    src = torch.zeros((at,), dtype=torch.uint8, device="cuda")
    ones = torch.ones((T,), dtype=torch.int32, device="cuda")
    slots = torch.zeros((T, n * n * channels), dtype=torch.uint8, device="cuda")
    slots[:, :channels] = 255
    for filt in (LANCZOS3, NEAREST):
        tiles = torch.full((T, channels), POISON64, dtype=torch.int64, device="cuda")
        totals = torch.full((2, channels), POISON64, dtype=torch.int64, device="cuda")
        gpu.distortion_varied_frames_device(src, n, n, filt, ones, ones, slots, descs=descs, channels=channels, out=(tiles, totals))
        torch.cuda.synchronize()
        assert gpu.decode_status() == 0
        assert (tiles.cpu().numpy() == exp).all(), (n, filt, tiles.cpu().numpy().tolist())
        k = len(per_image[0])
        assert (totals.cpu().numpy() == np.stack([exp[:k].sum(axis=0), exp[k:].sum(axis=0)])).all(), (n, filt)


# ---- the archive kernels: their own expands, and retile_assemble --------------------------------------------------------------------

NOT_OPAQUE_32 = not_opaque(32, 32)
# (64x64 source tiles: fewer patterns, so that the oracle's shrink of the whole image stays quick)
NOT_OPAQUE_64 = ("alpha 1..3", "alpha extremes", "alpha checker 254/255", "alpha v stripes 3/255", "white alpha 0", "one 254 @0", "one 0 @63",
                 "one 254 @64", "lone opaque @0")
FACTORS = (64.0, 1.0, 1.0 / 64.0)  # (what each decides is the oracle's business: three spread over the walk of value_patterns)


def upload(tw, th, slots):
    import torch
    return (torch.from_numpy(np.asarray(tw).astype(np.int32)).cuda(), torch.from_numpy(np.asarray(th).astype(np.int32)).cuda(),
            torch.from_numpy(np.array(slots)).cuda())


def fetch(out):
    return (out[0].cpu().numpy(), out[1].cpu().numpy().astype(np.uint32), out[2].cpu().numpy().astype(np.uint32), out[3].cpu().numpy())


@pytest.mark.parametrize("mode", [0, 1])
def test_reshrink_of_alpha_and_one_pixel_tiles(gpu, oracle, mode):
    """pxz_reshrink_varied_frames_device at 32x32 over stored tiles that ARE the alpha and one-pixel patterns (no shrink made
    them): the kernel's own expand, then its shrink, equal oracle.expand_image + oracle.shrink_image bit for bit"""
    import torch
    from test_gpu_varied_decode import poisoned
    lay = frame(32, 32, 4, ALL, NOT_OPAQUE_32)
    for xf in (LANCZOS3, CATMULLROM):
        back = expected(oracle, "not opaque 32", lay, 32, 32, 4, xf)
        for k in FACTORS:
            out, flags = poisoned(len(lay.names), 32 * 32 * 4, 1)
            gpu.reshrink_varied_frames_device([(lay.W, lay.H)], 4, 32, 32, mode, LANCZOS3, k, xf, *upload(lay.tw, lay.th, lay.slots), out=out,
                                              image_flags=flags)
            torch.cuda.synchronize()
            assert gpu.decode_status() == 0 and int(flags[0]) == 0
            same_tiles(fetch(out), oracle.shrink_image(np.array(back), 32, 32, mode, LANCZOS3, k), 4,
                       f"re-shrink, expand filter {xf}, mode {mode} k={k}", lay.names)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("src,dst", [((64, 64), (32, 32)), ((32, 32), (48, 20))])
def test_retile_of_alpha_and_one_pixel_tiles(gpu, oracle, src, dst, mode):
    """pxz_retile_varied_frames_device: the source tiles are the alpha and one-pixel patterns at every stored pair, the clones
    among them (retile_assemble copies those parts and expands the others); 64 -> 32 (a destination tile inside one source tile)
    and 32 -> 48x20 (straddling).  Equal to oracle.expand_image at the source block + oracle.shrink_image at the new one."""
    import torch
    from test_gpu_varied_decode import poisoned
    lay = frame(*src, 4, ALL, NOT_OPAQUE_64 if src == (64, 64) else NOT_OPAQUE_32)
    T = -(-lay.W // dst[0]) * -(-lay.H // dst[1])
    names = [f"destination tile {t}" for t in range(T)]
    back = np.array(expected(oracle, ("not opaque", src), lay, *src, 4, LANCZOS3))
    for k in FACTORS:
        out, flags = poisoned(T, dst[0] * dst[1] * 4, 1)
        gpu.retile_varied_frames_device([(lay.W, lay.H)], 4, *src, *dst, mode, LANCZOS3, k, LANCZOS3, *upload(lay.tw, lay.th, lay.slots), out=out,
                                        image_flags=flags)
        torch.cuda.synchronize()
        assert gpu.decode_status() == 0 and int(flags[0]) == 0
        same_tiles(fetch(out), oracle.shrink_image(back, *dst, mode, LANCZOS3, k), 4, f"re-tile {src} -> {dst} mode {mode} k={k}", names)


def archive_sums(oracle, ref_img, width, height, bw, bh, filt, sets):
    """int64 [K, T, 4]: per set, tile of the bw x bh grid and channel the sum of (reference image - oracle expansion of the set)^2;
    zeros where the set stores the tile at its full size (the archive kernels take such a tile as unchanged)"""
    out = []
    cols = -(-width // bw)
    for (tw, th, slots, _) in sets:
        img = oracle.expand_image(width, height, bw, bh, 4, filt, tw, th, slots)
        sums = tile_sums((ref_img.astype(np.int64) - img.astype(np.int64)) ** 2, width, height, bw, bh)
        for t in range(len(tw)):
            if (tw[t], th[t]) == (min(bw, width - (t % cols) * bw), min(bh, height - (t // cols) * bh)):
                sums[t] = 0
        out.append(sums)
    return np.stack(out)


def archive_call(call, K, T, sets):
    import torch
    tiles = torch.full((K, T, 4), POISON64, dtype=torch.int64, device="cuda")
    totals = torch.full((K, 1, 4), POISON64, dtype=torch.int64, device="cuda")
    flags = torch.full((1,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    dev_sets = upload(np.stack([s[0] for s in sets]), np.stack([s[1] for s in sets]), np.stack([s[2] for s in sets]))
    call(dev_sets, (tiles, totals), flags)
    torch.cuda.synchronize()
    assert int(flags[0]) == 0
    return tiles.cpu().numpy(), totals.cpu().numpy()


def rotated_sets(items, width, height, bw, bh):
    return [sp.fill(items[r:] + items[:r], width, height, bw, bh, 4) for r in (3, len(items) // 2)]


def test_reshrink_distortion_of_alpha_and_one_pixel_tiles(gpu, oracle):
    """pxz_reshrink_distortion_varied_device at 32x32: the archive's tiles and two sets of stored versions are all alpha and
    one-pixel patterns (other patterns at other stored sizes tile for tile); equal to the squared differences of the oracle's two
    expansions, added up per tile in int64"""
    lay = frame(32, 32, 4, ALL, NOT_OPAQUE_32)
    sets = rotated_sets(sp.items(32, 32, 4, ("pow2", "one pass", "odd"), NOT_OPAQUE_32), lay.W, lay.H, 32, 32)
    for xf, uf in ((LANCZOS3, LANCZOS3), (CATMULLROM, TRIANGLE)):
        exp = archive_sums(oracle, expected(oracle, "not opaque 32", lay, 32, 32, 4, xf), lay.W, lay.H, 32, 32, uf, sets)
        tiles, totals = archive_call(lambda dev, out, flags: gpu.reshrink_distortion_varied_device(
            [(lay.W, lay.H)], 4, 32, 32, xf, uf, *upload(lay.tw, lay.th, lay.slots), *dev, out=out, image_flags=flags), 2, len(lay.names), sets)
        assert gpu.decode_status() == 0
        bad = np.argwhere((tiles != exp).any(axis=2))
        assert bad.size == 0, f"filters {xf}/{uf}: " + ", ".join(f"set {k}: {sets[k][3][t]} over {lay.names[t]}" for k, t in bad[:8])
        assert (totals[:, 0] == exp.sum(axis=1)).all()


@pytest.mark.parametrize("src,dst", [((64, 64), (32, 32)), ((32, 32), (48, 20))])
def test_retile_distortion_of_alpha_and_one_pixel_tiles(gpu, oracle, src, dst):
    """pxz_retile_distortion_varied_device: the archive's tiles at the source block against two sets at the new block, all of them
    alpha and one-pixel patterns; equal to (oracle expansion at the source block - oracle expansion of the set at the new block)^2
    per tile of the new grid"""
    lay = frame(*src, 4, ALL, NOT_OPAQUE_64 if src == (64, 64) else NOT_OPAQUE_32)
    sets = rotated_sets(sp.items(*dst, 4, ("pow2", "one pass", "odd"), not_opaque(*dst)), lay.W, lay.H, *dst)
    T = len(sets[0][0])
    for xf, uf in ((LANCZOS3, LANCZOS3), (CATMULLROM, NEAREST)):
        exp = archive_sums(oracle, expected(oracle, ("not opaque", src), lay, *src, 4, xf), lay.W, lay.H, *dst, uf, sets)
        tiles, totals = archive_call(lambda dev, out, flags: gpu.retile_distortion_varied_device(
            [(lay.W, lay.H)], 4, *src, *dst, xf, uf, *upload(lay.tw, lay.th, lay.slots), *dev, out=out, image_flags=flags), 2, T, sets)
        assert gpu.decode_status() == 0
        bad = np.argwhere((tiles != exp).any(axis=2))
        assert bad.size == 0, f"{src} -> {dst} filters {xf}/{uf}: " + ", ".join(f"set {k}: {sets[k][3][t]} (tile {t})" for k, t in bad[:8])
        assert (totals[:, 0] == exp.sum(axis=1)).all()
