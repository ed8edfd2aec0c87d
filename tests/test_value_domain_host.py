"""The patterns of tests/value_patterns.py against the oracle alone (no GPU, no product code): they reach the stored sizes they
are meant to reach, they drive the resample's clamps and the un-premultiply's clamp, and on them the oracle's resize equals a
numpy restatement of fast_image_resize's u8 convolution byte for byte -- so that what tests/test_gpu_value_domain.py compares
the kernels with is itself pinned on these inputs."""
import functools

import numpy as np
import pytest

import value_patterns as vp

BLOCKS = [(16, 16), (32, 32), (64, 64), (48, 20), (24, 24)]
TRIANGLE, CATMULLROM, GAUSSIAN, LANCZOS3 = 1, 2, 3, 4


# ---- numpy restatement of orc_resize's convolution path (fir 4.2.1, U8x3 / U8x4 with the default premultiplication) -------------

def make_weights(oracle):
    @functools.lru_cache(maxsize=None)
    def weights(n_in, n_out, filt):
        """dense [n_out, n_in] int64 matrix of the integer weights, and their precision"""
        starts, sizes, k, prec = oracle.fir_coeffs(n_in, n_out, filt)
        K = np.zeros((n_out, n_in), np.int64)
        for o in range(n_out):
            K[o, starts[o]:starts[o] + sizes[o]] = k[o, :sizes[o]]
        return K, prec
    return weights


def h_pass(weights, img, nw, filt):
    """unclamped int64 sums of the horizontal pass (rounding constant included), and the precision"""
    K, prec = weights(img.shape[1], nw, filt)
    return np.einsum("oi,yic->yoc", K, img.astype(np.int64)) + (1 << (prec - 1)), prec


def v_pass(weights, img, nh, filt):
    K, prec = weights(img.shape[0], nh, filt)
    return np.einsum("oi,ixc->oxc", K, img.astype(np.int64)) + (1 << (prec - 1)), prec


def clip8(acc, prec):
    return np.clip(acc >> prec, 0, 255).astype(np.uint8)


def premultiply(tile):
    """mul_div_255 of every colour byte with its alpha"""
    t = tile[..., :3].astype(np.uint32) * tile[..., 3:4].astype(np.uint32) + 128
    out = tile.copy()
    out[..., :3] = ((t >> 8) + t) >> 8
    return out


def unpremultiply(tile):
    """the reciprocal table (precision 8, rounded; 0 for alpha 0), multiply, round, clamp"""
    a = tile[..., 3:4].astype(np.uint32)
    recip = np.where(a == 0, 0, ((255 * 512) // np.maximum(a, 1) + 1) >> 1)
    out = tile.copy()
    out[..., :3] = np.minimum((tile[..., :3].astype(np.uint32) * recip + 128) >> 8, 255)
    return out


def model_before_division(weights, tile, nw, nh, filt):
    """premultiply, horizontal pass, clamp, vertical pass, clamp: what `unpremultiply` is given"""
    cur = premultiply(tile) if tile.shape[2] == 4 else tile
    if nw != tile.shape[1]:
        cur = clip8(*h_pass(weights, cur, nw, filt))
    if nh != tile.shape[0]:
        cur = clip8(*v_pass(weights, cur, nh, filt))
    return cur


def model_resize(weights, tile, nw, nh, filt):
    if (nw, nh) == (tile.shape[1], tile.shape[0]):
        return tile.copy()
    out = model_before_division(weights, tile, nw, nh, filt)
    return unpremultiply(out) if tile.shape[2] == 4 else out


@pytest.fixture(scope="module")
def weights(oracle):
    return make_weights(oracle)


# ---- the helper itself -------------------------------------------------------------------------------------------------------------

def test_patterns_hold_the_values_they_name():
    for bw, bh in BLOCKS:
        rgba, rgb = vp.patterns(bw, bh, 4), vp.patterns(bw, bh, 3)
        assert [n for n, _ in rgba] == list(vp.OPAQUE + vp.ALPHA) and [n for n, _ in rgb] == list(vp.OPAQUE)
        again = dict(vp.patterns(bw, bh, 4))
        for (name, t), (_, t3) in zip(rgba, rgb):
            assert t.shape == (bh, bw, 4) and t.dtype == np.uint8 and (t == again[name]).all()
            assert (t[..., 3] == 255).all() and (t[..., :3] == t3).all(), name
        p = dict(rgba)
        for name in vp.OPAQUE:
            lo, hi = (0, 255) if "dither" not in name else (vp.DITHER, 255 - vp.DITHER)
            assert ((p[name][..., :3] <= lo) | (p[name][..., :3] >= hi)).all() and p[name].min() == 0 and p[name].max() == 255, name
        for name in vp.DITHERED:
            assert len(np.unique(p[name][..., :3])) == 2 * (vp.DITHER + 1), name
        for name in vp.ALPHA:
            assert np.isin(p[name][..., :3], (0, 255)).all(), name
        assert set(np.unique(p["noise"])) == {0, 255} and len({p["noise"][..., k].tobytes() for k in range(3)}) == 3
        assert set(np.unique(p["alpha 1..3"][..., 3])) == {1, 2, 3}
        assert set(np.unique(p["alpha extremes"][..., 3])) == {0, 1, 2, 127, 128, 254, 255}
        assert set(np.unique(p["alpha checker 0/255"][..., 3])) == {0, 255}
        assert set(np.unique(p["alpha checker 254/255"][..., 3])) == {254, 255}
        across, down = p["alpha ramp across"][..., 3], p["alpha ramp down"][..., 3]
        assert (across[0, 0], across[0, -1], down[0, 0], down[-1, 0]) == (0, 255, 1, 255)
        assert (np.diff(across.astype(int), axis=1) >= 0).all() and (np.diff(down.astype(int), axis=0) >= 0).all()
        assert (across == across[:1]).all() and (down == down[:, :1]).all()
        assert int((p["opaque pixel"][..., 3] == 255).sum()) == 1 and int((p["opaque pixel"][..., 3] == 0).sum()) == bw * bh - 1
        assert int((p["transparent pixel"][..., 3] == 0).sum()) == 1 and int((p["transparent pixel"][..., 3] == 255).sum()) == bw * bh - 1
        s = p["stripes alpha 3/255"]
        assert ((s[..., 3] == 3) == (s[..., 0] == 255)).all() and ((s[..., 3] == 255) == (s[..., 0] == 0)).all()
        assert (p["white alpha 1"] == np.array([255, 255, 255, 1], np.uint8)).all()


@pytest.mark.parametrize("channels", [4, 3])
def test_frame_lays_every_pattern_out_and_cuts_the_ragged_edge_from_them(channels):
    for bw, bh in BLOCKS:
        every = dict(vp.patterns(bw, bh, channels))
        for names in (None, vp.ALPHA if channels == 4 else vp.OPAQUE[:5], vp.interleave(vp.OPAQUE, vp.OPAQUE[::-1])):
            img, tile_names = vp.frame(bw, bh, channels, names)
            H, W, C = img.shape
            assert C == channels and W % bw == 7 and H % bh == 5 and img.flags["C_CONTIGUOUS"]
            cols, rows = -(-W // bw), -(-H // bh)
            full = vp.full_tiles(img, bw, bh)
            assert len(tile_names) == cols * rows == len(full)
            assert {n for n, f in zip(tile_names, full) if f} == set(every if names is None else names)
            for t, name in enumerate(tile_names):
                r, c = divmod(t, cols)
                part = img[r * bh:(r + 1) * bh, c * bw:(c + 1) * bw]
                assert part.shape[:2] == ((bh if r < rows - 1 else 5), (bw if c < cols - 1 else 7))
                assert full[t] == (part.shape[:2] == (bh, bw))
                assert (part == every[name][: part.shape[0], : part.shape[1]]).all(), (bw, bh, t, name)


def test_factors_keep_one_factor_per_decision(oracle):
    for (bw, bh), mode in (((32, 32), 0), ((32, 32), 1), ((48, 20), 1)):
        img, _ = vp.frame(bw, bh, 4)
        kept = vp.factors(oracle, img, bw, bh, mode)
        assert 2 <= len(kept) <= len(vp.WALK) and all(k in vp.WALK for k in kept)
        sizes = lambda k: tuple(a.tobytes() for a in oracle.shrink_image(img, bw, bh, mode, 4, k, want_pixels=False)[1:3])
        assert len({sizes(k) for k in kept}) == len(kept)
        assert {sizes(k) for k in kept} == {sizes(k) for k in vp.WALK}


# ---- coverage: which stored sizes a pattern reaches --------------------------------------------------------------------------------

def classes_of(oracle, tile, bw, bh, mode):
    tile = np.ascontiguousarray(tile)
    out = set()
    for k in vp.WALK:
        _, ow, oh, _ = oracle.shrink_image(tile, bw, bh, mode, LANCZOS3, k, want_pixels=False)
        out.add((int(ow[0]), int(oh[0])))
    return out


@pytest.mark.parametrize("bw,bh", BLOCKS)
@pytest.mark.parametrize("mode", [0, 1])
def test_every_pattern_reaches_its_classes(oracle, bw, bh, mode):
    """Mode 0: every pattern but the flat one is stored at every square class from 1x1 to the full tile, and at nothing else.
    Mode 1: period 2 is flat to the 3x3 Sobel windows (1x1 only); stripes, steps and the alpha tiles over them keep one side
    at 1 and reach every size of the other; the dithered stripes also reach every one-pass class (one side full, the other
    2, 4, 8, ...); blocks, the corner and the single pixels stay square.  RGB tiles decide as their RGBA twins do."""
    for channels in (4, 3):
        for name, tile in vp.patterns(bw, bh, channels):
            need, only = vp.required_classes(name, bw, bh, mode)
            got = classes_of(oracle, tile, bw, bh, mode)
            assert need <= got, f"{bw}x{bh} c{channels} mode {mode} {name}: never stored at {sorted(need - got)}"
            assert not only or got == need, f"{bw}x{bh} c{channels} mode {mode} {name}: also stored at {sorted(got - need)}"
    if mode == 1:
        for name in vp.DITHERED:
            need, _ = vp.required_classes(name, bw, bh, 1)
            one_pass = {k for k in need if (k[0] == bw) != (k[1] == bh) and min(k) > 1}
            assert len(one_pass) >= 3, (name, sorted(one_pass))


def test_pattern_frames_reach_the_same_classes_tile_by_tile(oracle):
    """what the GPU suite asserts from its results, on the oracle: over factors() every full tile of a frame is stored at its
    pattern's classes (the deduplication drops no decision)"""
    for bw, bh, channels, mode in ((32, 32, 4, 1), (16, 16, 3, 0), (48, 20, 4, 1)):
        img, tile_names = vp.frame(bw, bh, channels)
        full = vp.full_tiles(img, bw, bh)
        seen = {}
        for k in vp.factors(oracle, img, bw, bh, mode):
            _, ow, oh, _ = oracle.shrink_image(img, bw, bh, mode, LANCZOS3, k, want_pixels=False)
            for name, cl in vp.classes_by_pattern(tile_names, ow, oh, full).items():
                seen.setdefault(name, set()).update(cl)
        for name in set(tile_names):
            need, only = vp.required_classes(name, bw, bh, mode)
            assert need <= seen[name] and (not only or need == seen[name]), (bw, bh, channels, mode, name)


# ---- the clamps fire ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("filt", [LANCZOS3, CATMULLROM])
@pytest.mark.parametrize("n", [16, 8, 4])
def test_both_passes_overshoot_on_both_sides(weights, filt, n):
    """32 -> n with the two filters that have negative lobes, integer weights, int64, nothing clamped.  `over` means that the
    shifted sum exceeds 255, i.e. that the sum exceeds 255 << precision by more than the rounding constant hides: the clamp
    decides the byte.
    First pass: a step overshoots on both sides at every n.  Stripes of period 6 ring at 32 -> 16, where the period is three
    output pixels (below 0 with both filters, above 255 with Lanczos3); at 8 and 4 a window spans whole periods and averages
    them, as it does with period 2 at every n: asserted too, so that nobody counts on them.  Tiles that vary down the tile are
    the transposed twins: their first pass leaves them as they are and the vertical pass meets the same edges.
    Second pass, over the clamped intermediate: the corner step overshoots again on both sides at every n, blocks of 3x3 and
    the noise at 32 -> 16 only (at 8 and 4 they average out: asserted too)."""
    p = {name: t[..., :3] for name, t in vp.patterns(32, 32, 4)}
    under = lambda acc: bool((acc < 0).any())
    over = lambda acc, prec: bool(((acc >> prec) > 255).any())
    for name in ("v step", "v stripes 6", "v stripes 2"):
        acc, prec = h_pass(weights, p[name], n, filt)
        twin = p[name.replace("v ", "h ")]
        assert (twin == p[name].transpose(1, 0, 2)).all()
        mid = clip8(*h_pass(weights, twin, n, filt))
        assert (mid == twin[:, :1]).all(), f"{name}: the first pass changes constant rows"
        acc_v, prec_v = v_pass(weights, mid, n, filt)
        assert (acc_v == acc[0][:, None, :]).all() and prec_v == prec  # (every row of acc is the same)
        if name == "v step":
            assert under(acc) and over(acc, prec), (name, n, filt)
        elif name == "v stripes 6" and n == 16:
            assert under(acc) and (over(acc, prec) or filt == CATMULLROM), (name, n, filt)
        else:
            assert not under(acc) and not over(acc, prec), (name, n, filt)
    for name in ("corner step", "blocks 3", "noise"):
        acc, prec = h_pass(weights, p[name], n, filt)
        first = under(acc) and over(acc, prec)
        acc2, prec2 = v_pass(weights, clip8(acc, prec), n, filt)
        second = under(acc2) and over(acc2, prec2)
        if name == "corner step" or n == 16:
            assert first and second, (name, n, filt, first, second)
        else:  # 3x3 blocks and the noise average out at 8 and 4: no second overshoot on either side, for blocks no first one
            assert not under(acc2) and not over(acc2, prec2), (name, n, filt)
            assert name == "noise" or (not under(acc) and not over(acc, prec)), (name, n, filt)
    # the single pixels: one side each, in both passes
    for name, below in (("white pixel", True), ("black pixel", False)):
        acc, prec = h_pass(weights, p[name], n, filt)
        assert (under(acc), over(acc, prec)) == (below, not below), (name, n, filt)


# ---- unpremultiply saturates -------------------------------------------------------------------------------------------------------

NEGATIVE_LOBES_MEET_ALPHA = ("alpha 1..3", "alpha extremes", "alpha checker 0/255", "alpha ramp across", "alpha ramp down",
                             "stripes alpha 3/255")


def test_unpremultiply_is_given_colours_above_their_alpha(weights):
    """32 -> 16 with Lanczos3, the tile before the division: a premultiplied colour never exceeds its alpha going in, but the
    negative lobes take more from a pixel's alpha than from its colour where its neighbours are transparent and dark by turns,
    so that colour > alpha comes out and the clamp of div_and_clip decides the byte.  Alpha 1..3 stays at 1..3 (the largest
    reciprocals); the 3/255 stripes ring down to alpha 0 with colour left over (reciprocal 0: the colour is dropped)."""
    p = dict(vp.patterns(32, 32, 4))
    for name in vp.ALPHA:
        assert (premultiply(p[name])[..., :3] <= p[name][..., 3:4]).all()
    before = {name: model_before_division(weights, p[name], 16, 16, LANCZOS3).astype(np.int32) for name in vp.ALPHA}
    for name in NEGATIVE_LOBES_MEET_ALPHA:
        b = before[name]
        sat = b[..., :3] > b[..., 3:4]
        assert sat.any(), name
        a = b[..., 3:4].astype(np.uint32)
        recip = np.where(a == 0, 0, ((255 * 512) // np.maximum(a, 1) + 1) >> 1)
        assert (((b[..., :3].astype(np.uint32) * recip + 128) >> 8)[sat & (a > 0)] > 255).any() or name == "stripes alpha 3/255", name
    for name in ("alpha 1..3", "white alpha 1"):
        assert np.isin(before[name][..., 3], (1, 2, 3)).all(), name
    b = before["opaque pixel"]
    assert np.isin(b[..., 3], (1, 2, 3)).any() and (b[..., 3] == 0).any()
    b = before["stripes alpha 3/255"]
    assert ((b[..., 3] == 0) & (b[..., :3].max(axis=2) > 0)).any()
    # CatmullRom has the lobes too; Triangle (Hamming) and Gaussian are non-negative: colour <= alpha + rounding survives
    assert any((model_before_division(weights, p[n], 16, 16, CATMULLROM)[..., :3].astype(int).max(axis=2) >
                model_before_division(weights, p[n], 16, 16, CATMULLROM)[..., 3]).any() for n in NEGATIVE_LOBES_MEET_ALPHA)


# ---- the oracle against the model --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bw,bh", [(16, 16), (32, 32), (48, 20), (64, 64)])
@pytest.mark.parametrize("filt", [TRIANGLE, CATMULLROM, GAUSSIAN, LANCZOS3])
def test_oracle_resize_equals_the_numpy_model(oracle, weights, bw, bh, filt):
    """Every pattern, RGBA and RGB, at every pair of stored sizes a level pair gives (two passes, one pass across, one pass
    down, the clone): orc_resize == premultiply, integer weights plus the rounding constant, a clamp after each pass,
    the reciprocal table rounded, multiply, round, clamp."""
    ws, hs = vp.sides(bw), vp.sides(bh)
    if bw == 64:
        ws, hs = [64, 32, 8, 1], [64, 16, 2, 1]   # (the largest tiles on a few pairs: the arithmetic does not depend on the size)
    for channels in (4, 3):
        for name, tile in vp.patterns(bw, bh, channels):
            for nw in ws:
                for nh in hs:
                    got = oracle.resize(tile, nw, nh, filt)
                    exp = model_resize(weights, tile, nw, nh, filt)
                    assert (got == exp).all(), f"{bw}x{bh} -> {nw}x{nh} c{channels} filter {filt} {name}: {int((got != exp).sum())} bytes differ"
