"""The stored-tile patterns of tests/stored_patterns.py against the oracle and the numpy model of test_value_domain_host.py alone
(no GPU, no product code): on the way UP -- stored size to full tile -- the oracle's resize equals the model byte for byte, the
0/255 tiles drive every pass that runs above 255 and below 0 before its clamp (and never with the non-negative filters or over a
side of 1), the alpha tiles hand un-premultiply colours above their alpha and alpha 0, the one-pixel tiles give expanded tiles that
are opaque in some pixels and not in others, and a stored side of 1 always gives the single full-weight tap the kernels' one-row
shortcuts test for.  What tests/test_gpu_expand_domain.py compares the expand kernels with is thereby pinned on these inputs.

Which alpha pattern saturates on which stored pair depends on rounding (alpha 1..3 leaves sums of a few units), so it is recorded
per pattern and pair in tests/golden/expand_domain_alpha.json and asserted from there; the rules that do not depend on rounding
are asserted as rules.  `python tests/test_expand_domain_host.py` writes the record again."""
import json
import os

import numpy as np
import pytest

import stored_patterns as sp
from test_value_domain_host import clip8, h_pass, make_weights, model_before_division, model_resize, premultiply, v_pass

BLOCKS = [(16, 16), (32, 32), (64, 64), (48, 20), (24, 24)]
NEAREST, TRIANGLE, CATMULLROM, GAUSSIAN, LANCZOS3 = range(5)
CONVOLUTIONS = (TRIANGLE, CATMULLROM, GAUSSIAN, LANCZOS3)
NEGATIVE_LOBES = (CATMULLROM, LANCZOS3)
RECORD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "expand_domain_alpha.json")


_weights = {}


def weights_of(oracle):
    """the model's integer weight matrices, from the oracle's fir_coeffs: built once (no fixture: conftest.py has the only ones)"""
    if "w" not in _weights:
        _weights["w"] = make_weights(oracle)
    return _weights["w"]


# ---- the helper itself -------------------------------------------------------------------------------------------------------------

def test_patterns_hold_the_values_they_name():
    for tw, th in ((1, 1), (2, 1), (1, 2), (2, 2), (8, 1), (1, 16), (3, 8), (16, 16), (31, 16), (64, 32)):
        p = {n: sp.stored(n, tw, th, 4) for n in sp.names(tw, th, 4)}
        assert list(p) == list(sp.OPAQUE + sp.ALPHA + sp.one_pixel_names(tw, th))
        for n in sp.OPAQUE:
            t3 = sp.stored(n, tw, th, 3)
            assert p[n].shape == (th, tw, 4) and p[n].dtype == np.uint8 and (p[n] == sp.stored(n, tw, th, 4)).all()
            assert (p[n][..., 3] == 255).all() and (p[n][..., :3] == t3).all() and np.isin(t3, (0, 255)).all(), n
        assert (p["flat 0"][..., :3] == 0).all() and (p["flat 255"] == 255).all()
        assert int((p["white pixel"][..., 0] == 255).sum()) == 1 and int((p["black pixel"][..., 0] == 0).sum()) == 1
        for n in sp.ALPHA + sp.one_pixel_names(tw, th):
            assert np.isin(p[n][..., :3], (0, 255)).all(), n
        assert set(np.unique(p["alpha 1..3"][..., 3])) <= {1, 2, 3}
        assert set(np.unique(p["alpha extremes"][..., 3])) <= {0, 1, 2, 127, 128, 254, 255}
        if tw * th >= 64:
            assert set(np.unique(p["alpha 1..3"][..., 3])) == {1, 2, 3}
            assert set(np.unique(p["alpha extremes"][..., 3])) == {0, 1, 2, 127, 128, 254, 255}
        y, x = np.mgrid[0:th, 0:tw]
        odd = ((x + y) & 1) == 1
        assert (p["alpha checker 0/255"][..., 3] == np.where(odd, 255, 0)).all()
        assert (p["alpha checker 254/255"][..., 3] == np.where(odd, 255, 254)).all()
        assert (p["alpha v stripes 3/255"][..., 3] == np.where((x & 1) == 1, 3, 255)).all()
        assert (p["alpha h stripes 3/255"][..., 3] == np.where((y & 1) == 1, 3, 255)).all()
        # (the stripes vanish on a tile one pixel across them: opaque)
        assert tw > 1 or (p["alpha v stripes 3/255"][..., 3] == 255).all()
        assert th > 1 or (p["alpha h stripes 3/255"][..., 3] == 255).all()
        assert (p["white alpha 1"] == np.array([255, 255, 255, 1], np.uint8)).all()
        assert (p["white alpha 0"] == np.array([255, 255, 255, 0], np.uint8)).all()
        for n in sp.one_pixel_names(tw, th):
            kind, at = n.split(" @")
            a = p[n][..., 3].ravel()
            rest, own = {"one 254": (255, 254), "one 0": (255, 0), "lone opaque": (0, 255)}[kind]
            assert a[int(at)] == own and (np.delete(a, int(at)) == rest).all(), n
            assert (sp.opaque_twin(p[n])[..., 3] == 255).all() and (sp.opaque_twin(p[n])[..., :3] == p[n][..., :3]).all()


def test_one_pixel_tiles_sit_either_side_of_a_staging_round():
    assert sp.gate_indices(1) == [0] and sp.gate_indices(2) == [0, 1] and sp.gate_indices(64) == [0, 63]
    assert sp.gate_indices(65) == [0, 63, 64] and sp.gate_indices(128) == [0, 63, 64, 127]
    assert sp.gate_indices(256) == [0, 63, 64, 157, 255] and sp.gate_indices(512) == [0, 63, 64, 285, 511]
    for n in (256, 512, 1024, 2048):
        mid = sp.gate_indices(n)[3]
        assert mid // 64 >= 2 and 0 < mid % 64 < 63 and mid < n - 1


@pytest.mark.parametrize("channels", [4, 3])
def test_layout_puts_every_item_in_a_full_tile_and_clips_the_ragged_ones(channels):
    for bw, bh in BLOCKS:
        items = sp.items(bw, bh, channels)
        assert {(tw, th) for _, tw, th in items} == set(sp.all_pairs(bw, bh))
        for tw, th in sp.all_pairs(bw, bh):
            assert [n for n, w, h in items if (w, h) == (tw, th)] == list(sp.names(tw, th, channels))
        W, H, tile_w, tile_h, slots, names = sp.layout(items, bw, bh, channels)
        cols, rows = -(-W // bw), -(-H // bh)
        assert W % bw == 7 and H % bh == 5 and len(names) == cols * rows == len(tile_w) == len(tile_h) == len(slots)
        assert (cols - 1) * (rows - 1) >= len(items) and slots.shape[1] == bw * bh * channels
        full = [names[r * cols + c] for r in range(rows - 1) for c in range(cols - 1)]
        assert full[: len(items)] == [f"{n} {tw}x{th}" for n, tw, th in items]
        for t, name in enumerate(names):
            r, c = divmod(t, cols)
            fw, fh = (7 if c == cols - 1 else bw), (5 if r == rows - 1 else bh)
            pattern, size = name.rsplit(" ", 1)
            tw, th = (int(v) for v in size.split("x"))
            assert (tw, th) == (tile_w[t], tile_h[t]) and 1 <= tw <= fw and 1 <= th <= fh
            assert (slots[t, : tw * th * channels] == sp.stored(pattern, tw, th, channels).ravel()).all()
            assert (slots[t, tw * th * channels:] == 0).all()


# ---- the oracle against the model, on the way up -----------------------------------------------------------------------------------

@pytest.mark.parametrize("bw,bh", BLOCKS)
@pytest.mark.parametrize("filt", CONVOLUTIONS)
def test_oracle_resize_equals_the_numpy_model_on_the_way_up(oracle, bw, bh, filt):
    """Every pattern, RGBA and RGB, from every stored pair the GPU module uses to the full tile: two passes, one pass across, one
    pass down, sides of 1, odd sizes, the clone."""
    weights = weights_of(oracle)
    for channels in (4, 3):
        for tw, th in sp.all_pairs(bw, bh):
            for name in sp.names(tw, th, channels):
                tile = sp.stored(name, tw, th, channels)
                got = oracle.resize(tile, bw, bh, filt)
                exp = model_resize(weights, tile, bw, bh, filt)
                assert (got == exp).all(), f"{tw}x{th} -> {bw}x{bh} c{channels} filter {filt} {name}: {int((got != exp).sum())} bytes differ"


@pytest.mark.parametrize("filt", CONVOLUTIONS)
def test_oracle_resize_equals_the_numpy_model_on_the_other_pairs_of_the_gpu_module(oracle, filt):
    """the one-row tiles of a 32x32 tile at the widths no level pair gives (31, 12, 3 beside the powers of two), and the 192x192
    tiles with the patterns they carry there"""
    weights = weights_of(oracle)
    for w in sp.ONE_ROW_WIDTHS:
        for name in sp.ALPHA + sp.one_pixel_names(w, 1):
            tile = sp.stored(name, w, 1, 4)
            assert (oracle.resize(tile, 32, 32, filt) == model_resize(weights, tile, 32, 32, filt)).all(), (w, name, filt)
    for tw, th in sp.all_pairs(192, 192):
        for name in sp.BIG_PATTERNS:
            if name in sp.names(tw, th, 4):
                tile = sp.stored(name, tw, th, 4)
                assert (oracle.resize(tile, 192, 192, filt) == model_resize(weights, tile, 192, 192, filt)).all(), (tw, th, name, filt)


# ---- the clamps fire ---------------------------------------------------------------------------------------------------------------

def passes(weights, tile, bw, bh, filt):
    """-> ({"h" | "v": (some sum below 0, some shifted sum above 255)} of the passes that run, the result before any division).
    Unclamped int64 sums; the vertical pass takes the CLAMPED horizontal result."""
    th, tw = tile.shape[:2]
    out, cur = {}, tile
    if tw != bw:
        acc, prec = h_pass(weights, cur, bw, filt)
        out["h"] = (bool((acc < 0).any()), bool(((acc >> prec) > 255).any()))
        cur = clip8(acc, prec)
    if th != bh:
        acc, prec = v_pass(weights, cur, bh, filt)
        out["v"] = (bool((acc < 0).any()), bool(((acc >> prec) > 255).any()))
        cur = clip8(acc, prec)
    return out, cur


@pytest.mark.parametrize("bw,bh", BLOCKS)
@pytest.mark.parametrize("filt", CONVOLUTIONS)
def test_which_passes_overshoot(oracle, bw, bh, filt):
    """CatmullRom and Lanczos3: on EVERY stored pair, every pass that runs over a stored side >= 2 goes both below 0 and above 255
    before its clamp, on the four tiles of sp.OVERSHOOT alone (checker, corner step, white pixel, black pixel).
    Pinned, not assumed: a pass over a stored side of 1 never overshoots with any pattern (one tap), and Triangle and Gaussian
    never overshoot anywhere (no negative weights); there the results still reach exactly 0 and exactly 255."""
    weights = weights_of(oracle)
    for tw, th in sp.all_pairs(bw, bh):
        if (tw, th) == (bw, bh):
            continue
        seen = {}
        lo = hi = False
        for name in sp.OPAQUE:
            ran, out = passes(weights, sp.stored(name, tw, th, 3), bw, bh, filt)
            lo, hi = lo or bool((out == 0).any()), hi or bool((out == 255).any())
            assert set(ran) == ({"h"} if tw != bw else set()) | ({"v"} if th != bh else set())
            for axis, (under, over) in ran.items():
                side = tw if axis == "h" else th
                if filt not in NEGATIVE_LOBES or side == 1:
                    assert not under and not over, f"{tw}x{th} -> {bw}x{bh} filter {filt} {name}: pass {axis} overshoots"
                elif name in sp.OVERSHOOT:
                    u, o = seen.get(axis, (False, False))
                    seen[axis] = (u or under, o or over)
        assert lo and hi, f"{tw}x{th} -> {bw}x{bh} filter {filt}: the results do not reach 0 and 255"
        if filt in NEGATIVE_LOBES:
            need = ({"h"} if tw != bw and tw >= 2 else set()) | ({"v"} if th != bh and th >= 2 else set())
            assert set(seen) == need and all(u and o for u, o in seen.values()), f"{tw}x{th} -> {bw}x{bh} filter {filt}: {seen}"


# ---- un-premultiply: colours above their alpha, alpha 0 -----------------------------------------------------------------------------

def alpha_facts(weights, bw, bh, filt):
    """{pattern: (per pair of sp.all_pairs but the clone: '1' where some premultiplied colour exceeds its alpha going into
    un-premultiply, '1' where some alpha going in is 0)} as strings"""
    out = {}
    for name in sp.ALPHA:
        sat, zero = "", ""
        for tw, th in sp.all_pairs(bw, bh):
            if (tw, th) == (bw, bh):
                continue
            tile = sp.stored(name, tw, th, 4)
            assert (premultiply(tile)[..., :3] <= tile[..., 3:4]).all()
            b = model_before_division(weights, tile, bw, bh, filt).astype(np.int32)
            sat += "01"[bool((b[..., :3] > b[..., 3:4]).any())]
            zero += "01"[bool((b[..., 3] == 0).any())]
        out[name] = (sat, zero)
    return out


def record_key(bw, bh, filt):
    return f"{bw}x{bh} filter {filt}"


@pytest.mark.parametrize("bw,bh", BLOCKS)
def test_what_unpremultiply_is_given(oracle, bw, bh):
    """Per alpha pattern, stored pair and filter: does un-premultiply get a colour above its alpha (its clamp to 255 decides the
    byte), does it get alpha 0 (reciprocal 0: the colour is dropped)?  Both as recorded, the "does not" cases included, and:
      * Triangle and Gaussian never give a colour above its alpha (no negative weights: colour <= alpha survives a pass);
      * no pattern does on a pair whose passes all run over a side of 1 (1x1, full x 1, 1 x full): one tap copies the pixel;
      * flat tiles (white at alpha 1, white at alpha 0) never do; white at alpha 0 gives alpha 0 everywhere, the 254/255 checker
        and white at alpha 1 never give alpha 0;
      * the column stripes are opaque on a 1 x n tile and the row stripes on an n x 1 tile: neither condition there;
      * with CatmullRom and Lanczos3 EVERY other pair is given a colour above its alpha by some pattern, and on every pair but
        1x1 the 254/255 checker or the extremes do it alone -- so each kernel text meets the clamp on each pair that can;
      * on the pairs 2x2, 4x4, 8x8, half x half, half x 1, 1 x half and full x half with Lanczos3: the column stripes 3/255
        (but on 1 x half) and the 254/255 checker give a colour above its alpha, the 0/255 checker and the column stripes
        alpha 0.  Alpha 1..3 does so on most of them, not on all: its sums are a few units, and whether a colour ends above its
        alpha is a matter of two roundings -- recorded per pair, like the rest."""
    weights = weights_of(oracle)
    with open(RECORD) as f:
        record = json.load(f)
    pairs = [p for p in sp.all_pairs(bw, bh) if p != (bw, bh)]
    copies = [k for k, (tw, th) in enumerate(pairs) if (tw in (1, bw)) and (th in (1, bh))]
    assert len(copies) == 3
    for filt in CONVOLUTIONS:
        facts = alpha_facts(weights, bw, bh, filt)
        assert {n: list(v) for n, v in facts.items()} == record[record_key(bw, bh, filt)], f"{bw}x{bh} filter {filt}"
        sat = {n: np.array([c == "1" for c in s]) for n, (s, _) in facts.items()}
        zero = {n: np.array([c == "1" for c in z]) for n, (_, z) in facts.items()}
        for n in sp.ALPHA:
            assert filt in NEGATIVE_LOBES or not sat[n].any(), (filt, n)
            assert not sat[n][copies].any(), (filt, n)
        assert not sat["white alpha 1"].any() and not sat["white alpha 0"].any()
        assert zero["white alpha 0"].all() and not zero["white alpha 1"].any() and not zero["alpha checker 254/255"].any()
        for k, (tw, th) in enumerate(pairs):
            assert tw > 1 or not (sat["alpha v stripes 3/255"][k] or zero["alpha v stripes 3/255"][k]), (filt, tw, th)
            assert th > 1 or not (sat["alpha h stripes 3/255"][k] or zero["alpha h stripes 3/255"][k]), (filt, tw, th)
        if filt in NEGATIVE_LOBES:
            union = np.any([sat[n] for n in sp.ALPHA], axis=0)
            assert [k for k in range(len(pairs)) if not union[k]] == copies, (filt, [pairs[k] for k in np.nonzero(~union)[0]])
            two = sat["alpha checker 254/255"] | sat["alpha extremes"]
            assert [k for k in range(len(pairs)) if not two[k]] == copies
        if filt == LANCZOS3 and bw == bh and bw in (16, 32, 64):
            half = bw // 2
            for tw, th in ((2, 2), (4, 4), (8, 8), (half, half), (half, 1), (1, half), (bw, half)):
                k = pairs.index((tw, th))
                assert sat["alpha checker 254/255"][k] and zero["alpha checker 0/255"][k], (tw, th)
                assert (sat["alpha v stripes 3/255"][k] or tw in (1, bw)) and (zero["alpha v stripes 3/255"][k] or tw in (1, bw)), (tw, th)


# ---- the gates: tiles with one pixel that differs -----------------------------------------------------------------------------------

@pytest.mark.parametrize("bw,bh", BLOCKS)
@pytest.mark.parametrize("filt", [NEAREST, TRIANGLE, CATMULLROM, GAUSSIAN, LANCZOS3])
def test_one_pixel_tiles_expand_to_opaque_and_other_pixels(oracle, bw, bh, filt):
    """"one 254" and "one 0" (opaque but for one stored pixel): the expanded tile holds pixels of alpha 255 AND pixels of another
    alpha, so that a wave-wide "nobody holds anything but 255" gate sees some lanes of each kind; the flat-opaque twin (the same
    colours at alpha 255) expands to alpha 255 everywhere.  What cannot be: a 1x1 tile is its one pixel (no alpha 255 is left),
    and the Gaussian spreads the transparent pixel of a two-pixel tile over every output (its window spans both).
    "lone opaque" (transparent but for one pixel), the mirror: alpha above 0 and alpha below 255 both come out; at 1x1 the tile
    is opaque."""
    for tw, th in sp.all_pairs(bw, bh):
        for name in sp.one_pixel_names(tw, th):
            tile = sp.stored(name, tw, th, 4)
            a = oracle.resize(tile, bw, bh, filt)[..., 3]
            what = f"{name} {tw}x{th} -> {bw}x{bh} filter {filt}"
            if name.startswith("lone opaque"):
                assert (a > 0).any() and ((a < 255).any() or tw * th == 1), what
                assert tw * th > 1 or (a == 255).all(), what
            else:
                assert (a != 255).any(), what
                none_left = tw * th == 1 or (filt == GAUSSIAN and name.startswith("one 0") and tw * th == 2)
                assert bool((a == 255).any()) != none_left, what
            assert (oracle.resize(sp.opaque_twin(tile), bw, bh, filt)[..., 3] == 255).all(), what


# ---- the one-row shortcuts ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("filt", CONVOLUTIONS)
def test_a_stored_side_of_1_is_one_full_weight_tap(oracle, filt):
    """expand_tile_mfma (the table's "copied" word) and the general form (`one_row`) skip the vertical product of a stored height of
    1 when every window of the way up is that row with the single weight 2^precision.  fir_coeffs gives exactly that for 1 -> n
    with every convolution filter and every full side the suites use -- so no stored pair with a side of 1 takes the long way, and
    the GPU module has none to offer: every n x 1 tile there goes through the shortcut."""
    for n in (16, 20, 24, 32, 48, 64, 192, 5, 7):
        starts, sizes, k, prec = oracle.fir_coeffs(1, n, filt)
        assert (starts == 0).all() and (sizes == 1).all() and (k[:, 0] == (1 << prec)).all() and prec < 15, (n, filt)


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from oracle import binding
    binding.build()
    w = make_weights(binding)
    rec = {record_key(bw, bh, f): {n: list(v) for n, v in alpha_facts(w, bw, bh, f).items()} for bw, bh in BLOCKS for f in CONVOLUTIONS}
    with open(RECORD, "w") as out:
        json.dump(rec, out, indent=0, sort_keys=True)
        out.write("\n")
