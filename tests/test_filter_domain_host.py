"""The frames of tests/filter_patterns.py against the oracle alone (no GPU, no product code): the Python model of process() and of
the tree::process recursion equals oracle.process_image / oracle.tree_process_image on every frame, filter pair and threshold
tests/test_gpu_filter_domain.py uses, and the model's census shows what those inputs drive: every reduction from "unchanged"
down to 1x1 on a full tile of process(), every level of the recursion with pixelised, split and kept rectangles, pixelised
rectangles of alpha <= 3 below level 0 and of one pixel's width, and -- per geometry, filter pair and reduction -- which of the
resample passes leave 0..255 before their clamp and where un-premultiply is handed a colour above its alpha, on the way down and
on the way up.  The part of the latter that is required is asserted as a rule; everything is pinned as measured in
tests/golden/filter_domain.json (`python tests/test_filter_domain_host.py` writes the record again)."""
import json
import os

import numpy as np
import pytest

import filter_patterns as fp
import value_patterns as vp
from test_expand_domain_host import passes, weights_of
from test_value_domain_host import model_before_division, model_resize, premultiply

NEAREST, TRIANGLE, CATMULLROM, GAUSSIAN, LANCZOS3 = range(5)
NEGATIVE_LOBES = (CATMULLROM, LANCZOS3)
RECORD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "filter_domain.json")
# every full-tile geometry of the GPU module: process() blocks and the tree's level-0 blocks ("pixelise everything" is process())
GEOMETRIES = ((16, 16, False), (32, 32, False), (64, 64, False), (20, 12, False), (64, 32, False), (50, 50, False), (37, 61, False),
              (100, 36, False), (128, 128, True))


def classes(bw, bh):
    """the reductions of a full tile, level by level: unchanged, half, ... 1x1"""
    ws, hs = vp.sides(bw), vp.sides(bh)
    return [(ws[min(l, len(ws) - 1)], hs[min(l, len(hs) - 1)]) for l in range(max(len(ws), len(hs)))]


# ---- the helper itself -------------------------------------------------------------------------------------------------------------

def test_sparse_tiles_hold_the_values_they_name():
    for bw, bh in ((16, 16), (32, 32), (50, 50), (37, 61), (20, 12)):
        for kind, (fg, bg) in fp.KINDS.items():
            for per in fp.PERS:
                t, m = fp.sparse(bw, bh, per, kind, 4), fp.sparse_mask(bw, bh, per, kind)
                assert t.shape == (bh, bw, 4) and t.dtype == np.uint8 and (t == fp.sparse(bw, bh, per, kind, 4)).all()
                assert (t[~m] == np.array(bg, np.uint8)).all()
                if fg is not None:
                    assert (t[m] == np.array(fg, np.uint8)).all()
                else:
                    assert (t[m][:, 3] == 255).all() and np.isin(t[m][:, :3], (0, 255)).all() and (m.sum() < 16 or len(np.unique(t[m], axis=0)) > 2)
                if bw * bh >= 1024:
                    assert 0.5 / per < m.mean() < 2.0 / per, (bw, bh, kind, per)
                if kind in fp.OPAQUE_KINDS:
                    assert (fp.sparse(bw, bh, per, kind, 3) == t[..., :3]).all()
        assert list(fp.tiles(bw, bh, 4)) == fp.sparse_names(4) + list(vp.OPAQUE + vp.ALPHA)
        assert list(fp.tiles(bw, bh, 3)) == fp.sparse_names(3) + list(vp.OPAQUE)


@pytest.mark.parametrize("channels", [4, 3])
def test_frame_lays_every_tile_out_with_the_edge_it_is_given(channels):
    for bw, bh in ((16, 16), (37, 61), (20, 12)):
        every = fp.tiles(bw, bh, channels)
        for edge in fp.EDGES:
            for names in (None, fp.subset(channels)):
                frames, (n0, n1) = fp.batch(bw, bh, channels, edge, names)
                _, H, W, C = frames.shape
                want = list(every) if names is None else names
                cols, rows = -(-W // bw), -(-H // bh)
                assert C == channels and W % bw == edge[0] and H % bh == edge[1] and cols <= 9 and rows <= 9
                assert len(n0) == len(n1) == cols * rows
                for img, tile_names, rot in ((frames[0], n0, 0), (frames[1], n1, 1)):
                    full = vp.full_tiles(img, bw, bh)
                    assert [n for n, f in zip(tile_names, full) if f][: len(want)] == want[rot:] + want[:rot]
                    for t, name in enumerate(tile_names):
                        r, c = divmod(t, cols)
                        part = img[r * bh:(r + 1) * bh, c * bw:(c + 1) * bw]
                        assert part.shape[:2] == ((bh if r < rows - 1 else edge[1]), (bw if c < cols - 1 else edge[0]))
                        assert (part == every[name][: part.shape[0], : part.shape[1]]).all(), (bw, bh, edge, t, name)


# ---- process(): the model, and which reductions occur --------------------------------------------------------------------------------

@pytest.mark.parametrize("bw,bh,edge,sub", fp.PROCESS_CASES)
def test_process_model_equals_the_oracle_and_walks_every_reduction(oracle, bw, bh, edge, sub):
    """Equality on both frames, RGBA and RGB, every filter pair.  Then, from the census of the full tiles of frame 0:
      * the opaque sparse kinds are pixelised at each of the five levels below "unchanged" (half ... 1 / 32, or down to 1x1);
      * the low-alpha tiles -- the alpha kinds of the sparse family and the alpha tiles of value_patterns -- at
        "unchanged" and each of those five levels;
      * all tiles together at every level there is, 1x1 included.
    The subset of the 128-px case holds one opaque kind and a few alpha tiles: all tiles together reach "unchanged" and the
    five levels below."""
    for channels in (4, 3):
        frames, names = fp.case_batch(bw, bh, channels, edge, sub)
        for n in range(2):
            memo = {}
            for down, up in fp.FILTER_PAIRS:
                got, census = fp.process(oracle, frames[n], bw, bh, down, up, memo)
                assert (got == oracle.process_image(frames[n], bw, bh, down, up)).all(), (channels, n, down, up)
        _, census = fp.process(oracle, frames[0], bw, bh, 4, 0)
        cols = -(-frames.shape[2] // bw)
        seen = {}
        for _, _, x, y, w, h, nw, nh in census:
            if (w, h) == (bw, bh):
                seen.setdefault(names[0][(y // bh) * cols + x // bw], set()).add((nw, nh))
        cl = classes(bw, bh)
        of = lambda pick: set().union(*[s for name, s in seen.items() if pick(name)])
        opaque = of(lambda name: name.startswith("sparse") and name.endswith(fp.OPAQUE_KINDS))
        everything = of(lambda name: True)
        if sub:
            need = set(cl[0:6] if channels == 4 else cl[1:6])   # (no opaque tile stays unchanged: a deviation of 0.5 at the most)
            assert need <= everything, (channels, sorted(need - everything))
            continue
        assert set(cl[1:6]) <= opaque, (channels, sorted(set(cl[1:6]) - opaque))
        assert everything == set(cl) if channels == 4 else everything == set(cl[1:]), (channels, sorted(set(cl) ^ everything))
        if channels == 4:
            low = of(lambda name: name.endswith(fp.ALPHA_KINDS) or name in vp.ALPHA)
            assert set(cl[0:6]) <= low, sorted(set(cl[0:6]) - low)


# ---- tree::process: the model, and what the thresholds drive ---------------------------------------------------------------------------

def tree_runs(oracle, case, channels, pairs=fp.FILTER_PAIRS):
    """the model against the oracle on both frames, every pair and threshold -> {(frame, threshold): (image, census)} of pairs[0]"""
    bw, bh, mw, mh, edge, sub = case
    frames, _ = fp.case_batch(bw, bh, channels, edge, sub)
    out = {}
    memos = [{}, {}]
    for down, up in pairs:
        exp = fp.tree_references(oracle, frames, bw, bh, mw, mh, down, up)
        for n in range(2):
            for thr in fp.THRESHOLDS:
                got, census = fp.tree_process(oracle, frames[n], bw, bh, thr, mw, mh, down, up, memos[n])
                assert (got == exp[n, thr]).all(), (case, channels, n, down, up, thr)
                if (down, up) == pairs[0]:
                    out[n, thr] = (got, census)
    return out


@pytest.mark.parametrize("case", fp.TREE_GRID_CASES + fp.TREE_RECT_CASES)
def test_tree_model_equals_the_oracle_and_reaches_every_level(oracle, case):
    """Equality on both frames, RGBA and RGB, every filter pair and threshold.  Then, over the thresholds, from frame 0:
      * every level of the recursion has a pixelised and a split rectangle, and the level below the last a kept one;
      * RGBA: some rectangle pixelised below level 0 holds pixels of alpha <= 3;
      * 50x50 down to the 4x4 minimum (50 -> 25 -> 12 + 12 + 1): some pixelised rectangle is 1 px wide;
      * the negative threshold gives another image than its positive twin;
      * only 0.0 gives the source back and only 50.0 the image of process()."""
    bw, bh, mw, mh, edge, sub = case
    levels = 0
    while (bw >> levels) > max(mw, 4) and (bh >> levels) > max(mh, 4):
        levels += 1
    assert levels >= 2
    for channels in (4, 3):
        frames, _ = fp.case_batch(bw, bh, channels, edge, sub)
        runs = tree_runs(oracle, case, channels)
        what = set()
        low_alpha = narrow = False
        for thr in fp.THRESHOLDS:
            for level, kind, x, y, w, h, nw, nh in runs[0, thr][1]:
                what.add((level, kind))
                if kind == "pixelised":
                    narrow |= w == 1
                    low_alpha |= level > 0 and channels == 4 and bool((frames[0][y:y + h, x:x + w, 3] <= 3).any())
        need = {(l, k) for l in range(levels) for k in ("pixelised", "split")} | {(levels, "kept")}
        assert what == need, (channels, sorted(need ^ what))
        assert low_alpha or channels == 3
        assert narrow or (bw, bh, mw, mh) != (50, 50, 4, 4)
        assert -0.16 in fp.THRESHOLDS and 0.16 in fp.THRESHOLDS
        for n in range(2):
            assert (runs[n, -0.16][0] != runs[n, 0.16][0]).any()
            src = fp.rgba(frames[n])
            flat = oracle.process_image(frames[n], bw, bh, *fp.FILTER_PAIRS[0])
            for thr in fp.THRESHOLDS:
                assert bool((runs[n, thr][0] == src).all()) == (thr == 0.0), (channels, n, thr)
                assert bool((runs[n, thr][0] == flat).all()) == (thr == 50.0), (channels, n, thr)


# ---- the clamps and the reciprocal --------------------------------------------------------------------------------------------------

FLAGS = ("down h under", "down h over", "down v under", "down v over", "down colour above alpha",
         "up h under", "up h over", "up v under", "up v over", "up colour above alpha")


def one_way(oracle, weights, tile, nw, nh, filt):
    """-> ([h under, h over, v under, v over, colour above alpha going into un-premultiply], the resized tile)"""
    if filt == NEAREST or (nw, nh) == (tile.shape[1], tile.shape[0]):
        return [False] * 5, oracle.resize(tile, nw, nh, filt)
    ran, _ = passes(weights, premultiply(tile), nw, nh, filt)
    b = model_before_division(weights, tile, nw, nh, filt).astype(np.int32)
    out = model_resize(weights, tile, nw, nh, filt)
    assert (out == oracle.resize(tile, nw, nh, filt)).all()
    return list(ran.get("h", (False, False))) + list(ran.get("v", (False, False))) + [bool((b[..., :3] > b[..., 3:4]).any())], out


def facts(oracle, bw, bh, sub, down, up):
    """{"nw x nh": one '0' / '1' per entry of FLAGS}: over the full RGBA tiles of the geometry that process() reduces to nw x nh"""
    weights = weights_of(oracle)
    every = fp.tiles(bw, bh, 4)
    out = {}
    for name in (fp.subset(4) if sub else every):
        tile = every[name]
        v = oracle.lod_oklab_identity(tile)
        nw, nh, _ = oracle.reduce_dims(v, v, bw, bh)
        if (nw, nh) == (bw, bh):
            continue
        d, small = one_way(oracle, weights, tile, nw, nh, down)
        u, _ = one_way(oracle, weights, small, bw, bh, up)
        have = out.setdefault(f"{nw}x{nh}", [False] * 10)
        out[f"{nw}x{nh}"] = [a or b for a, b in zip(have, d + u)]
    return {k: "".join("01"[f] for f in v) for k, v in out.items()}


def record_key(bw, bh, down, up):
    return f"{bw}x{bh} down {down} up {up}"


@pytest.mark.parametrize("bw,bh,sub", GEOMETRIES)
def test_which_passes_overshoot_and_where_unpremultiply_saturates(oracle, bw, bh, sub):
    """Per filter pair and reduction, over the full RGBA tiles: does the horizontal / vertical pass of the way down and of the
    way up go below 0 and above 255 before its clamp, is un-premultiply handed a colour above its alpha -- all as recorded, the
    "does not" cases included.  The rules:
      * Nearest, Triangle and Gaussian never overshoot and never hand a colour above its alpha (no negative weights);
      * CatmullRom and Lanczos3 at half size: both passes of their way overshoot both ways;
      * CatmullRom and Lanczos3: on their way, un-premultiply saturates on some reduction."""
    with open(RECORD) as f:
        record = json.load(f)
    half = "%dx%d" % classes(bw, bh)[1]
    for down, up in fp.FILTER_PAIRS:
        got = facts(oracle, bw, bh, sub, down, up)
        assert got == record[record_key(bw, bh, down, up)], (bw, bh, down, up)
        for filt, first in ((down, 0), (up, 5)):
            way = {k: v[first:first + 5] for k, v in got.items()}
            if filt not in NEGATIVE_LOBES:
                assert all(v == "00000" for v in way.values()), (bw, bh, down, up, way)
                continue
            assert way[half][:4] == "1111", f"{bw}x{bh} filter {filt} {'down' if first == 0 else 'up'} at {half}: {way[half]}"
            assert any(v[4] == "1" for v in way.values()), f"{bw}x{bh} filter {filt} {'down' if first == 0 else 'up'}: no colour above its alpha"


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from oracle import binding
    binding.build()
    rec = {record_key(bw, bh, d, u): facts(binding, bw, bh, sub, d, u) for bw, bh, sub in GEOMETRIES for d, u in fp.FILTER_PAIRS}
    with open(RECORD, "w") as out:
        json.dump(rec, out, indent=0, sort_keys=True)
        out.write("\n")
