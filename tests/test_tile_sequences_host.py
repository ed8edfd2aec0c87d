"""What the frames of tile_sequences.py make the ORACLE do -- no GPU, no code under test.  The coverage the GPU module relies on
(every ordered pair of kinds at every stride, every shrink_by triple, exactly n listed tiles, whole and partial detector batches)
is asserted here from the oracle's stored sizes; the assertion is the condition the seeds were picked by.  For the detectors' alpha
sequences the kinds are the inputs themselves, and what is asserted on the oracle is that they BITE: a tile valued with alpha
bytes of the tile a period before it gets another value, bit for bit."""
import numpy as np
import pytest

import tile_sequences as ts

BLOCKS = (16, 32, 64)


@pytest.mark.parametrize("channels", [4, 3])
@pytest.mark.parametrize("block", BLOCKS)
def test_pair_frames_hold_every_ordered_pair_at_strides_1_to_8(oracle, block, channels):
    img, planned = ts.pair_frame(oracle, block, channels)
    cols = ts.PAIR_COLS
    assert img.shape == (ts.PAIR_ROWS * block, (cols - 1) * block + 7, channels) and cols > max(ts.STRIDES)
    seen_sizes = {}
    for filt in (ts.LANCZOS3, ts.NEAREST):  # (the detector decides the size: the filter must not matter)
        _, ow, oh, _ = oracle.shrink_image(img, block, block, ts.DIRECTIONAL, filt, ts.FACTOR, want_pixels=False)
        kinds = ts.kinds_of_frame(img, block, block, ow, oh)
        assert kinds == planned, [(t, a, b) for t, (a, b) in enumerate(zip(kinds, planned)) if a != b][:8]
        assert "other" not in kinds
        assert ts.missing_pairs(kinds, channels) == []
        seen_sizes[filt] = (ow.tobytes(), oh.tobytes())
        if block == 32:  # the classes of shrink32_kernel by name
            sizes = {(int(w), int(h)) for w, h, k in zip(ow, oh, kinds) if k == "sliver"}
            assert sizes and sizes <= {(16, 2), (16, 1)}, sizes
            narrow = {(int(w), int(h)) for w, h, k in zip(ow, oh, kinds) if k == "narrow"}
            assert narrow and all(w <= 4 and 1 < h <= 16 for w, h in narrow), narrow
            mid = {(int(w), int(h)) for w, h, k in zip(ow, oh, kinds) if k == "mid"}
            assert mid and all(4 <= w <= 16 and 4 <= h <= 16 for w, h in mid), mid
    assert seen_sizes[ts.LANCZOS3] == seen_sizes[ts.NEAREST]
    if channels == 4:  # an alpha tile has exactly one pixel that is not opaque, and it is 254
        a = img[..., 3]
        assert int((a != 255).sum()) == planned.count(ts.ALPHA) and set(np.unique(a).tolist()) == {254, 255}


def test_a_pair_is_reported_missing_when_it_is():
    """missing_pairs() on a sequence that lacks one pair at one stride"""
    kinds = ts.planned_pair_kinds(4, ts.PAIR_SEEDS[(32, 4)])
    assert ts.missing_pairs(kinds, 4) == []
    broken = ["one" if k == "whole" and kinds[t + 3:t + 4] == ["sliver"] else k for t, k in enumerate(kinds)]
    assert (3, "whole", "sliver") in ts.missing_pairs(broken, 4)


@pytest.mark.parametrize("channels", [4, 3])
@pytest.mark.parametrize("block", BLOCKS)
def test_triple_frames_hold_all_eight_triples_at_strides_1_to_8(oracle, block, channels):
    img, planned = ts.triple_frame(oracle, block, channels)
    assert img.shape == (ts.TRIPLE_ROWS * block, ts.TRIPLE_COLS * block, channels)
    _, ow, oh, _ = oracle.shrink_image(img, block, block, ts.SHRINK_BY, ts.LANCZOS3, ts.BY_FACTOR, want_pixels=False)
    kinds = ts.whole_or_reduced(ow, oh, block, block)
    assert kinds == planned
    assert ts.missing_triples(kinds) == []
    assert len({(int(w), int(h)) for w, h in zip(ow, oh)}) >= 4  # the reduced tiles are of several sizes
    # the noise tile is among the whole ones, a flat tile among the reduced ones
    whole, reduced = ts.by_pools(oracle, block, block, channels)
    assert any((t[..., :3] == t[0, 0, :3]).all() for t in reduced) and len(np.unique(whole[0][..., :3])) == 2


@pytest.mark.parametrize("block", [32, 64])
@pytest.mark.parametrize("n", ts.LIST_COUNTS)
def test_list_frames_hold_exactly_n_tiles_of_the_class(oracle, block, n):
    for n_alpha, n_sliver in ((n, 0), (0, n)):
        img, alpha, sliver = ts.list_frame(oracle, block, n_alpha, n_sliver)
        assert img.shape == (8 * block, 8 * block, 4)
        _, ow, oh, _ = oracle.shrink_image(img, block, block, ts.DIRECTIONAL, ts.LANCZOS3, ts.FACTOR, want_pixels=False)
        kinds = ts.kinds_of_frame(img, block, block, ow, oh)
        assert kinds.count(ts.ALPHA) == n_alpha == int(alpha.sum())
        assert kinds.count("sliver") == n_sliver == int(sliver.sum())
        assert [k == "sliver" for k in kinds] == sliver.tolist()
        assert len(set(kinds)) >= 5 and "other" not in kinds and ts.RAGGED not in kinds  # the rest: mixed kinds


@pytest.mark.parametrize("n", ts.LIST_COUNTS)
def test_tall_list_frames_put_all_n_tiles_on_one_blocks_tiles(oracle, n):
    """18 x 8 tiles of 64x64: the n tiles with the pixel all lie on residue class 0 mod 4 -- the tiles that block 0 of
    shrink64_kernel's four-block launch on one CU walks, in order -- and no other class has one"""
    img, alpha, sliver = ts.tall_list_frame(oracle, n)
    assert img.shape == (ts.LIST_TALL_ROWS * 64, 8 * 64, 4) and not sliver.any()
    _, ow, oh, _ = oracle.shrink_image(img, 64, 64, ts.DIRECTIONAL, ts.LANCZOS3, ts.FACTOR, want_pixels=False)
    kinds = ts.kinds_of_frame(img, 64, 64, ow, oh)
    per_class = [sum(k == ts.ALPHA for k in kinds[r::ts.LIST_CLASS]) for r in range(ts.LIST_CLASS)]
    assert per_class == [n, 0, 0, 0], per_class
    assert [k == ts.ALPHA for k in kinds] == alpha.tolist()
    assert len(kinds[0::ts.LIST_CLASS]) == 36 and "sliver" not in kinds and "other" not in kinds and ts.RAGGED not in kinds
    # the listed tiles are not one run: opaque tiles of the same block come between them
    mine = [k == ts.ALPHA for k in kinds[0::ts.LIST_CLASS]]
    assert any(a and not b for a, b in zip(mine, mine[1:])) and any(b and not a for a, b in zip(mine, mine[1:]))
    assert len({k for k in kinds if k != ts.ALPHA}) >= 5


def test_the_list_frame_with_both_classes(oracle):
    img, alpha, sliver = ts.list_frame(oracle, 32, 17, 17)
    _, ow, oh, _ = oracle.shrink_image(img, 32, 32, ts.DIRECTIONAL, ts.LANCZOS3, ts.FACTOR, want_pixels=False)
    kinds = ts.kinds_of_frame(img, 32, 32, ow, oh)
    assert kinds.count(ts.ALPHA) == 17 and kinds.count("sliver") == 17 and not (alpha & sliver).any()


def test_seam_counts_bracket_one_two_and_three_batches_of_every_detector():
    for b in ts.DETECTOR_BATCHES:
        for k in (1, 2, 3):
            assert k * b in ts.SEAM_COUNTS and k * b + 1 in ts.SEAM_COUNTS, (b, k)
    assert set((1, 2, 3, 4, 13, 14, 15, 16, 28, 29, 30, 31, 43, 44, 45, 46)) <= set(ts.SEAM_COUNTS)


# ---- e. detector alpha sequences --------------------------------------------------------------------------------------------------

# (bw, bh, width of a ragged right column, height of a ragged bottom row)
ALPHA_FRAMES = ([g + (0, 0) for g in ts.ALPHA_GEOMS[:3]] + [(32, 32, 0, ts.ALPHA_SHORT_ROW), (64, 64, 0, ts.ALPHA_SHORT_ROW)] +
                [g + ts.ALPHA_RAGGED[g] for g in ts.ALPHA_GEOMS[3:]])
ALPHA_FRAME_IDS = [f"{bw}x{bh}" + (f"-edge{ew}x{eh}" if ew or eh else "") for bw, bh, ew, eh in ALPHA_FRAMES]


def alpha_strides(ew):
    """the strides a frame is sequenced for: a ragged column means run-time geometry, oklab_kernel alone (15 tiles per batch)"""
    return (15,) if ew else ts.ALPHA_STRIDES


def test_alpha_seeds_are_the_first_that_leave_no_pair_and_no_triple_missing():
    assert ts.ALPHA_STRIDES == tuple(sorted(ts.DETECTOR_BATCHES))
    assert all(ts.ALPHA_COLS * ts.ALPHA_ROWS % b == 0 for b in ts.ALPHA_STRIDES)
    first = {False: ts.find_alpha_seed(False), True: ts.find_alpha_seed(True)}
    assert ts.ALPHA_SEEDS == {g: first[g in ts.ALPHA_RAGGED] for g in ts.ALPHA_GEOMS}
    for bw, bh, ew, eh in ALPHA_FRAMES:
        cols, rows, seq = ts.alpha_layout(bw, bh, ew, eh)
        kinds = ts.planned_alpha_kinds(ts.ALPHA_SEEDS[(bw, bh)], cols * rows)
        assert ts.missing_alpha_pairs(kinds, alpha_strides(ew), seq) == [], (bw, bh, ew, eh)
    # and a pair or a triple that is not there is reported
    kinds = ts.planned_alpha_kinds(ts.ALPHA_SEEDS[(32, 32)], 210)
    broken = ["top" if k == "bottom" and kinds[t + 14:t + 15] == ["middle"] else k for t, k in enumerate(kinds)]
    assert (14, "bottom", "middle") in ts.missing_alpha_pairs(broken)
    broken = ["full" if k == "opaque" and kinds[t + 3:t + 4] == ["opaque"] and kinds[t + 6:t + 7] == ["opaque"] else k for t, k in enumerate(kinds)]
    assert (3, "opaque", "opaque", "opaque") in ts.missing_alpha_pairs(broken)


def kind_of_plane(a):
    """the alpha kind of a tile, from its alpha bytes alone"""
    h, w = a.shape
    clear = a != 255
    n, rows = int(clear.sum()), np.nonzero(clear.any(axis=1))[0].tolist()
    if n == 0:
        return "opaque"
    if n == h * w:
        return "full"
    if n == 1 and a[clear][0] == 254:
        return "one 254"
    if len(rows) == 1 and len(set(a[clear].tolist())) == 1 and a[clear][0] < 240:
        kind = "top" if rows[0] == 0 else "bottom" if rows[0] == h - 1 else "middle"
        return kind if n == min(ts.ALPHA_PIXELS[kind], w) else "other"
    return "other"


def stored_value_bits(oracle, tile):
    """the bits of the value the oracle stores for a tile in shrink_by at BY_FACTOR: the detector's value through reduce_dims"""
    v = oracle.lod_oklab(tile, ts.BY_FACTOR)
    return int(oracle.reduce_dims(v, v, tile.shape[1], tile.shape[0])[2].view(np.uint32))


_alpha_frames = {}


def alpha_frame(oracle, key):
    if key not in _alpha_frames:
        _alpha_frames[key] = ts.alpha_sequence_frame(oracle, *key)
    return _alpha_frames[key]


@pytest.mark.parametrize("key", ALPHA_FRAMES, ids=ALPHA_FRAME_IDS)
def test_alpha_frames_hold_what_was_planned_and_transparent_tiles_of_both_fates(oracle, key):
    bw, bh, ew, eh = key
    img, planned = alpha_frame(oracle, key)
    cols, rows, seq = ts.alpha_layout(bw, bh, ew, eh)
    assert img.shape == ((rows - 1) * bh + (eh or bh), (cols - 1) * bw + (ew or bw), 4) and len(planned) == cols * rows
    parts = [img[r * bh:(r + 1) * bh, c * bw:(c + 1) * bw] for r in range(rows) for c in range(cols)]
    assert [kind_of_plane(p[..., 3]) for p in parts] == planned
    assert ts.missing_alpha_pairs(planned, alpha_strides(ew), seq) == []
    if not ew:  # every tile the frame holds is sequenced: the flat index is the detector's item number
        assert all(seq) and cols == ts.ALPHA_COLS
    else:       # the ragged column and the ragged row go to launches of their own, and both hold transparent pixels
        assert [s for s in seq] == [c < cols - 1 and r < rows - 1 for r in range(rows) for c in range(cols)]
        assert sum(k != "opaque" for k, s, p in zip(planned, seq, parts) if not s and p.shape[1] == ew) >= 4
        assert sum(k != "opaque" for k, s, p in zip(planned, seq, parts) if not s and p.shape[0] == eh) >= 4
    if eh and not ew:  # a short tile follows a tile that is transparent in every band, and some short tiles are transparent too
        short = [t for t, p in enumerate(parts) if p.shape[0] == eh]
        assert len(short) == cols and all(planned[t - cols] == "full" for t in short) and len({planned[t] for t in short}) >= 3
    if bw == 64 and bh == 64:  # top, middle and bottom fall to three different producer waves of oklab2_kernel<64>
        for p, k in zip(parts, planned):
            if k == "middle" and p.shape[0] == 64:
                r = int(np.nonzero((p[..., 3] != 255).any(axis=1))[0][0])
                assert r % 8 // 2 in (1, 2) and 0 % 8 // 2 == 0 and 63 % 8 // 2 == 3
    # a tile's non-opaque alpha is its own: none of its neighbours at the strides shares it
    for s in ts.ALPHA_STRIDES:
        for t in range(s, len(parts)):
            if planned[t] in ts.ALPHA_BASE and planned[t] == planned[t - s]:
                a, b = parts[t][..., 3], parts[t - s][..., 3]
                assert a[a != 255][0] != b[b != 255][0]
    # the oracle stores transparent tiles whole (the fast kernels leave their copy alone) and reduced (they resample them)
    vals, ow, oh, _ = oracle.shrink_image(img, bw, bh, ts.SHRINK_BY, ts.LANCZOS3, ts.BY_FACTOR, want_pixels=False)
    fates = {(k != "opaque", (int(w), int(h)) == p.shape[1::-1]) for k, w, h, p, s in zip(planned, ow, oh, parts, seq) if s}
    assert fates == {(False, False), (False, True), (True, False), (True, True)}, fates
    for kind in ts.ALPHA_KINDS:  # ... of every kind but `full`, whose alpha is noise: stored whole whatever lies under it
        whole = {(int(w), int(h)) == p.shape[1::-1] for k, w, h, p, s in zip(planned, ow, oh, parts, seq) if s and k == kind}
        assert whole == ({True} if kind == "full" else {False, True}), kind
    # stored_value_bits() of a tile is what shrink_image() reports for it: the bite condition below works tile by tile
    for t in range(0, len(parts), 5):
        assert stored_value_bits(oracle, np.ascontiguousarray(parts[t])) == int(vals[t:t + 1].view(np.uint32)[0])


@pytest.mark.parametrize("key", ALPHA_FRAMES, ids=ALPHA_FRAME_IDS)
def test_alpha_frames_bite_a_neighbours_alpha_changes_the_value_bits(oracle, key):
    """THE BITE CONDITION, on the inputs.  For every sequenced tile t and every stride s with a sequenced predecessor t - s the
    oracle values the tile under four alpha planes: its own, the opaque one, the predecessor's (a stale copy: cut to the tile's
    rows where the tile is a short one), and the per-pixel minimum of both (stale bytes mixed in).  Wherever two of these PLANES
    differ, the two VALUES must differ in their bits: a kernel that credits a tile with alpha left over from the tile its wave
    met a period earlier cannot produce the oracle's value.
    All four planes differ from each other -- the four values are four bit patterns -- whenever both tiles are transparent and
    neither plane lies under the other; that is asserted for every pair of top / bottom / middle / one 254 tiles whose planes are
    not equal.  Planes coincide only where they must: own = opaque for an opaque tile, predecessor = opaque after an opaque tile
    (then minimum = own), minimum = the lower plane where one lies under the other (a `full` tile against a few pixels of a
    higher alpha, one 254 against anything that covers its pixel), and all of them for `one 254` after `one 254` or opaque after
    opaque.  This is a condition on the draws, not a tolerance: a violation is mended in ALPHA_PIXELS / ALPHA_BASE."""
    bw, bh, ew, eh = key
    img, planned = alpha_frame(oracle, key)
    cols, rows, seq = ts.alpha_layout(bw, bh, ew, eh)
    parts = [np.array(img[r * bh:(r + 1) * bh, c * bw:(c + 1) * bw]) for r in range(rows) for c in range(cols)]

    def bits(tile, plane):
        t = tile.copy()
        t[..., 3] = plane
        return stored_value_bits(oracle, t)

    own_bits = {t: bits(p, p[..., 3]) for t, p in enumerate(parts) if seq[t]}
    twin_bits = {t: bits(p, 255) for t, p in enumerate(parts) if seq[t]}
    four = dict.fromkeys(alpha_strides(ew), 0)
    for s in alpha_strides(ew):
        for t in range(s, len(parts)):
            if not (seq[t] and seq[t - s]):
                continue
            h, w = parts[t].shape[:2]
            own, pred = parts[t][..., 3], parts[t - s][:h, :w, 3]
            planes = [own, np.full_like(own, 255), pred, np.minimum(own, pred)]
            values = [own_bits[t], twin_bits[t], bits(parts[t], planes[2]), bits(parts[t], planes[3])]
            for i in range(4):
                for j in range(i):
                    if (planes[i] != planes[j]).any():
                        assert values[i] != values[j], (s, t, planned[t - s], planned[t], i, j)
            sparse = set(ts.ALPHA_PIXELS)
            if planned[t] in sparse and planned[t - s] in sparse and h == bh and (own != pred).any():
                assert len(set(values)) == 4, (s, t, planned[t - s], planned[t])
            four[s] += len(set(values)) == 4
    assert all(n >= 30 for n in four.values()), four


@pytest.mark.parametrize("channels", [4, 3])
@pytest.mark.parametrize("geom", ts.SEAM_GEOMS, ids=lambda g: f"{g[0]}x{g[1]}")
def test_seam_frames_are_one_row_of_whole_and_reduced_tiles(oracle, geom, channels):
    bw, bh = geom
    both = set()
    for n in ts.SEAM_COUNTS:
        img, planned = ts.seam_frame(oracle, bw, bh, channels, n)
        assert img.shape == (bh, n * bw, channels)
        _, ow, oh, _ = oracle.shrink_image(img, bw, bh, ts.SHRINK_BY, ts.LANCZOS3, ts.BY_FACTOR, want_pixels=False)
        kinds = ts.whole_or_reduced(ow, oh, bw, bh)
        assert kinds == planned
        both |= set(kinds)
        if n >= 6:
            assert set(kinds) == {"whole", "reduced"}, (n, kinds)
    assert both == {"whole", "reduced"}
