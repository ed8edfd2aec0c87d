"""What the frames of tile_sequences.py make the ORACLE do -- no GPU, no code under test.  The coverage the GPU module relies on
(every ordered pair of kinds at every stride, every shrink_by triple, exactly n listed tiles, whole and partial detector batches)
is asserted here from the oracle's stored sizes; the assertion is the condition the seeds were picked by."""
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
