"""Re-tile ladder (pxz_retile_varied_ladder_frames_device, and pxz_transcode_varied_ladder_files with another block size), the
part that needs no GPU: the symbols, the LDS footprint of the kernel from its own layout function, and the inputs of
tests/test_gpu_retile_ladder.py -- the batches of tests/test_retile_host.py with, per rung, what the oracle composition

    oracle.decode_container -> oracle.expand_image(source block, expand_filter) -> oracle.shrink_image(destination block, factors[r])

makes of them, held against the conditions that make a ladder worth running: destination tiles whose rungs need several
resamples of one assembled image, tiles with clone rungs beside reduced ones, and one-axis keys."""
import functools
import os
import subprocess

import numpy as np
import pytest

from test_reshrink_host import DIRECTIONAL, LANCZOS3, LDS_PER_CU, SHRINK_BY
from test_reshrink_ladder_host import FACTORS, TINY_BLOCKS
from test_retile_host import CASES, PROMISED, TINY, cached_retile_case, case_id, filter_pairs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pixlzr_hip.h")

# Family A on the tiny pairs: tiles of 15-16 pixels change level around factors of 4-300 (the cases' own factors), so the common
# lists leave nearly every rung of theirs a clone (0.02-0.04 of the tiles with two reduced sizes).  Their list is the case's own
# factor scaled, unsorted like the common ones.
TINY_SCALES = [1.0, 0.5, 0.25, 0.125, 2.0, 4.0, 0.0625, 8.0]


def ladder_factors(case):
    if case.family == "A" and case.pair in TINY:
        return [case.factor * s for s in TINY_SCALES]
    return list(FACTORS[case.mode])


# ---- inputs ---------------------------------------------------------------------------------------------------------------

def oracle_retile_rungs(oracle, case, factors):
    """per rung the oracle composition's tiles of the whole batch, concatenated in the varied layout at the destination block:
    [(values, w, h, slots)]"""
    (sw, sh), (dw, dh) = case.pair
    per_rung = [[] for _ in factors]
    for (_, tw, th, slots), (w, h) in zip(case.inputs, case.sizes):
        img = oracle.expand_image(w, h, sw, sh, case.c, case.expand_filter, tw, th, slots)
        for r, f in enumerate(factors):
            per_rung[r].append(oracle.shrink_image(img, dw, dh, case.mode, case.filt, f))
    return [tuple(np.concatenate([x[k] for x in rung]) for k in range(4)) for rung in per_rung]


class RetileLadder:
    """one batch of tests/test_retile_host.py and its expected rungs"""

    def __init__(self, oracle, case, factors):
        self.case, self.factors = case, list(factors)
        self.rungs = oracle_retile_rungs(oracle, case, self.factors)

    def counts(self):
        case = self.case
        fw, fh = case.cat(case.dst_full, 0), case.cat(case.dst_full, 1)
        ow = np.stack([r[1] for r in self.rungs])  # [K, T]
        oh = np.stack([r[2] for r in self.rungs])
        clone = (ow == fw) & (oh == fh)
        has_clone, has_reduced = clone.any(axis=0), (~clone).any(axis=0)
        distinct = np.array([len({(int(ow[r, t]), int(oh[r, t])) for r in range(ow.shape[0]) if not clone[r, t]}) for t in range(fw.size)])
        return dict(n=int(fw.size), two=int((distinct >= 2).sum()), mixed=int((has_clone & has_reduced).sum()),
                    h_only=int(((ow < fw) & (oh == fh)).any(axis=0).sum()), v_only=int(((ow == fw) & (oh < fh)).any(axis=0).sum()))

    def check_conditions(self):
        case, k = self.case, self.counts()
        what = f"{case_id((case.family, case.mode, case.pair, case.c))} filters {case.expand_filter}/{case.filt}: {k}"
        assert 23 <= k["n"] <= 456, what
        assert k["two"] * 5 >= k["n"], what       # two or more distinct reduced sizes among a tile's rungs: several resamples of one X
        assert k["mixed"] * 10 >= k["n"], what    # a clone rung and a reduced rung: the clone is stored before the premultiply
        if case.family == "B" and case.mode == DIRECTIONAL:
            assert k["h_only"] >= 1, what         # X -> A alone, along the rows
            assert k["v_only"] >= 1, what         # X -> A alone, along the columns
        case.check_conditions()                   # the source side: stored small / full, straddling, mixed, inside


@functools.lru_cache(maxsize=None)
def cached_retile_ladder(family, mode, pair, c, expand_filter, filt):
    """built once and shared, unchanged, by the tests that need them"""
    from oracle import binding
    binding.build()
    case = cached_retile_case(family, mode, pair, c, expand_filter, filt)
    return RetileLadder(binding, case, ladder_factors(case))


# ---- 1. symbols -----------------------------------------------------------------------------------------------------------

def test_symbols_are_exported_declared_and_bound(product):
    """fails before the re-tile ladder exists"""
    names = ["pxz_retile_varied_ladder_frames_device", "pxz_retile_ladder_lds_bytes"]
    lib = product.load_library()
    text = open(HEADER).read()
    for name in names:
        assert hasattr(lib, name), name
        assert f"int {name}(" in text, name
        assert name in product.EXPORTED_SYMBOLS, name
    out = subprocess.run(["nm", "-D", "--defined-only", product.library_path()], capture_output=True, text=True, check=True).stdout
    for name in names:
        assert f" T {name}" in out, name
    assert hasattr(product.Handle, "retile_varied_ladder_frames_device") and hasattr(product, "retile_ladder_lds_bytes")


# ---- 2. footprint ---------------------------------------------------------------------------------------------------------

def test_lds_footprint_refuses_bad_arguments(product):
    for args in [(0, 16, 16, 16, 4, 0, 0), (16, 0, 16, 16, 4, 0, 0), (16, 16, 0, 16, 4, 0, 0), (16, 16, 16, 0, 4, 0, 0), (16, 16, 16, 16, 2, 0, 0),
                 (16, 16, 16, 16, 5, 0, 0), (16, 16, 16, 16, 4, 2, 0), (16, 16, 16, 16, 4, 0, 5)]:
        with pytest.raises(product.PxzError) as e:
            product.retile_ladder_lds_bytes(*args)
        assert e.value.code == -1
    assert product.load_library().pxz_retile_ladder_lds_bytes(16, 16, 16, 16, 4, 0, 0, None) == -1


@pytest.mark.parametrize("mode", [SHRINK_BY, DIRECTIONAL])
@pytest.mark.parametrize("c", [3, 4])
@pytest.mark.parametrize("filt", range(5))
def test_lds_footprint_admits_what_the_retile_admits(product, mode, c, filt):
    """the ladder needs no other plane for X (its tail goes X -> I -> F), so where I + F fit the image's plane -- every block but
    tiny ones -- a block takes at most what the one-factor re-tile takes"""
    for (src, dst) in PROMISED:
        got = product.retile_ladder_lds_bytes(*src, *dst, c, mode, filt)
        assert got <= product.retile_lds_bytes(*src, *dst, mode, filt) <= LDS_PER_CU, (src, dst, got)
    # four blocks per CU at the destination blocks of 32x32 and 48x20, whatever the source block up to 64x64
    for src in [(16, 16), (32, 32), (48, 20), (37, 61), (64, 64)]:
        for dst in [(32, 32), (48, 20)]:
            assert product.retile_ladder_lds_bytes(*src, *dst, c, mode, filt) <= LDS_PER_CU // 4, (src, dst)
    # beyond the CU: a plane above 64 KB; two blocks that leave parts as large as a 64 KB source tile; a one-row block
    for (src, dst) in [((129, 128), (129, 128)), ((128, 128), (128, 127)), ((128, 127), (128, 128)), ((16384, 1), (16384, 1)), ((1, 16384), (1, 16384))]:
        assert product.retile_ladder_lds_bytes(*src, *dst, c, mode, filt) > LDS_PER_CU, (src, dst)


def window_dwords(product, src, filt):
    """dwords of one staged window for the up-scaling tables of a source block: 1 + ceil(widest window / 2) over every (full
    size, stored size) of its two sides; 1 when there is no table (a 1x1 block)"""
    widest = 0
    for full in set(src):
        for stored in range(1, full):
            widest = max(widest, window_taps(product, stored, full, filt))
    return 1 + (widest + 1) // 2


@functools.lru_cache(maxsize=None)
def window_taps(product, stored, full, filt):
    return product.axis_table(stored, full, filt)[2].shape[1]


def restated_footprint(mode, src, dst, c, wdw):
    """the layout of retile_ladder_lds, said again: [Oklab tables, shrink_by only] [X: D] [U = max(assembly, A)]"""
    (sw, sh), (dw, dh) = src, dst

    def up16(v):
        return (v + 15) & ~15
    d = up16(dw * dh * 4)
    if d > 65536 or sw * sh * 4 > 65536:
        return 0xffffffff
    cw, ch = min(sw, dw), min(sh, dh)
    pw, ph = min(sw, cw + 2 * (wdw - 1) + 2), min(sh, ch + 2 * (wdw - 1) + 2)
    assembly = up16(pw * ph * 4) + up16(cw * ph * 4) + (((sw + sh) * wdw + 3) & ~3) * 4
    hw, hh = ((dw + 1) // 2 if dw > 1 else 0), ((dh + 1) // 2 if dh > 1 else 0)
    a = max(up16(hw * dh * c) + up16(hw * hh * c), up16(dw * hh * c))
    if mode == SHRINK_BY:
        a = max(a, 16384)
    return (14336 if mode == SHRINK_BY else 0) + d + max(assembly, a)


SWEEP = PROMISED + TINY + [((bw, bh), (bw, bh)) for (bw, bh, _) in TINY_BLOCKS] + \
    [((3, 5), (32, 32)), ((32, 32), (3, 5)), ((1, 1), (1, 1)), ((1, 7), (7, 1)), ((64, 64), (128, 128)), ((128, 128), (16, 16)), ((128, 128), (64, 64)),
     ((256, 16), (16, 256)), ((61, 37), (48, 20)), ((128, 128), (128, 127)), ((129, 128), (16, 16)), ((16, 16), (129, 128))]


@pytest.mark.parametrize("mode", [SHRINK_BY, DIRECTIONAL])
@pytest.mark.parametrize("filt", range(5))
def test_lds_footprint_equals_the_restated_layout(product, mode, filt):
    for (src, dst) in SWEEP:
        wdw = window_dwords(product, src, filt)
        for c in (3, 4):
            want = restated_footprint(mode, src, dst, c, 1)  # (a pair beyond the CU with windows of one dword is reported as that)
            if want <= LDS_PER_CU:
                want = restated_footprint(mode, src, dst, c, wdw)
            assert product.retile_ladder_lds_bytes(*src, *dst, c, mode, filt) == want, (src, dst, c, wdw)
    if mode == DIRECTIONAL:
        # by hand, a 3x5 RGBA block: D = 3*5*4 = 60 -> 64; I = ceil(3/2)*5*4 = 40 -> 48 and F = ceil(3/2)*ceil(5/2)*4 = 24 -> 32, so
        # A = 80 > D.  The assembly of 3x5 parts from 3x5 tiles: 3x5 staged dwords (64), as large an intermediate (64), 8 windows
        assert restated_footprint(mode, (3, 5), (3, 5), 4, 1) == 64 + max(64 + 64 + 8 * 4, 80)


# ---- 3. the inputs of the GPU tests ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_gpu_inputs_meet_their_conditions(oracle, case):
    fam, mode, pair, c = case
    for (xf, sf) in filter_pairs(pair):
        lad = cached_retile_ladder(fam, mode, pair, c, xf, sf)
        assert len(lad.rungs) == len(lad.factors) == 8
        lad.check_conditions()
        # rung by rung the ladder's expectation is the one-factor batch's own, where the factors meet
        if lad.case.factor in lad.factors:
            r = lad.factors.index(lad.case.factor)
            exp = tuple(lad.case.cat(lad.case.expected, k) for k in range(4))
            assert all((a == b).all() for a, b in zip(lad.rungs[r][1:], exp[1:]))
            assert (lad.rungs[r][0].view(np.uint32) == exp[0].view(np.uint32)).all()


def test_tiny_family_a_lists_hold_the_cases_own_factor(oracle):
    for mode in (SHRINK_BY, DIRECTIONAL):
        for pair in TINY:
            c = 3 if pair == TINY[0] else 4
            lad = cached_retile_ladder("A", mode, pair, c, LANCZOS3, LANCZOS3)
            assert lad.factors[0] == lad.case.factor and lad.factors != FACTORS[mode]
