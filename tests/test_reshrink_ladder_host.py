"""Re-shrink ladder (pxz_reshrink_varied_ladder_frames_device, pxz_transcode_varied_ladder_files), the part that needs no GPU:
the symbols, the LDS footprint of the kernel from its own layout function, and the inputs of tests/test_gpu_reshrink_ladder.py --
the batches of tests/test_reshrink_host.py with, per rung, what the oracle composition

    oracle.decode_container -> oracle.expand_image(expand_filter) -> oracle.shrink_image(mode, filter, factors[r])

makes of them, held against the conditions that make a ladder worth running: tiles whose rungs need several resamples, tiles
with clone rungs beside reduced ones, tiles that are expanded first, and one-axis keys."""
import functools
import os
import subprocess

import numpy as np
import pytest

from test_reshrink_host import CASES, DIRECTIONAL, FILTER_PAIRS, LDS_PER_CU, LIMIT_BLOCK, SHRINK_BY, cached_case, case_id

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pixlzr_hip.h")

# the factor lists of the varied ladder's tests, unsorted on purpose (a rung's place in the list must not matter)
FACTORS = {SHRINK_BY: [1.0, 0.5, 0.25, 0.125, 2.0, 0.05, 0.02, 0.01], DIRECTIONAL: [16.0, 8.0, 4.0, 2.0, 1.0, 0.5, 32.0, 0.1]}
TINY_BLOCKS = [(3, 5, 4), (5, 3, 3), (3, 3, 4)]


# ---- inputs ---------------------------------------------------------------------------------------------------------------

def oracle_rungs(oracle, case, factors, bw=None, bh=None):
    """per rung the oracle composition's tiles of the whole batch, concatenated in the varied layout: [(values, w, h, slots)]"""
    bw, bh = bw or case.bw, bh or case.bh
    per_rung = [[] for _ in factors]
    for (_, tw, th, slots), (w, h) in zip(case.inputs, case.sizes):
        img = oracle.expand_image(w, h, case.bw, case.bh, case.c, case.expand_filter, tw, th, slots)
        for r, f in enumerate(factors):
            per_rung[r].append(oracle.shrink_image(img, bw, bh, case.mode, case.filt, f))
    return [tuple(np.concatenate([x[k] for x in rung]) for k in range(4)) for rung in per_rung]


class Ladder:
    """one batch of tests/test_reshrink_host.py and its expected rungs"""

    def __init__(self, oracle, case, factors):
        self.case, self.factors = case, list(factors)
        self.rungs = oracle_rungs(oracle, case, self.factors)

    def counts(self):
        case = self.case
        tw, th = case.cat(case.inputs, 1), case.cat(case.inputs, 2)
        fw, fh = case.cat(case.full, 0), case.cat(case.full, 1)
        ow = np.stack([r[1] for r in self.rungs])  # [K, T]
        oh = np.stack([r[2] for r in self.rungs])
        clone = (ow == fw) & (oh == fh)
        has_clone, has_reduced = clone.any(axis=0), (~clone).any(axis=0)
        distinct = np.array([len({(int(ow[r, t]), int(oh[r, t])) for r in range(ow.shape[0]) if not clone[r, t]}) for t in range(tw.size)])
        stored_reduced = (tw != fw) | (th != fh)
        return dict(n=int(tw.size), three=int((distinct >= 3).sum()), mixed=int((has_clone & has_reduced).sum()),
                    expanded_mixed=int((stored_reduced & has_clone & has_reduced).sum()),
                    h_only=int(((ow < fw) & (oh == fh)).any(axis=0).sum()), v_only=int(((ow == fw) & (oh < fh)).any(axis=0).sum()))

    def check_conditions(self):
        case, k = self.case, self.counts()
        what = f"{case_id((case.family, case.mode, (case.bw, case.bh), case.c))} filters {case.expand_filter}/{case.filt}: {k}"
        assert 23 <= k["n"] <= 74, what
        assert k["three"] * 5 >= k["n"], what         # three or more distinct reduced sizes among a tile's rungs: several resamples of one X
        assert k["mixed"] * 5 >= k["n"], what         # a clone rung and a reduced rung: the clone is stored before the premultiply
        if case.family == "B":
            assert k["expanded_mixed"] >= 2, what     # ... on a tile that was expanded first
            if case.mode == DIRECTIONAL:
                assert k["h_only"] >= 1, what         # X -> A alone, along the rows
                assert k["v_only"] >= 1, what         # X -> A alone, along the columns


@functools.lru_cache(maxsize=None)
def cached_ladder(family, mode, tile, c, expand_filter, filt):
    """built once and shared, unchanged, by the tests that need them"""
    from oracle import binding
    binding.build()
    return Ladder(binding, cached_case(family, mode, tile, c, expand_filter, filt), FACTORS[mode])


# ---- 1. symbols -----------------------------------------------------------------------------------------------------------

def test_symbols_are_exported_and_declared(product):
    """fails before the re-shrink ladder exists"""
    names = ["pxz_reshrink_varied_ladder_frames_device", "pxz_transcode_varied_ladder_files", "pxz_reshrink_ladder_lds_bytes"]
    lib = product.load_library()
    text = open(HEADER).read()
    for name in names:
        assert hasattr(lib, name), name
        assert f"int {name}(" in text, name
        assert name in product.EXPORTED_SYMBOLS, name
    out = subprocess.run(["nm", "-D", "--defined-only", product.library_path()], capture_output=True, text=True, check=True).stdout
    for name in names:
        assert f" T {name}" in out, name
    assert hasattr(product.Handle, "reshrink_varied_ladder_frames_device") and hasattr(product.Handle, "transcode_varied_ladder_files")
    assert hasattr(product, "reshrink_ladder_lds_bytes")


# ---- 2. footprint ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", [SHRINK_BY, DIRECTIONAL])
@pytest.mark.parametrize("c", [3, 4])
@pytest.mark.parametrize("filt", range(5))
def test_lds_footprint_at_and_beyond_the_limit(product, mode, c, filt):
    """the function the kernel lays its LDS out with: within the CU's 160 KB at the documented limit, over it one step beyond on
    either axis, and never below the one-factor re-shrink's (the same planes and windows; the resampled images on top only
    where the free plane cannot hold them)"""
    bw, bh = LIMIT_BLOCK
    at = product.reshrink_ladder_lds_bytes(bw, bh, c, mode, filt)
    # two planes, the windows of both axes (at most 5 dwords per output sample), shrink_by's Oklab tables: I + F of a 128x128
    # tile are 48 KB at most and lie in the free plane
    assert 2 * 65536 < at <= 2 * 65536 + (bw + bh) * 5 * 4 + (14336 if mode == SHRINK_BY else 0) <= LDS_PER_CU, at
    for (w, h) in [(bw + 1, bh), (bw, bh + 1), (256, 65), (1, 16385)]:
        assert product.reshrink_ladder_lds_bytes(w, h, c, mode, filt) > LDS_PER_CU, (w, h)
    for (w, h) in [LIMIT_BLOCK, (256, 64), (64, 64), (37, 61), (48, 20), (32, 32), (16, 16), (1, 1)] + [(w, h) for (w, h, _) in TINY_BLOCKS]:
        got = product.reshrink_ladder_lds_bytes(w, h, c, mode, filt)
        assert product.reshrink_lds_bytes(w, h, mode, filt) <= got <= LDS_PER_CU, (w, h, got)
    assert product.reshrink_ladder_lds_bytes(32, 32, c, mode, filt) <= LDS_PER_CU // 3  # still several blocks per CU


@pytest.mark.parametrize("mode", [SHRINK_BY, DIRECTIONAL])
def test_lds_footprint_of_tiny_blocks(product, mode):
    """A is not always within one plane.  By hand: a 3x5 RGBA block has a plane of 3*5*4 = 60 -> 64 bytes; its widest horizontal
    result I is ceil(3/2)*5*4 = 40 -> 48 bytes and the result F behind it ceil(3/2)*ceil(5/2)*4 = 24 -> 32 bytes: 80 bytes, which
    the layout must place beside the planes (directional; shrink_by's detector takes 16 KB of its own either way, as in the
    re-shrink)"""
    for (bw, bh, c) in TINY_BLOCKS:
        for filt in range(5):
            got = product.reshrink_ladder_lds_bytes(bw, bh, c, mode, filt)
            assert got <= LDS_PER_CU and got % 16 == 0, (bw, bh, c, got)
            assert got >= product.reshrink_lds_bytes(bw, bh, mode, filt)
    if mode == DIRECTIONAL:
        assert product.reshrink_ladder_lds_bytes(3, 5, 4, mode, 4) == product.reshrink_lds_bytes(3, 5, mode, 4) + 80


def test_lds_footprint_refuses_bad_arguments(product):
    for args in [(0, 16, 4, 0, 0), (16, 0, 4, 0, 0), (16, 16, 2, 0, 0), (16, 16, 5, 0, 0), (16, 16, 4, 2, 0), (16, 16, 4, 0, 5)]:
        with pytest.raises(product.PxzError) as e:
            product.reshrink_ladder_lds_bytes(*args)
        assert e.value.code == -1


# ---- 3. the inputs of the GPU tests ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_gpu_inputs_meet_their_conditions(oracle, case):
    fam, mode, tile, c = case
    for (xf, sf) in FILTER_PAIRS:
        ladder = cached_ladder(fam, mode, tile, c, xf, sf)
        assert len(ladder.rungs) == len(FACTORS[mode]) == 8
        ladder.check_conditions()
        # rung by rung the ladder's expectation is the one-factor batch's own, where the factors meet
        if ladder.case.factor in ladder.factors:
            r = ladder.factors.index(ladder.case.factor)
            exp = tuple(ladder.case.cat(ladder.case.expected, k) for k in range(4))
            assert all((a == b).all() for a, b in zip(ladder.rungs[r][1:], exp[1:]))
            assert (ladder.rungs[r][0].view(np.uint32) == exp[0].view(np.uint32)).all()
