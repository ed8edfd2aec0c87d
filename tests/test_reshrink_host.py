"""Re-shrink of stored tiles (pxz_reshrink_varied_frames_device, pxz_transcode_varied_files), the part that needs no GPU: the
symbols, the LDS footprint of the kernel at and beyond the documented limit, and the inputs of tests/test_gpu_reshrink.py --
built here, with their expected results from the oracle composition

    oracle.decode_container -> oracle.expand_image(expand_filter) -> oracle.shrink_image(mode, filter, factor)

and held against the conditions that make them worth running (enough tiles cloned in, cloned out, reduced on both axes, on
one axis, changed), so that no GPU test passes on inputs that exercise nothing."""
import functools
import os
import subprocess

import numpy as np
import pytest

from test_varied_decode_host import draw_tiles

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pixlzr_hip.h")

TILES = [(16, 16), (32, 32), (64, 64), (48, 20), (37, 61)]
NEAREST, TRIANGLE, CATMULLROM, GAUSSIAN, LANCZOS3 = range(5)
# (expand_filter, the shrink's filter): the five filters on both sides, and one pair that differs
FILTER_PAIRS = [(f, f) for f in range(5)] + [(NEAREST, LANCZOS3)]
SHRINK_BY, DIRECTIONAL = 0, 1
LDS_PER_CU = 160 * 1024
LIMIT_BLOCK = (128, 128)  # block_w * block_h * 4 <= 65536, RGB and RGBA alike
# family A: the factor a file was written with, and the stronger one it is re-shrunk at


def factors_a(mode, tile, c):
    """shrink_by 2.0 -> 1.0, directional 32 -> 16.  The RGBA batches of shrink_by, whose every second image is DIST_ALPHA, keep
    nearly all tiles full at those factors (13-24 of 64-74 reduced on both axes: below the third the conditions ask for), so
    they take a stronger pair -- the factor pair is changed, never the threshold."""
    if mode == DIRECTIONAL:
        return (32.0, 16.0)
    if c == 4:
        return (0.5, 0.25) if tile == (64, 64) else (1.0, 0.5)
    return (2.0, 1.0)


# family B: drawn tiles
FACTOR_B = {SHRINK_BY: 1.0, DIRECTIONAL: 8.0}

CASES = [(fam, mode, tile, c) for fam in "AB" for mode in (SHRINK_BY, DIRECTIONAL) for tile in TILES for c in (3, 4)]


def case_id(case):
    fam, mode, (bw, bh), c = case
    return f"{fam}-{'by' if mode == SHRINK_BY else 'dir'}-{bw}x{bh}-c{c}"


# ---- inputs ---------------------------------------------------------------------------------------------------------------

def batch_sizes(bw, bh, mode, family):
    """5-9 images of sides <= 300: the smallest image the mode takes, one a pixel short of a tile, one a pixel past a tile on
    both axes (shrink_by; the directional call refuses 1-px edge tiles, so there the edge tiles are 2 px wide and 2 px high:
    the 0/0 path), and images of several tiles with ragged edges"""
    past = 1 if mode == SHRINK_BY else 2
    sizes = [(1, 1) if mode == SHRINK_BY else (2, 2), (bw - 1, bh - 1), (bw + past, bh + past)]
    big = [(min(5 * bw + 3, 300), min(4 * bh + 5, 300)), (min(4 * bw + 7, 300 - bw // 4), min(5 * bh + 2, 300 - bh // 3)), (3 * bw + 9, 2 * bh)]
    if family == "B":
        big = [(2 * bw + 3, bh + 6), (bw + 5, 3 * bh + 2), (3 * bw, bh)]
    sizes += big
    assert 5 <= len(sizes) <= 9 and all(w <= 300 and h <= 300 for (w, h) in sizes)
    return sizes


def full_sizes(w, h, bw, bh):
    cols, rows = -(-w // bw), -(-h // bh)
    fw = np.array([bw if tx < cols - 1 else w - (cols - 1) * bw for ty in range(rows) for tx in range(cols)], np.uint32)
    fh = np.array([bh if ty < rows - 1 else h - (rows - 1) * bh for ty in range(rows) for tx in range(cols)], np.uint32)
    return fw, fh


class Case:
    """one batch of stored tiles (as files of the oracle's writer and as the oracle's reader returns them) and what the oracle
    composition makes of them"""

    def __init__(self, oracle, family, mode, tile, c, expand_filter, filt, sizes=None):
        from oracle import binding as ob
        bw, bh = tile
        self.family, self.mode, self.bw, self.bh, self.c, self.expand_filter, self.filt = family, mode, bw, bh, c, expand_filter, filt
        self.sizes = sizes if sizes is not None else batch_sizes(bw, bh, mode, family)
        seed = bw * 131 + bh * 7 + c + 1000 * mode
        rng = np.random.default_rng(seed)
        self.files = []
        if family == "A":
            f1, self.factor = factors_a(mode, tile, c)
            for k, (w, h) in enumerate(self.sizes):
                dist = ob.DIST_ALPHA if c == 4 and k % 2 == 1 else ob.DIST_OPAQUE
                img = oracle.synth_frame(w, h, c, frame_index=k, dist=dist)
                vals, tw, th, slots = oracle.shrink_image(img, bw, bh, mode, filt, f1)
                self.files.append(oracle.encode_container(w, h, bw, bh, c, 0, vals, None, tw, th, slots))
        else:
            self.factor = FACTOR_B[mode]
            counts = [-(-w // bw) * -(-h // bh) for (w, h) in self.sizes]
            dealt = np.split(rng.permutation(np.arange(sum(counts)) % 3), np.cumsum(counts)[:-1])  # FULL / HALVED / ANY, evenly
            for (w, h), cl in zip(self.sizes, dealt):
                vals, tw, th, slots, _ = draw_tiles(rng, w, h, bw, bh, c, cl)
                self.files.append(oracle.encode_container(w, h, bw, bh, c, 0, vals, None, tw, th, slots))
        # the oracle composition, image by image
        self.inputs, self.expected, self.full = [], [], []
        for raw, (w, h) in zip(self.files, self.sizes):
            d = oracle.decode_container(raw)
            slots = np.ascontiguousarray(d["slots"][:, : bw * bh * c])
            self.inputs.append((d["values"], d["tw"], d["th"], slots))
            img = oracle.expand_image(w, h, bw, bh, c, expand_filter, d["tw"], d["th"], slots)
            self.expected.append(oracle.shrink_image(img, bw, bh, mode, filt, self.factor))
            self.full.append(full_sizes(w, h, bw, bh))

    def cat(self, which, k):
        return np.concatenate([x[k] for x in which])

    def counts(self):
        tw, th = self.cat(self.inputs, 1), self.cat(self.inputs, 2)
        ow, oh = self.cat(self.expected, 1), self.cat(self.expected, 2)
        fw, fh = self.cat(self.full, 0), self.cat(self.full, 1)
        return dict(n=tw.size, in_full=int(((tw == fw) & (th == fh)).sum()), out_full=int(((ow == fw) & (oh == fh)).sum()),
                    both=int(((ow < fw) & (oh < fh)).sum()), one=int(((ow < fw) != (oh < fh)).sum()),
                    changed=int(((ow != tw) | (oh != th)).sum()))

    def check_conditions(self):
        k = self.counts()
        what = f"{case_id((self.family, self.mode, (self.bw, self.bh), self.c))} filters {self.expand_filter}/{self.filt}: {k}"
        n = k["n"]
        if self.family == "A":
            assert k["in_full"] * 10 >= n, what      # tiles stored full (clone in)
            assert k["out_full"] * 10 >= n, what     # tiles that stay full (clone out)
            assert k["both"] * 3 >= n, what          # reduced on both axes
            assert k["changed"] * 3 >= n, what       # the stored size changes
        elif self.mode == DIRECTIONAL:
            assert k["one"] * 10 >= n, what          # reduced on exactly one axis
        else:
            assert k["out_full"] * 10 >= 9 * n, what  # every expand form feeds the detector and the clone-out store
        small = (1, 1) if self.mode == SHRINK_BY else (2, 2)
        assert small in self.sizes and (self.bw - 1, self.bh - 1) in self.sizes, what
        if self.mode == DIRECTIONAL:
            assert any(w % self.bw == 2 and h % self.bh == 2 and w > self.bw and h > self.bh for (w, h) in self.sizes), what
        else:
            assert (self.bw + 1, self.bh + 1) in self.sizes, what


@functools.lru_cache(maxsize=None)
def cached_case(family, mode, tile, c, expand_filter, filt):
    """the batches are built once and shared, unchanged, by the tests that need them"""
    from oracle import binding
    binding.build()
    return Case(binding, family, mode, tile, c, expand_filter, filt)


# ---- 1. symbols -----------------------------------------------------------------------------------------------------------

def test_symbols_are_exported_and_declared(product):
    """fails before the re-shrink exists"""
    names = ["pxz_reshrink_varied_frames_device", "pxz_transcode_varied_files", "pxz_reshrink_lds_bytes"]
    lib = product.load_library()
    text = open(HEADER).read()
    for name in names:
        assert hasattr(lib, name), name
        assert f"int {name}(" in text, name
        assert name in product.EXPORTED_SYMBOLS, name
    out = subprocess.run(["nm", "-D", "--defined-only", product.library_path()], capture_output=True, text=True, check=True).stdout
    for name in names:
        assert f" T {name}" in out, name
    assert hasattr(product.Handle, "reshrink_varied_frames_device") and hasattr(product.Handle, "transcode_varied_files")


# ---- 2. footprint ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", [SHRINK_BY, DIRECTIONAL])
@pytest.mark.parametrize("filt", range(5))
def test_lds_footprint_at_and_beyond_the_limit(product, mode, filt):
    """the function the launch sizes its LDS with: within the CU's 160 KB at the documented limit (the footprint does not depend
    on the channel count: a plane is a dword per pixel for RGB and RGBA), over it one step beyond, on either axis"""
    bw, bh = LIMIT_BLOCK
    assert bw * bh * 4 == 65536
    at = product.reshrink_lds_bytes(bw, bh, mode, filt)
    # two planes, the windows of both axes (at most 5 dwords per output sample), shrink_by's Oklab tables
    assert 2 * 65536 < at <= 2 * 65536 + (bw + bh) * 5 * 4 + (14336 if mode == SHRINK_BY else 0) <= LDS_PER_CU, at
    for (w, h) in [(bw + 1, bh), (bw, bh + 1), (256, 65), (1, 16385)]:
        assert product.reshrink_lds_bytes(w, h, mode, filt) > LDS_PER_CU, (w, h)
    for (w, h) in [(256, 64), (512, 32), (64, 64), (37, 61), (1, 1)]:
        assert product.reshrink_lds_bytes(w, h, mode, filt) <= LDS_PER_CU, (w, h)
    # (the staged windows grow with block_w + block_h: a block of one row of 16384 pixels is within the planes' limit, not within LDS)
    assert product.reshrink_lds_bytes(1, 16384, mode, filt) > LDS_PER_CU
    # small planes: the detector's own 16 KB beside them (shrink_by), and still several blocks per CU
    assert product.reshrink_lds_bytes(32, 32, mode, filt) <= LDS_PER_CU // 4


def test_lds_footprint_refuses_bad_arguments(product):
    for args in [(0, 16, 0, 0), (16, 0, 0, 0), (16, 16, 2, 0), (16, 16, 0, 5)]:
        with pytest.raises(product.PxzError) as e:
            product.reshrink_lds_bytes(*args)
        assert e.value.code == -1


# ---- 3. the inputs of the GPU tests ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_gpu_inputs_meet_their_conditions(oracle, case):
    fam, mode, tile, c = case
    for (xf, sf) in FILTER_PAIRS:
        batch = cached_case(fam, mode, tile, c, xf, sf)
        assert 5 <= len(batch.sizes) <= 9
        batch.check_conditions()
