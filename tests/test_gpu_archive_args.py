"""The precedence of the argument checks of the archive calls (stored tiles in, stored tiles out): pxz_reshrink_varied_frames_device,
pxz_reshrink_varied_ladder_frames_device, pxz_retile_varied_frames_device, pxz_retile_varied_ladder_frames_device,
pxz_reshrink_distortion_varied_device, pxz_retile_distortion_varied_device and pxz_patch_windows_device.

Every call has a list of single faults.  Every pair of them is applied together, and the call must answer with the code and text
of the fault that EXPECTED names for the pair, with every output still poisoned: all validation runs on the host, before
anything is written or launched.  One clean call per entry point follows.

EXPECTED is recorded, not derived: `python tests/test_gpu_archive_args.py` on a GPU prints it for the library in the tree.  It
was filled from the build of the commit before the host bodies of these calls were folded into shared steps, so that the fold
is held to the order of checks each call had.  Row i of a call is a string over the faults j > i: '<' fault i is reported,
'>' fault j, '-' the pair is not formed (both faults change the same argument)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from test_gpu_reshrink import SIZE_POISON, assert_still_poisoned
from test_gpu_varied_decode import poisoned
from test_reshrink_host import DIRECTIONAL, LANCZOS3, LDS_PER_CU, SHRINK_BY

pytestmark = pytest.mark.gpu

INVALID_ARG, TILE_TOO_SMALL, UNSUPPORTED = -1, -4, -5
POISON64 = 0x5A5A5A5A5A5A5A5A

# three images of at most 64x64; image 1 has a 1-px edge column in the 16x16 grid and in the 32x32 grid
SIZES = [(40, 40), (33, 64), (64, 64)]
SW, SH, BW, BH, CH = 32, 32, 16, 16, 4
S_TILES, T_TILES = 4 + 4 + 4, 9 + 12 + 16
# the patch: one window inside tile (0, 0) of image 0, one in the 1-px edge column of image 1
WINDOWS = [(0, 1, 1, 5, 5, 20, 0), (1, 32, 0, 1, 4, 4, 512)]
W_TILES = 2
NAN = float("nan")

# name -> (what it changes in the arguments of a clean call, code, start of the text)
COMMON = {
    "null device pointer": (dict(null="tw"), INVALID_ARG, "null device pointer"),
    "bad channels": (dict(c=5), INVALID_ARG, "channels must be 3 or 4, got 5"),
    "zero block": (dict(bw=0), INVALID_ARG, "zero block size"),
    "bad mode": (dict(mode=2), INVALID_ARG, "mode must be 0 or 1"),
    "bad filter": (dict(filt=5), INVALID_ARG, "filter must be 0..4"),
    "non-finite factor": (dict(factor=NAN), INVALID_ARG, "factor must be finite"),
    "zero source block": (dict(sw=0), INVALID_ARG, "zero source block size"),
    "bad expand_filter": (dict(xf=5), INVALID_ARG, "expand_filter must be 0..4, got 5"),
    "null descriptors": (dict(no_descs=True), INVALID_ARG, "null image descriptors"),
    "empty batch": (dict(n_images=0), INVALID_ARG, "empty image batch"),
    "empty side": (dict(sizes=[(40, 40), (33, 64), (0, 7)]), INVALID_ARG, "image 2: empty image (0x7)"),
    "1-px edge, directional": (dict(mode=DIRECTIONAL), TILE_TOO_SMALL, "image 1: directional detector needs tiles of at least 2x2 px"),
    "tile above 64 KB": (dict(bh=1025), UNSUPPORTED, "varied batches stage every tile in LDS"),
    "no sets": (dict(n_sets=0), INVALID_ARG, "n_sets must be at least 1"),
    "null factors": (dict(factors=None), INVALID_ARG, "null factors"),
    "no factors": (dict(n_factors=0), INVALID_ARG, "n_factors must be 1..32, got 0"),
    "non-finite rung": (dict(factors=[1.0, NAN]), INVALID_ARG, "factor 1 must be finite"),
}


def beyond(text, **change):
    return (change, UNSUPPORTED, text)


class Entry:
    """one device entry point: its faults in the order the call checks them (for readers), how it is called, what it writes"""

    def __init__(self, name, faults, own=None, ladder=False, src=False, distortion=False, patch=False):
        self.name, self.ladder, self.src, self.distortion, self.patch = name, ladder, src, distortion, patch
        table = {**COMMON, **(own or {})}
        self.faults = [(f, *table[f]) for f in faults]

    def base(self):
        return dict(sizes=SIZES, n_images=None, no_descs=False, c=CH, sw=SW, sh=SH, bw=BW, bh=BH, mode=SHRINK_BY, filt=LANCZOS3, factor=1.0,
                    xf=LANCZOS3, factors=[1.0, 0.5], n_factors=2, n_sets=2, null=None)

    def buffers(self):
        """-> (inputs by name, outputs, flags): stored tiles of 1x1 px in every place, every output poisoned"""
        import torch
        K = 2 if (self.ladder or self.distortion) else None
        n_in = W_TILES if self.patch else (S_TILES if self.src else T_TILES)
        n_out = W_TILES if self.patch else T_TILES
        in_slot = (SW * SH if self.src else BW * BH) * CH
        ones = lambda *shape: torch.ones(shape, dtype=torch.int32, device="cuda")  # noqa: E731
        zeros = lambda *shape: torch.zeros(shape, dtype=torch.uint8, device="cuda")  # noqa: E731
        if self.distortion:
            ins = dict(ref_w=ones(n_in), ref_h=ones(n_in), ref_slots=zeros(n_in, in_slot), tw=ones(K, n_out), th=ones(K, n_out),
                       slots=zeros(K, n_out, BW * BH * CH))
            full = lambda *shape: torch.full(shape, POISON64, dtype=torch.int64, device="cuda")  # noqa: E731
            out = (full(K, n_out, CH), full(K, len(SIZES), CH))
            flags = torch.full((len(SIZES),), SIZE_POISON, dtype=torch.int32, device="cuda")
            return ins, out, flags
        ins = dict(tw=ones(n_in), th=ones(n_in), slots=zeros(n_in, in_slot))
        if self.patch:
            ins["patch"] = zeros(1024)
        out, flags = poisoned(n_out * (K or 1), BW * BH * CH, len(WINDOWS) if self.patch else len(SIZES))
        return ins, out, flags

    def assert_untouched(self, out, flags):
        if not self.distortion:
            return assert_still_poisoned(out, flags)
        for t in out:
            assert (t.cpu().numpy().view(np.uint64) == POISON64).all()
        assert (flags.cpu().numpy().view(np.uint32) == SIZE_POISON).all()

    def call(self, gpu, product, ins, out, flags, a):
        """-> (return code, pxz_last_error)"""
        L = gpu._L
        geoms = [(w, h, 0, 0) if self.patch else (w, h, w * a["c"], 0) for (w, h) in a["sizes"]]
        descs = None if a["no_descs"] else C.cast(product.image_descs(geoms), C.c_void_p)
        n = len(geoms) if a["n_images"] is None else a["n_images"]
        mode, factor = (0, 0.0) if self.distortion else (a["mode"], 0.0 if self.ladder else a["factor"])
        pd = product.binding.Params(a["bw"], a["bh"], mode, a["filt"], factor, 0)
        ptr = {k: C.c_void_p(t.data_ptr()) for k, t in ins.items()}
        if a["null"]:
            ptr[a["null"]] = None
        src = (a["sw"], a["sh"]) if self.src else ()
        fac = None if a["factors"] is None else np.ascontiguousarray(a["factors"], np.float32)
        rungs = (None if fac is None else C.c_void_p(fac.ctypes.data), a["n_factors"]) if self.ladder else ()
        outs = [C.c_void_p(t.data_ptr()) for t in out] + [C.c_void_p(flags.data_ptr())]
        if self.distortion:
            rc = getattr(L, self.name)(gpu._h, descs, n, a["c"], *src, C.byref(pd), a["xf"], a["n_sets"], ptr["ref_w"], ptr["ref_h"],
                                       ptr["ref_slots"], ptr["tw"], ptr["th"], ptr["slots"], *outs)
        elif self.patch:
            rc = L.pxz_patch_windows_device(gpu._h, descs, n, C.cast(product.window_descs(WINDOWS), C.c_void_p), len(WINDOWS), a["c"], C.byref(pd),
                                            a["xf"], ptr["patch"], ptr["tw"], ptr["th"], ptr["slots"], *outs)
        else:
            rc = getattr(L, self.name)(gpu._h, descs, n, a["c"], *src, C.byref(pd), a["xf"], *rungs, ptr["tw"], ptr["th"], ptr["slots"], *outs)
        return rc, (L.pxz_last_error(gpu._h) or b"").decode()


PARAMS = ["null device pointer", "bad channels", "zero block", "bad mode", "bad filter"]
BATCH = ["null descriptors", "empty batch", "empty side", "1-px edge, directional"]
RESHRINK_LDS = beyond("a re-shrink keeps two planes", bh=1025)
RETILE_LDS = beyond("a re-tile keeps a 16x16 tile image", sh=2048)
PATCH_EDGE = (dict(mode=DIRECTIONAL), TILE_TOO_SMALL, "window 1: directional detector needs tiles of at least 2x2 px")

ENTRIES = [
    Entry("pxz_reshrink_varied_frames_device", PARAMS + ["non-finite factor", "bad expand_filter", "beyond LDS"] + BATCH,
          {"beyond LDS": RESHRINK_LDS}),
    Entry("pxz_reshrink_varied_ladder_frames_device",
          ["null factors", "no factors", "non-finite rung"] + PARAMS + ["bad expand_filter", "beyond LDS"] + BATCH,
          {"beyond LDS": beyond("a re-shrink ladder keeps two planes", bh=1025)}, ladder=True),
    Entry("pxz_retile_varied_frames_device", PARAMS + ["non-finite factor", "tile above 64 KB", "zero source block", "bad expand_filter", "beyond LDS"] + BATCH,
          {"beyond LDS": RETILE_LDS}, src=True),
    Entry("pxz_retile_varied_ladder_frames_device",
          ["null factors", "no factors", "non-finite rung"] + PARAMS + ["tile above 64 KB", "zero source block", "bad expand_filter", "beyond LDS"] + BATCH,
          {"beyond LDS": RETILE_LDS}, ladder=True, src=True),
    # (the distortions read neither mode nor factor)
    Entry("pxz_reshrink_distortion_varied_device",
          ["null device pointer", "bad channels", "zero block", "bad filter", "tile above 64 KB", "no sets", "bad expand_filter", "null descriptors", "empty batch",
           "empty side", "beyond LDS"],
          {"beyond LDS": beyond("a wave keeps three planes", bh=1024)}, distortion=True),
    Entry("pxz_retile_distortion_varied_device",
          ["null device pointer", "bad channels", "zero block", "bad filter", "tile above 64 KB", "zero source block", "no sets", "bad expand_filter", "beyond LDS",
           "null descriptors", "empty batch", "empty side"],
          {"beyond LDS": beyond("the distortion of re-tiled tiles keeps two 16x16 tile images", sh=2048)}, distortion=True, src=True),
    Entry("pxz_patch_windows_device", PARAMS + ["non-finite factor", "bad expand_filter", "beyond LDS"] + BATCH,
          {"beyond LDS": RESHRINK_LDS, "1-px edge, directional": PATCH_EDGE}, patch=True),
]

# recorded from the build of the parent of the fold (see above); the comments name fault i of each row
EXPECTED = {
    "pxz_reshrink_varied_frames_device": [
        "<<<<<<<<<<<",  # null device pointer
        "<<<<<<<<<<",  # bad channels
        "<<<<<<<<<",  # zero block
        "<<<<<<<-",  # bad mode
        "<<<<<<<",  # bad filter
        "<<<<<<",  # non-finite factor
        "<<<<<",  # bad expand_filter
        "<<<<",  # beyond LDS
        "<<<",  # null descriptors
        "<<",  # empty batch
        ">",  # empty side
        "",  # 1-px edge, directional
    ],
    "pxz_reshrink_varied_ladder_frames_device": [
        "<-<<<<<<<<<<<",  # null factors
        "<<<<<<<<<<<<",  # no factors
        "<<<<<<<<<<<",  # non-finite rung
        "<<<<<<<<<<",  # null device pointer
        "<<<<<<<<<",  # bad channels
        "<<<<<<<<",  # zero block
        "<<<<<<-",  # bad mode
        "<<<<<<",  # bad filter
        "<<<<<",  # bad expand_filter
        "<<<<",  # beyond LDS
        "<<<",  # null descriptors
        "<<",  # empty batch
        ">",  # empty side
        "",  # 1-px edge, directional
    ],
    "pxz_retile_varied_frames_device": [
        "<<<<<<<<<<<<<",  # null device pointer
        "<<<<<<<<<<<<",  # bad channels
        "<<<<<<<<<<<",  # zero block
        "<<<<<<<<<-",  # bad mode
        "<<<<<<<<<",  # bad filter
        "<<<<<<<<",  # non-finite factor
        "<<<<<<<",  # tile above 64 KB
        "<<<<<<",  # zero source block
        "<<<<<",  # bad expand_filter
        "<<<<",  # beyond LDS
        "<<<",  # null descriptors
        "<<",  # empty batch
        ">",  # empty side
        "",  # 1-px edge, directional
    ],
    "pxz_retile_varied_ladder_frames_device": [
        "<-<<<<<<<<<<<<<",  # null factors
        "<<<<<<<<<<<<<<",  # no factors
        "<<<<<<<<<<<<<",  # non-finite rung
        "<<<<<<<<<<<<",  # null device pointer
        "<<<<<<<<<<<",  # bad channels
        "<<<<<<<<<<",  # zero block
        "<<<<<<<<-",  # bad mode
        "<<<<<<<<",  # bad filter
        "<<<<<<<",  # tile above 64 KB
        "<<<<<<",  # zero source block
        "<<<<<",  # bad expand_filter
        "<<<<",  # beyond LDS
        "<<<",  # null descriptors
        "<<",  # empty batch
        ">",  # empty side
        "",  # 1-px edge, directional
    ],
    "pxz_reshrink_distortion_varied_device": [
        "<<<<<<<<<<",  # null device pointer
        "<<<<<<<<<",  # bad channels
        "<<<<<<<<",  # zero block
        "<<<<<<<",  # bad filter
        "<<<<<-",  # tile above 64 KB
        "<<<<<",  # no sets
        "<<<<",  # bad expand_filter
        "<<<",  # null descriptors
        "<<",  # empty batch
        "<",  # empty side
        "",  # beyond LDS
    ],
    "pxz_retile_distortion_varied_device": [
        "<<<<<<<<<<<",  # null device pointer
        "<<<<<<<<<<",  # bad channels
        "<<<<<<<<<",  # zero block
        "<<<<<<<<",  # bad filter
        "<<<<<<<",  # tile above 64 KB
        "<<<<<<",  # zero source block
        "<<<<<",  # no sets
        "<<<<",  # bad expand_filter
        "<<<",  # beyond LDS
        "<<",  # null descriptors
        "<",  # empty batch
        "",  # empty side
    ],
    "pxz_patch_windows_device": [
        "<<<<<<<<<<<",  # null device pointer
        "<<<<<<<<<<",  # bad channels
        "<<<<<<<<<",  # zero block
        "<<<<<<<-",  # bad mode
        "<<<<<<<",  # bad filter
        "<<<<<<",  # non-finite factor
        "<<<<<",  # bad expand_filter
        "<<<<",  # beyond LDS
        "<<<",  # null descriptors
        "<<",  # empty batch
        "<",  # empty side
        "",  # 1-px edge, directional
    ],
}


def lds_query(product, entry, a):
    """what the call's own size query says of the blocks of `a`"""
    name = entry.name
    if name == "pxz_patch_windows_device" or name == "pxz_reshrink_varied_frames_device":
        return product.reshrink_lds_bytes(a["bw"], a["bh"], a["mode"], a["xf"])
    if name == "pxz_reshrink_varied_ladder_frames_device":
        return product.reshrink_ladder_lds_bytes(a["bw"], a["bh"], a["c"], a["mode"], a["xf"])
    if name == "pxz_retile_varied_frames_device":
        return product.retile_lds_bytes(a["sw"], a["sh"], a["bw"], a["bh"], a["mode"], a["xf"])
    if name == "pxz_retile_varied_ladder_frames_device":
        return product.retile_ladder_lds_bytes(a["sw"], a["sh"], a["bw"], a["bh"], a["c"], a["mode"], a["xf"])
    if name == "pxz_reshrink_distortion_varied_device":
        return product.reshrink_distortion_lds_bytes(a["bw"], a["bh"], a["c"], a["xf"], a["filt"])
    return product.retile_distortion_lds_bytes(a["sw"], a["sh"], a["bw"], a["bh"], a["c"], a["xf"], a["filt"])


def observe(gpu, product, entry):
    """every single fault, then every pair: -> the rows of EXPECTED as this library answers them"""
    import torch
    ins, out, flags = entry.buffers()
    base = entry.base()

    def reported(change):
        rc, err = entry.call(gpu, product, ins, out, flags, {**base, **change})
        assert rc != 0, f"{entry.name} took {change}: a faulted call must be rejected on the host"
        torch.cuda.synchronize()
        entry.assert_untouched(out, flags)
        return rc, err

    for (name, change, code, text) in entry.faults:
        rc, err = reported(change)
        assert rc == code and err.startswith(text), (entry.name, name, rc, err)
    lds = dict((f[0], f[1]) for f in entry.faults)["beyond LDS"]
    assert lds_query(product, entry, base) <= LDS_PER_CU < lds_query(product, entry, {**base, **lds})
    rows = []
    for i, (ni, ci, codei, texti) in enumerate(entry.faults):
        row = ""
        for (nj, cj, codej, textj) in entry.faults[i + 1:]:
            if set(ci) & set(cj):
                row += "-"
                continue
            rc, err = reported({**ci, **cj})
            first, second = rc == codei and err.startswith(texti), rc == codej and err.startswith(textj)
            assert first != second, (entry.name, ni, nj, rc, err)
            row += "<" if first else ">"
        rows.append(row)
    return ins, out, flags, rows


@pytest.fixture(scope="module")
def gpu(product):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    h = product.Handle(0)
    yield h
    h.close()


@pytest.mark.parametrize("entry", ENTRIES, ids=[e.name for e in ENTRIES])
def test_pairs_of_faults_report_the_one_checked_first(gpu, product, entry):
    import torch
    ins, out, flags, rows = observe(gpu, product, entry)
    names = [f[0] for f in entry.faults]
    for i, (got, want) in enumerate(zip(rows, EXPECTED[entry.name])):
        for j, (g, w) in enumerate(zip(got, want)):
            assert g == w, f"{entry.name}: '{names[i]}' with '{names[i + 1 + j]}' reports the {'second' if g == '>' else 'first'}"
    assert len(rows) == len(EXPECTED[entry.name]) and all(len(g) == len(w) for g, w in zip(rows, EXPECTED[entry.name]))
    # the clean call: every stored tile is 1x1, so every tile of a shrink_by comes out 1x1; nothing is flagged
    rc, err = entry.call(gpu, product, ins, out, flags, entry.base())
    assert rc == 0, err
    torch.cuda.synchronize()
    assert gpu.decode_status() == 0 and (flags.cpu().numpy() == 0).all()
    if entry.distortion:
        assert (out[0].cpu().numpy() == 0).all() and (out[1].cpu().numpy() == 0).all()  # (zeros against zeros)
    else:
        assert (out[1].cpu().numpy() == 1).all() and (out[2].cpu().numpy() == 1).all()


if __name__ == "__main__":  # the recorder
    from conftest import load_product
    product = load_product()
    gpu = product.Handle(0)
    print("EXPECTED = {")
    for entry in ENTRIES:
        rows = observe(gpu, product, entry)[3]
        print(f'    "{entry.name}": [')
        for (fault, row) in zip(entry.faults, rows):
            print(f'        "{row}",  # {fault[0]}')
        print("    ],")
    print("}")
    gpu.close()
