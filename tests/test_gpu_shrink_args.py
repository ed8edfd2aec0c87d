"""The precedence of the argument checks of the single-geometry shrink calls: pxz_shrink_frames_device, pxz_lod_frames_device,
pxz_shrink_ladder_frames_device and pxz_process_frames_device.

Every call has a list of single faults.  Every pair of them is applied together, and the call must answer with the code and text
of the fault that EXPECTED names for the pair, with every output still poisoned: all validation runs on the host, before
anything is written or launched.  One clean call per entry point follows.

EXPECTED is recorded, not derived: `python tests/test_gpu_shrink_args.py` on a GPU prints it for the library in the tree.  It
was filled from the build of the commit before the route of these calls became a value planned once on the host, so that the
plan is held to the order of checks each call had.  Row i of a call is a string over the faults j > i: '<' fault i is reported,
'>' fault j, '-' the pair is not formed (both faults change the same argument).

The refusal "a WxH RGB tile needs more LDS than there is (and this filter cannot run it as RGBA)" is not in the lists: it takes
PXZ_NO_BIG_TILES in the environment of the process and a table set in which an opaque alpha does not stay opaque, and no filter
and block shape between the two LDS limits has such a set (tests/test_shrink_plan_host.py holds the plan to that text with the
fact given as an input)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

INVALID_ARG, TILE_TOO_SMALL, UNSUPPORTED = -1, -4, -5
SHRINK_BY, DIRECTIONAL, LANCZOS3, NEAREST = 0, 1, 4, 0
POISON, POISON32 = 0x5A, 0x5A5A5A5A
NAN = float("nan")

# two RGBA frames of 64x64 in tiles of 32x32; a height of 33 leaves a 1-px edge row
W, H, N, CH, BW, BH, K = 64, 64, 2, 4, 32, 32, 2
TILES = N * 2 * 2

# name -> (what it changes in the arguments of a clean call, code, start of the text)
FAULTS = {
    "null factors": (dict(factors=None), INVALID_ARG, "null factors"),
    "no factors": (dict(n_factors=0), INVALID_ARG, "n_factors must be 1..16, got 0"),
    "non-finite rung": (dict(factors=[1.0, NAN]), INVALID_ARG, "factor 1 must be finite"),
    "null device pointer": (dict(null=True), INVALID_ARG, "null device pointer"),
    "null descriptor": (dict(no_frames=True), INVALID_ARG, "null descriptor"),
    "empty batch": (dict(n=0), INVALID_ARG, "empty frame batch"),
    "side above 2^24": (dict(w=2 ** 24 + 1), UNSUPPORTED, "image sides above 2^24 are not supported"),
    "bad channels": (dict(c=5), INVALID_ARG, "channels must be 3 or 4, got 5"),
    "pitch below a row": (dict(pitch_less=1), INVALID_ARG, "pitch smaller than a row"),
    "stride below a frame": (dict(stride_less=1), INVALID_ARG, "frame stride smaller than a frame"),
    "zero block": (dict(bh=0), INVALID_ARG, "zero block size"),
    "bad mode": (dict(mode=2), INVALID_ARG, "mode must be 0 or 1"),
    "bad filter": (dict(filt=5), INVALID_ARG, "filter must be 0..4"),
    "non-finite factor": (dict(factor=NAN), INVALID_ARG, "factor must be finite"),
    "1-px edge, directional": (dict(h=33, mode=DIRECTIONAL), TILE_TOO_SMALL, "directional detector needs tiles of at least 2x2 px"),
    "block side above 65535": (dict(bw=65536), UNSUPPORTED, "block side above 65535"),
    "block of 2^20 pixels": (dict(bw=32768), UNSUPPORTED, "a 32768x32 tile needs"),
}
FRAMES = ["null device pointer", "null descriptor", "empty batch", "side above 2^24", "bad channels", "pitch below a row", "stride below a frame"]
BLOCKS = ["block side above 65535", "block of 2^20 pixels"]


class Entry:
    """one device entry point: its faults in the order the call checks them (for readers), how it is called, what it writes"""

    def __init__(self, name, faults):
        self.name = name
        self.faults = [(f, *FAULTS[f]) for f in faults]

    def base(self):
        return dict(w=W, h=H, c=CH, n=N, pitch_less=0, stride_less=0, no_frames=False, null=False, bw=BW, bh=BH, mode=SHRINK_BY, filt=LANCZOS3,
                    factor=1.0, factors=[1.0, 0.5], n_factors=K)

    def buffers(self):
        """-> (the frames: zeros, the outputs: poisoned)"""
        import torch
        pixels = torch.zeros(N * H * W * CH, dtype=torch.uint8, device="cuda")
        words = lambda *shape: torch.full(shape, POISON32, dtype=torch.int32, device="cuda")  # noqa: E731
        if self.name == "pxz_lod_frames_device":
            return pixels, (words(TILES), words(TILES))
        if self.name == "pxz_process_frames_device":
            return pixels, (torch.full((N, H, W, 4), POISON, dtype=torch.uint8, device="cuda"),)
        k = K if self.name == "pxz_shrink_ladder_frames_device" else 1
        return pixels, (words(k * TILES), words(k * TILES), words(k * TILES), torch.full((k * TILES, BW * BH * CH), POISON, dtype=torch.uint8, device="cuda"))

    def assert_untouched(self, out):
        for t in out:
            assert (t.cpu().numpy().view(np.uint8) == POISON).all()

    def call(self, gpu, product, pixels, out, a):
        """-> (return code, pxz_last_error)"""
        L = gpu._L
        pitch = a["w"] * a["c"] - a["pitch_less"]
        fd = product.binding.Frames(a["w"], a["h"], a["c"], pitch, a["n"], 0, pitch * a["h"] - a["stride_less"])
        frames = None if a["no_frames"] else C.byref(fd)
        pd = product.binding.Params(a["bw"], a["bh"], a["mode"], a["filt"], a["factor"], 0)
        src = None if a["null"] else C.c_void_p(pixels.data_ptr())
        outs = [C.c_void_p(t.data_ptr()) for t in out]
        if self.name == "pxz_process_frames_device":
            rc = L.pxz_process_frames_device(gpu._h, frames, C.byref(pd), NEAREST, src, *outs, W * 4, W * 4 * H)
        elif self.name == "pxz_shrink_ladder_frames_device":
            fac = None if a["factors"] is None else np.ascontiguousarray(a["factors"], np.float32)
            rc = L.pxz_shrink_ladder_frames_device(gpu._h, frames, C.byref(pd), None if fac is None else C.c_void_p(fac.ctypes.data), a["n_factors"],
                                                   src, *outs)
        else:
            rc = getattr(L, self.name)(gpu._h, frames, C.byref(pd), src, *outs)
        return rc, (L.pxz_last_error(gpu._h) or b"").decode()


PARAMS = ["zero block", "bad mode", "bad filter", "non-finite factor"]
ENTRIES = [
    Entry("pxz_shrink_frames_device", FRAMES + PARAMS + ["1-px edge, directional"] + BLOCKS),
    Entry("pxz_lod_frames_device", FRAMES + PARAMS + ["1-px edge, directional"] + BLOCKS),
    # (a rung's factor stands in the place of the parameters' factor, which is not read)
    Entry("pxz_shrink_ladder_frames_device",
          ["null factors", "no factors", "non-finite rung"] + FRAMES + ["zero block", "bad mode", "bad filter", "1-px edge, directional"] + BLOCKS),
    # (process() reads neither mode nor factor)
    Entry("pxz_process_frames_device", FRAMES + ["zero block", "bad filter"] + BLOCKS),
]

# recorded from the build of the parent of the plan (see above); the comments name fault i of each row
EXPECTED = {
    "pxz_shrink_frames_device": [
        "<<<<<<<<<<<<<",  # null device pointer
        "<<<<<<<<<<<<",  # null descriptor
        "<<<<<<<<<<<",  # empty batch
        "<<<<<<<<<<",  # side above 2^24
        "<<<<<<<<<",  # bad channels
        "<<<<<<<<",  # pitch below a row
        "<<<<<<<",  # stride below a frame
        "<<<<<<",  # zero block
        "<<-<<",  # bad mode
        "<<<<",  # bad filter
        "<<<",  # non-finite factor
        "<<",  # 1-px edge, directional
        "-",  # block side above 65535
        "",  # block of 2^20 pixels
    ],
    "pxz_lod_frames_device": [
        "<<<<<<<<<<<<<",  # null device pointer
        "<<<<<<<<<<<<",  # null descriptor
        "<<<<<<<<<<<",  # empty batch
        "<<<<<<<<<<",  # side above 2^24
        "<<<<<<<<<",  # bad channels
        "<<<<<<<<",  # pitch below a row
        "<<<<<<<",  # stride below a frame
        "<<<<<<",  # zero block
        "<<-<<",  # bad mode
        "<<<<",  # bad filter
        "<<<",  # non-finite factor
        "<<",  # 1-px edge, directional
        "-",  # block side above 65535
        "",  # block of 2^20 pixels
    ],
    "pxz_shrink_ladder_frames_device": [
        "<-<<<<<<<<<<<<<",  # null factors
        "<<<<<<<<<<<<<<",  # no factors
        "<<<<<<<<<<<<<",  # non-finite rung
        "<<<<<<<<<<<<",  # null device pointer
        "<<<<<<<<<<<",  # null descriptor
        "<<<<<<<<<<",  # empty batch
        "<<<<<<<<<",  # side above 2^24
        "<<<<<<<<",  # bad channels
        "<<<<<<<",  # pitch below a row
        "<<<<<<",  # stride below a frame
        "<<<<<",  # zero block
        "<-<<",  # bad mode
        "<<<",  # bad filter
        "<<",  # 1-px edge, directional
        "-",  # block side above 65535
        "",  # block of 2^20 pixels
    ],
    "pxz_process_frames_device": [
        "><<<<<<<<<",  # null device pointer
        "<<<<<<<<<",  # null descriptor
        "<<<<<<<<",  # empty batch
        "<<<<<<<",  # side above 2^24
        "<<<<<<",  # bad channels
        "<<<<<",  # pitch below a row
        "<<<<",  # stride below a frame
        "<<<",  # zero block
        "<<",  # bad filter
        "-",  # block side above 65535
        "",  # block of 2^20 pixels
    ],
}


def observe(gpu, product, entry, notes=None):
    """every single fault, then every pair: -> the rows of EXPECTED as this library answers them (notes: the recorder's list for
    answers that are neither fault's, marked '?' in the row, instead of failing)"""
    import torch
    pixels, out = entry.buffers()
    base = entry.base()

    def reported(change):
        rc, err = entry.call(gpu, product, pixels, out, {**base, **change})
        assert rc != 0, f"{entry.name} took {change}: a faulted call must be rejected on the host"
        torch.cuda.synchronize()
        entry.assert_untouched(out)
        return rc, err

    for (name, change, code, text) in entry.faults:
        rc, err = reported(change)
        if notes is not None and not (rc == code and err.startswith(text)):
            notes.append((entry.name, name, rc, err))
            continue
        assert rc == code and err.startswith(text), (entry.name, name, rc, err)
    rows = []
    for i, (ni, ci, codei, texti) in enumerate(entry.faults):
        row = ""
        for (nj, cj, codej, textj) in entry.faults[i + 1:]:
            if set(ci) & set(cj):
                row += "-"
                continue
            rc, err = reported({**ci, **cj})
            first, second = rc == codei and err.startswith(texti), rc == codej and err.startswith(textj)
            if notes is not None and first == second:
                notes.append((entry.name, ni, nj, rc, err))
                row += "?"
                continue
            assert first != second, (entry.name, ni, nj, rc, err)
            row += "<" if first else ">"
        rows.append(row)
    return pixels, out, rows


def clean_call(gpu, product, entry, pixels, out):
    """frames of zeros: every tile of a shrink_by is flat and comes out 1x1 with value 0; process() gives the zeros back"""
    import torch
    rc, err = entry.call(gpu, product, pixels, out, entry.base())
    assert rc == 0, err
    torch.cuda.synchronize()
    if entry.name == "pxz_process_frames_device":
        assert (out[0].cpu().numpy() == 0).all()
    elif entry.name == "pxz_lod_frames_device":
        assert (out[0].cpu().numpy() != POISON32).all() and (out[1].cpu().numpy() != POISON32).all()
    else:
        assert (out[0].cpu().numpy() == 0).all() and (out[1].cpu().numpy() == 1).all() and (out[2].cpu().numpy() == 1).all()
        assert (out[3].cpu().numpy()[:, :CH] == 0).all()


@pytest.fixture(scope="module")
def gpu(product):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    h = product.Handle(0)
    yield h
    h.close()


@pytest.mark.parametrize("entry", ENTRIES, ids=[e.name for e in ENTRIES])
def test_pairs_of_faults_report_the_one_checked_first(gpu, product, entry):
    pixels, out, rows = observe(gpu, product, entry)
    names = [f[0] for f in entry.faults]
    for i, (got, want) in enumerate(zip(rows, EXPECTED[entry.name])):
        for j, (g, w) in enumerate(zip(got, want)):
            assert g == w, f"{entry.name}: '{names[i]}' with '{names[i + 1 + j]}' reports the {'second' if g == '>' else 'first'}"
    assert len(rows) == len(EXPECTED[entry.name]) and all(len(g) == len(w) for g, w in zip(rows, EXPECTED[entry.name]))
    clean_call(gpu, product, entry, pixels, out)


if __name__ == "__main__":  # the recorder
    from conftest import load_product
    product = load_product()
    gpu = product.Handle(0)
    notes = []
    print("EXPECTED = {")
    for entry in ENTRIES:
        pixels, out, rows = observe(gpu, product, entry, notes)
        clean_call(gpu, product, entry, pixels, out)
        print(f'    "{entry.name}": [')
        for (fault, row) in zip(entry.faults, rows):
            print(f'        "{row}",  # {fault[0]}')
        print("    ],")
    print("}")
    for note in notes:
        print("#", note)
    gpu.close()
