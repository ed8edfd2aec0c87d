"""The route of a single-geometry shrink call, planned on the host (pxz_shrink_plan.h), without a GPU.

pxz_shrink_plan_check.bin reads cases and prints the route's fields; the expected fields below are written out by hand from the
rules, the rule named beside each case -- the program produces none of them.  A case states what differs from the default call:
one 64x64 RGBA frame, tight rows, 32x32 tiles, shrink_directionally, Lanczos3, pixels wanted, an aligned address, 256 CUs, no
statistics.  The program's sweep asserts the plan's invariants over every block side of 1..130 and 256, 512, 1024."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "pixlzr-rust_amd", "csrc", "pxz_shrink_plan_check.bin")
BY = "mode=0"
UNKNOWN = 0xFFFFFFFF


def routes(lines):
    assert os.path.exists(TOOL), "run __graft_entry__.build()"
    r = subprocess.run([TOOL], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    out = []
    for line in r.stdout.splitlines():
        if line.startswith("rc=0") or line.startswith("ladder="):
            out.append(dict(tok.split("=", 1) for tok in line.split()))
        else:
            rc, text = line.split(" ", 1)
            out.append({"rc": rc[3:], "text": text[5:]})
    assert len(out) == len(lines)
    return out


def check(cases):
    got = routes([c[1] for c in cases])
    for (rule, line, want), g in zip(cases, got):
        for key, value in want.items():
            if key == "text":
                assert g.get("text", "").startswith(value), (rule, line, g)
            else:
                assert g.get(key) == str(value), (rule, line, key, g)


# the LDS image of a 32x32 tile, in dwords: rows of 16 pixel pairs skewed to 18, 4 planes of 18 x 32, the transposed planes 4 x 16 x 18
# (or shrink_by's own detector planes, 3 x 1024, where they are larger), 4 x 18 + 4 x 18 of slack
T32, T32_LAB, T32_BARE = 2304 + 1152 + 144, 2304 + 3072 + 144, 2304 + 144

ALIGNMENT = [
    ("aligned address, pitch 256: as given, every tile on the fast path", "low=0", dict(input="given", full="2x2", rgba=0, tile=T32, lab=0)),
    ("address & 15 = 4: re-pitched into scratch", "low=4", dict(input="repitched", pitch=256, stride=16384, rgba=16384, full="2x2")),
    ("address & 15 = 1: re-pitched", "low=1", dict(input="repitched", rgba=16384, full="2x2")),
    ("PXZ_NO_REPITCH: as given, no fast path", "low=4 knob=no_repitch", dict(input="given", rgba=0, full="0x0", okrows=0)),
    ("a pitch of 260 is no multiple of 16", "pitch=260", dict(input="repitched", pitch=256, stride=16384)),
    ("one frame: its stride does not count", "stride=16388", dict(input="given", full="2x2", stride=16384)),
    ("two frames: a stride of 16388 is no multiple of 16", "n=2 stride=16388", dict(input="repitched", rgba=32768, stride=16384)),
]

# shrink_by on RGBA: region 1 the right column (edge_w x bh), 2 the bottom row (bw x edge_h), 3 the corner; rN=tiles:bands
EDGES = [
    ("32: 40x40, edge 8x8; 8 rows are a whole band (256 / 32), so the detector's interior launch takes the last row", f"{BY} w=40 h=40",
     dict(det="rgba", full="1x1", okrows=2, edges=5, r1="1:1", r2="0:0", r3="1:1", clone=1, lab=0, bands=4, okscratch=0)),
    ("32: 64x40, full columns, last row of 8", f"{BY} h=40", dict(det="rgba", full="2x1", okrows=2, edges=0)),
    ("32: 64x36, a last row of 4 is half a band: region 2, two tiles of 128 px", f"{BY} h=36", dict(full="2x1", okrows=1, edges=2, r2="2:1")),
    ("32: 33x64, a 1-px column walked as one quad: region 1, two tiles; rows of 132 bytes are re-pitched to 144", f"{BY} w=33",
     dict(input="repitched", pitch=144, full="1x2", okrows=2, edges=1, r1="2:1", r3="0:0")),
    ("16: 20x20, edge 4x4; the quantum is 16 rows, so no ragged row is ever whole bands", f"{BY} bw=16 bh=16 w=20 h=20",
     dict(full="1x1", okrows=1, edges=7, r1="1:1", r2="1:1", r3="1:1", bands=1)),
    ("16: 32x24", f"{BY} bw=16 bh=16 w=32 h=24", dict(full="2x1", okrows=1, edges=2, r2="2:1")),
    ("16: 32x32, no edge", f"{BY} bw=16 bh=16 w=32 h=32", dict(full="2x2", okrows=2, edges=0)),
    ("64: 128x72, a last row of 8 is a whole super-band", f"{BY} bw=64 bh=64 w=128 h=72", dict(full="2x1", okrows=2, edges=0, bands=16, okscratch=0)),
    ("64: 128x68, a last row of 4 is not", f"{BY} bw=64 bh=64 w=128 h=68", dict(full="2x1", okrows=1, edges=2, r2="2:1")),
]

SHAPES = [
    ("8x8 = 64 px is in", f"{BY} bw=8 bh=8 w=16 h=16", dict(det="rgba", lab=0, full="2x2", clone=0, bands=1, tile=128 + 64 + 32)),
    ("4x12 = 48 px is out: own detector planes, no fast region, not even a re-pitch", f"{BY} bw=4 bh=12 w=8 h=24 low=4",
     dict(input="given", det="none", lab=144, full="0x0", tile=96 + 144 + 32)),
    ("128x128 = 16384 px is in; 64 bands are parked in HBM, 13 dwords per pixel quad; the image itself is beyond LDS", f"{BY} bw=128 bh=128 w=128 h=128",
     dict(det="rgba", lab=0, bands=64, okscratch=64 * 3328, full="1x1", tile=51216, lds=51216 * 4 + 256, big=512, blocks=1, bigscratch=51216 * 4)),
    ("128x132 is out", f"{BY} bw=128 bh=132 w=128 h=132", dict(det="none", lab=3 * 128 * 132, full="0x0", tile=86064)),
    ("a block width of 6 is out", f"{BY} bw=6 bh=16 w=12 h=32", dict(det="none", lab=288, full="0x0")),
    ("a frame narrower than a block: the layout keeps its detector planes, no detector launch", f"{BY} w=20",
     dict(det="none", lab=3072, tile=T32_LAB, full="0x2", edges=0)),
]

RGB = [
    ("native at 32: rows of 192 bytes are 4-byte aligned; RGB keeps the generic kernel's planes", f"{BY} c=3",
     dict(input="given", ch=3, det="rgb", clone=1, full="2x2", lab=3072, tile=T32_LAB, needs_opaque=0)),
    ("native at 16: no clone_ahead", f"{BY} c=3 bw=16 bh=16 w=32 h=32", dict(input="given", det="rgb", clone=0, full="2x2")),
    ("native at 64", f"{BY} c=3 bw=64 bh=64 w=128 h=128", dict(input="given", det="rgb", clone=1, full="2x2", okscratch=0)),
    ("an odd address: widened, slots in scratch", f"{BY} c=3 low=1",
     dict(input="widened", ch=4, pitch=256, rgba=16384, slots4=4 * 4096, needs_opaque=1, det="rgba", lab=0, clone=1, tile=T32)),
    ("24x8, a general shape: widened when an opaque alpha stays opaque", f"{BY} c=3 bw=24 bh=8 w=48 h=16 opaque=1",
     dict(input="widened", ch=4, pitch=192, det="rgba", lab=0, needs_opaque=1)),
    ("... and not otherwise", f"{BY} c=3 bw=24 bh=8 w=48 h=16 opaque=0", dict(input="given", ch=3, det="none", lab=576, needs_opaque=1)),
    ("96x96 RGB under PXZ_NO_BIG_TILES: 47248 dwords with its planes do not fit, 29200 as RGBA without them do",
     f"{BY} c=3 bw=96 bh=96 w=96 h=96 knob=no_big_tiles opaque=1", dict(input="widened", tile=29200, big=0, lab=0)),
    ("... and the filter cannot run it as RGBA", f"{BY} c=3 bw=96 bh=96 w=96 h=96 knob=no_big_tiles opaque=0",
     dict(rc=-5, text="a 96x96 RGB tile needs more LDS than there is (and this filter cannot run it as RGBA)")),
]

# directional, a convolution: 116x116 is 4 x 58 x 116 + 4 x 58 x 58 + 8 x 58 = 40832 dwords and 16 waves' sums = 163584 bytes of 163840;
# 117x117 is 4 x 60 x 117 + 4 x 59 x 60 + 8 x 60 = 42720 dwords
LDS = [
    ("the largest square block in LDS", "bw=116 bh=116 w=116 h=116", dict(tile=40832, lds=163584, big=0, blocks=0, bigscratch=0)),
    ("the next one runs from HBM: 2 blocks per CU, capped by the tile count", "bw=117 bh=117 w=117 h=117",
     dict(tile=42720, lds=171136, big=512, blocks=1, bigscratch=170880)),
    ("... 12 tiles", "bw=117 bh=117 w=351 h=468", dict(big=512, blocks=12, bigscratch=12 * 170880)),
    ("... on 4 CUs", "bw=117 bh=117 w=351 h=468 cus=4", dict(big=8, blocks=8, bigscratch=8 * 170880)),
    ("2^20 pixels", "bw=1024 bh=1024 w=1024 h=1024", dict(rc=-5, text="a 1024x1024 tile needs")),
    ("PXZ_NO_BIG_TILES", "bw=117 bh=117 w=117 h=117 knob=no_big_tiles",
     dict(rc=-5, text="a 117x117 tile needs 171136 B of LDS (limit 163840) and has too many pixels for the HBM-resident form (limit 2^20 - 1)")),
    # shrink_by with its planes: 89x89 is 4 x 46 x 89 + 3 x 89 x 89 + 8 x 46 = 40508 dwords (+ 8 waves' sums: 162160 bytes),
    # 90x90 is 4 x 46 x 90 + 3 x 8100 + 368 = 41228 dwords = 164912 bytes
    ("the ladder's probe: both layouts of 89x89 are in LDS", f"{BY} ladder=1 bw=89 bh=89 w=89 h=89", dict(ladder=1, tile=16376 + 4 * 45 * 46 + 368)),
    ("... of 90x90 the one with planes is not", f"{BY} ladder=1 bw=90 bh=90 w=90 h=90", dict(ladder=0)),
    ("... and never for the directional detector", "ladder=1", dict(ladder=0)),
]

BIG, HUGE = "w=2048 h=1024", "w=4096 h=2048"  # 2048 and 8192 tiles
TRANSPARENCY = [
    ("2047 tiles with transparency seen", f"{BIG} sig=own seen=2047", dict(alpha=0, first=0)),
    ("2048: shrink32a_kernel, and as that is all tiles, it goes first", f"{BIG} sig=own seen=2048", dict(alpha=1, first=1)),
    ("one below half of 8192 tiles", f"{HUGE} sig=own seen=4095", dict(alpha=1, first=0)),
    ("half of them", f"{HUGE} sig=own seen=4096", dict(alpha=1, first=1)),
    ("counts of another configuration are not trusted", f"{HUGE} sig=other seen=5000 listed=7", dict(alpha=0, first=0, listed=UNKNOWN)),
    ("the listed tiles of the last launch size the worklist grid", f"{HUGE} sig=own seen=0 listed=7", dict(alpha=0, listed=7)),
    ("the caller's hint", "hint=1", dict(alpha=1, first=0, listed=UNKNOWN, stats=1)),
    ("quiet: no statistics are written; what is read is read", f"{BIG} sig=own seen=2048 quiet=1", dict(alpha=1, first=1, stats=0)),
]

# 7 rows + 112 bytes must fit 32 bits: 613566740 is the last pitch that does.  RGB rows need 4-byte alignment, RGBA rows 16
PITCH = [
    ("RGB, the last pitch", "c=3 pitch=613566740", dict(input="given", full="2x2")),
    ("RGB, the next aligned one", "c=3 pitch=613566744", dict(input="given", full="0x0", okrows=0)),
    ("an unaligned one is widened into tight rows", "c=3 pitch=613566741", dict(input="widened", pitch=256, full="2x2")),
    ("RGBA, the last aligned pitch", "pitch=613566736", dict(input="given", full="2x2")),
    ("RGBA, the next", "pitch=613566752", dict(input="given", full="0x0")),
    ("shrink_by, whose layout counted on the detector: refused as it always was", f"{BY} pitch=613566752",
     dict(rc=-5, text="internal: Oklab values missing for a layout sized without detector planes")),
]

OUTPUTS = [
    ("no pixels: no transposed planes, no clone_ahead", f"{BY} px=0", dict(tmp=0, tile=T32_BARE, det="rgba", clone=0, slots4=0, factor=16, scale=10)),
    ("lod outputs of the directional detector", "px=0 factor=0.5", dict(tmp=0, tile=T32_BARE, det="none", full="2x2", factor=0.5, scale=10)),
    ("identity: factor 1, scale 1", f"{BY} px=0 factor=0.5 ident=1", dict(factor=1, scale=1, det="rgba")),
    ("RGB without pixels is widened without asking the tables", f"{BY} c=3 low=1 px=0", dict(input="widened", needs_opaque=0, slots4=0)),
    ("Nearest: no convolution", f"{BY} c=3 low=1 filt=0", dict(input="widened", needs_opaque=0, tmp=0, slots4=16384)),
]

REFUSALS = [
    ("1-px edge under the directional detector", "w=33", dict(rc=-4, text="directional detector needs tiles of at least 2x2 px (edge tile is 1x32)")),
    ("... reported before the block side", "w=33 bw=65536 h=33", dict(rc=-4, text="directional detector needs tiles of at least 2x2 px (edge tile is 33x1)")),
    ("block side above 65535", f"{BY} bw=65536", dict(rc=-5, text="block side above 65535")),
    ("more than 2^32 - 1 tiles", f"{BY} bw=1 bh=1 w=65536 h=65536 n=2", dict(rc=-5, text="too many tiles")),
]


@pytest.mark.parametrize("cases", [ALIGNMENT, EDGES, SHAPES, RGB, LDS, TRANSPARENCY, PITCH, OUTPUTS, REFUSALS],
                         ids=["alignment", "edges", "shapes", "rgb", "lds", "transparency", "pitch", "outputs", "refusals"])
def test_routes_at_their_breakpoints(cases):
    check(cases)


# knob -> (the case it is flipped on, the fields that change and their values with the knob; every other field stays)
LAB32 = dict(lab=3072, tile=T32_LAB, lds=T32_LAB * 4)
KNOBS = {
    "no_alpha_kernel": ("hint=1", dict(alpha=0)),
    "no_alpha_first": (f"{HUGE} sig=own seen=4096", dict(first=0)),
    "no_oklab_general": (f"{BY} bw=8 bh=8 w=16 h=16", dict(det="none", full="0x0", okrows=0, lab=192, tile=128 + 192 + 32, lds=(128 + 192 + 32) * 4)),
    "no_oklab32": (BY, dict(det="none", clone=0, **LAB32)),
    "no_oklab_edges": (f"{BY} w=40 h=40", dict(edges=0, r1="0:0", r3="0:0", **LAB32)),
    "no_repitch": ("low=4", dict(input="given", rgba=0, full="0x0", okrows=0)),
    "no_widen": (f"{BY} c=3 low=1", dict(input="given", ch=3, pitch=192, stride=12288, rgba=0, slots4=0, needs_opaque=0, det="none", clone=0, full="0x0",
                                        okrows=0, **LAB32)),
    "no_native_rgb": (f"{BY} c=3", dict(input="widened", ch=4, pitch=256, stride=16384, rgba=16384, slots4=16384, needs_opaque=1, det="rgba", lab=0,
                                       tile=T32, lds=T32 * 4)),
    "no_clone_ahead": (BY, dict(clone=0)),
    "oklab_v1": (f"{BY} bw=64 bh=64 w=128 h=72", dict(clone=0, okscratch=4 * 16 * 3328)),
}


@pytest.mark.parametrize("knob", sorted(KNOBS))
def test_a_knob_flips_its_decision_and_nothing_else(knob):
    line, want = KNOBS[knob]
    base, flipped = routes([line, f"{line} knob={knob}"])
    assert base["rc"] == "0" and flipped["rc"] == "0"
    changed = {k: flipped[k] for k in base if base[k] != flipped[k]}
    assert changed == {k: str(v) for k, v in want.items()}, (knob, base, flipped)


def test_sweep_holds_the_invariants():
    """A: with clone_ahead, every tile a fast kernel may skip was taken by the detector of the same launch; B: a detector runs
    only on frames of at least one block each way; and a layout sized without detector planes has every tile's value covered."""
    assert os.path.exists(TOOL), "run __graft_entry__.build()"
    r = subprocess.run([TOOL, "sweep"], capture_output=True, text=True)
    words = r.stdout.split()
    assert r.returncode == 0 and words[0] == "ok" and int(words[1]) > 10_000_000, r.stdout + r.stderr
