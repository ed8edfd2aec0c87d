"""The overlay of patch_kernel and the splice (pxz_patch.hip, the piece list in pxz_api.cpp) on the directed inputs of
tests/patch_seams.py: every alignment class of the per-row copy, rows longer than one wave trip, piece lists of more than 2048
pieces, of 131 tile rows and of every shape the host loop has a branch for, a flagged file between good ones, and piece boundaries
swept across the 16 KB chunks, the 16-byte stores and the capacity.  Every comparison is exact and against test_gpu_patch.model(),
the oracle's expand, overlay, shrink and container writer; tests/test_patch_seams_host.py asserts on the CPU that each input
reaches the class it is named for."""
import numpy as np
import pytest

import patch_model as pm
import patch_seams as S
from test_gpu_patch import Chain, GUARD, POISON, host_form, same_tiles

pytestmark = pytest.mark.gpu

GEOMS = {"small": S.SMALL, "long": S.LONG}
MODES = {"by": pm.SHRINK_BY, "directional": pm.DIRECTIONAL}
SHAPES = {"many": S.many_pieces, "tall": S.tall, "tall every row": S.tall_every_row, "wrapping": S.wrapping}
SHAPE_CONFIGS = {"many": ("rgb-by", "rgba-directional"), "tall": ("rgb-directional", "rgba-by"), "tall every row": ("rgb-by", "rgba-directional"),
                 "wrapping": tuple(S.SPLICE_CONFIGS)}


@pytest.fixture(scope="module")
def gpu(product):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    h = product.Handle(0)
    yield h
    h.close()


def run(gpu, product, call, **kw):
    return Chain(gpu, product, call.sources, call.c, call.bw, call.bh, call.p, call.rects, call.patches, **kw)


def clean(ch):
    assert ch.status == 0
    for flags in (ch.rflags, ch.pflags, ch.iflags):
        assert (flags.cpu().numpy() == 0).all()


def patch_untouched(ch):
    assert ch.patch.data_ptr() % 16 == 0  # what overlay_classes takes the source's alignment from
    assert (ch.patch.cpu().numpy() == ch.host_patch).all()


# ---- the overlay sweep -----------------------------------------------------------------------------------------------------------

def overlay_sweep(gpu, product, oracle, call, geom):
    want_files, want_tiles = call.want(oracle)
    for k, v in enumerate(S.VARIANTS[geom]):
        for in_place in (False, True)[:1 + k]:  # the last placement again in place
            placement = S.place(call.specs, call.sizes[0], call.bw, call.bh, call.c, call.patches, v)
            ch = run(gpu, product, call, placement=placement, in_place=in_place)
            clean(ch)
            same_tiles(ch.new_host, want_tiles, call.c, f"placement {v}, in place {in_place}")
            assert ch.file(0) == want_files[0], f"placement {v}, in place {in_place}"
            patch_untouched(ch)
            if in_place:
                assert ch.new[3].data_ptr() == ch.old[3].data_ptr()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("c", (3, 4))
@pytest.mark.parametrize("geom", GEOMS)
def test_overlay_sweep(gpu, product, oracle, geom, c, mode):
    """noise under noise: every covered tile is stored at full size, so each byte the overlay wrote or left is compared"""
    overlay_sweep(gpu, product, oracle, S.overlay_call(oracle, GEOMS[geom], c, MODES[mode]), GEOMS[geom])


def test_overlay_sweep_nearest(gpu, product, oracle):
    overlay_sweep(gpu, product, oracle, S.overlay_call(oracle, S.SMALL, 4, pm.DIRECTIONAL, filt=pm.NEAREST), S.SMALL)


@pytest.mark.parametrize("c,mode", ((3, "by"), (4, "directional")))
def test_overlay_sweep_over_resampled_tiles(gpu, product, oracle, c, mode):
    """the fixtures' picture and factors: covered tiles that are expanded before and resampled after the overlay"""
    overlay_sweep(gpu, product, oracle, S.overlay_call(oracle, S.SMALL, c, MODES[mode], fixtures_factors=True), S.SMALL)


# ---- the splice: piece-list shapes -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape,config", [(s, c) for s in SHAPES for c in SHAPE_CONFIGS[s]])
def test_piece_list_shapes(gpu, product, oracle, shape, config):
    call = SHAPES[shape](oracle, config)
    want_files, want_tiles = call.want(oracle)
    ch = run(gpu, product, call)
    clean(ch)
    same_tiles(ch.new_host, want_tiles, call.c, shape)
    got = [ch.file(i) for i in range(len(call.sources))]
    for i, (g, w) in enumerate(zip(got, want_files)):
        if g != w:
            a, b = np.frombuffer(g, np.uint8), np.frombuffer(w, np.uint8)
            n = min(len(a), len(b))
            first = int(np.nonzero(a[:n] != b[:n])[0][0]) if (a[:n] != b[:n]).any() else n
            offs = S.piece_offsets([p for p in call.pieces(oracle) if p.image == i])
            pytest.fail(f"{shape}: file {i} has {len(g)} bytes for {len(w)} and differs from byte {first}, in piece {int(np.searchsorted(offs, first, 'right')) - 1} of its {len(offs) - 1}")
    assert ch.o.tolist() == [0] + np.cumsum([len(w) for w in want_files]).tolist()
    assert host_form(gpu, call.sources, call.bw, call.bh, call.p, call.rects, call.patches) == want_files


@pytest.mark.parametrize("config", ("rgb-by", "rgba-directional"))
def test_a_flagged_file_between_good_ones(gpu, product, oracle, config):
    """a stored width of the middle file's second window zeroed behind the reader: that file comes out empty, its seven pieces
    without bytes between the others', and the four other files are the model's"""
    call = S.flagged(oracle, config)
    want_files, want_tiles = call.want(oracle)
    to = product.patch_check(call.sizes, [r + (0, 0) for r in call.rects], call.bw, call.bh)
    ch = run(gpu, product, call, break_tile=int(to[S.FLAGGED_WINDOW]))
    assert ch.status == 1 and (ch.rflags.cpu().numpy() == 0).all()
    assert ch.pflags.cpu().numpy().tolist() == [int(k == S.FLAGGED_WINDOW) for k in range(len(call.rects))]
    assert ch.iflags.cpu().numpy().tolist() == [0, 0, 1, 0, 0]
    assert int(ch.o[2]) == int(ch.o[3])
    for i in (0, 1, 3, 4):
        assert ch.file(i) == want_files[i], i
    sizes = [len(w) for w in want_files]
    sizes[2] = 0
    assert ch.o.tolist() == [0] + np.cumsum(sizes).tolist()
    keep = [t for t in range(int(to[-1])) if not int(to[2]) <= t < int(to[5])]  # the tiles of the other files' windows
    same_tiles(tuple(a[keep] for a in ch.new_host), tuple(a[keep] for a in want_tiles), call.c, "the other files' tiles")


# ---- the splice: chunk, alignment and capacity sweeps ----------------------------------------------------------------------------

def spliced(gpu, product, call, want_files, skew=0, capacity=None, lead=3):
    """the chain into a view that starts `skew` bytes behind a multiple of 16 and holds `capacity` bytes (default: what the files
    need), poison around it: the offsets are the full sizes, the view holds the expected bytes up to the capacity, and every byte
    before the view and at or beyond the capacity is still poison"""
    import torch
    expect = b"".join(want_files)
    total = len(expect)
    cap = total if capacity is None else capacity
    whole = torch.full((GUARD + 16 + max(cap, total) + GUARD,), POISON, dtype=torch.uint8, device="cuda")
    assert whole.data_ptr() % 16 == 0
    view = whole[GUARD + skew:GUARD + skew + cap]
    assert view.data_ptr() % 16 == skew
    offs = torch.full((len(call.sources) + 1,), -1, dtype=torch.int64, device="cuda")
    ch = run(gpu, product, call, out=(offs, view), lead=lead)
    clean(ch)
    got = whole.cpu().numpy()
    what = (skew, capacity, lead)
    assert ch.o.tolist() == [0] + np.cumsum([len(f) for f in want_files]).tolist(), what
    n = min(cap, total)
    same = got[GUARD + skew:GUARD + skew + n] == np.frombuffer(expect, np.uint8)[:n]
    assert same.all(), (what, "first wrong byte", int(np.nonzero(~same)[0][0]))
    assert (got[:GUARD + skew] == POISON).all() and (got[GUARD + skew + n:] == POISON).all(), what
    return ch


@pytest.mark.parametrize("which", S.SEAM_BOUNDARIES)
def test_piece_boundaries_around_a_chunks_end(gpu, product, oracle, which):
    """the windowed file's first byte, the start of a staging piece and the end of one on 16384 * m + d for every d"""
    for d in S.SEAM_DELTAS:
        call = S.behind_filler(oracle, S.seam_filler_length(oracle, which, d))
        spliced(gpu, product, call, call.want(oracle)[0])


@pytest.mark.parametrize("lead", S.ALIGN_LEADS)
def test_every_destination_alignment(gpu, product, oracle, lead):
    """the output view 0..15 bytes behind a multiple of 16, the files `lead` bytes behind one"""
    call = S.behind_filler(oracle, S.ALIGN_FILLER)
    expect = call.want(oracle)[0]
    for skew in range(16):
        spliced(gpu, product, call, expect, skew=skew, lead=lead)


def test_capacities(gpu, product, oracle):
    """a capacity on every piece boundary and a byte either side, inside the longest piece's head and body, and inside a touched
    row's entry of the line table"""
    length = S.cap_filler(oracle)
    call = S.behind_filler(oracle, length)
    expect = call.want(oracle)[0]
    for capacity in sorted(S.capacities(oracle, length)):
        spliced(gpu, product, call, expect, capacity=capacity)
