"""The directed inputs of tests/patch_seams.py on the CPU: the restatements of the overlay's and the splice's address arithmetic
stand on their own (against answers made by hand, and the piece list against the model's files, which it must rebuild), and every
input reaches the class it is named for -- the overlay's alignment classes per channel count, the piece counts, the pieces without
bytes, the landings on 16384 * m + d, the capacity cuts -- so that tests/test_gpu_patch_seams.py compares the kernels on inputs that
discriminate."""
import numpy as np
import pytest

import patch_model as pm
import patch_seams as S
from test_gpu_patch import records

GEOMS = {"small": S.SMALL, "long": S.LONG}
MODES = {"by": pm.SHRINK_BY, "directional": pm.DIRECTIONAL}
LDS_LIMIT = 163840


# ---- the restatements ------------------------------------------------------------------------------------------------------------

def test_overlay_classes_by_hand():
    tile = (32, 16, 16, 8)  # tile (2, 2) of 16x8 blocks
    # one RGB pixel a row at column 3: at = (row * 16 + 3) * 3 = 9 (mod 4: 1); the source on 1 (mod 4) agrees, head = the row
    p = S.overlay_classes((35, 17, 1, 2), tile, 3, 8, 33)
    assert [(r.at, r.src_mod, r.same, r.head, r.body, r.tail) for r in p.rows] == [(57, 1, True, 3, 0, 0), (105, 1, True, 3, 0, 0)]
    assert (p.n_rows, p.whole, p.interior) == (2, False, True)
    # ... and one byte on: a byte loop over the row
    p = S.overlay_classes((35, 17, 1, 2), tile, 3, 8, 34)
    assert [(r.same, r.head, r.body, r.tail) for r in p.rows] == [(False, 0, 0, 3)] * 2
    # a pitch of 1 (mod 4): every fourth row agrees.  5 RGB px from column 2: at = 6 (mod 4: 2), head 2, body 3, tail 1
    p = S.overlay_classes((34, 16, 5, 5), tile, 3, 17, 18)
    assert [r.same for r in p.rows] == [True, False, False, False, True]
    assert [(r.head, r.body, r.tail) for r in p.rows if r.same] == [(2, 3, 1)] * 2 and not p.interior
    # the part of a window that began in the tile to the left and above: the source skips 2 rows and 3 pixels
    p = S.overlay_classes((29, 14, 8, 4), tile, 4, 40, 16)
    assert [(r.at, r.src_mod, r.head, r.body, r.tail) for r in p.rows] == [(0, 0, 0, 5, 0), (64, 0, 0, 5, 0)]
    assert S.overlay_classes((32, 16, 16, 8), tile, 4, 64, 0).whole


def test_splice_pieces_by_hand():
    kinds = lambda rects, size=(40, 24): [(p.kind, p.lo, p.hi) for p in S.splice_pieces([size], rects, 8, 8)]  # noqa: E731  (5x3 tiles)
    assert kinds([]) == [("file", ("file_start",), ("file_end",))]
    assert kinds([(0, 9, 9, 2, 2)]) == [("header", ("file_start",), ("row", 0)), ("gap", ("row", 0), ("rec_start", 6)),
                                         ("staging", ("stage", 6), ("stage_end", 6)), ("tail", ("rec_end", 6), ("file_end",))]
    assert kinds([(0, 0, 0, 40, 24)]) == [("header", ("file_start",), ("row", 0))] + [("staging", ("stage", 5 * r), ("stage_end", 5 * r + 4)) for r in range(3)]
    # the last column of row 0, then column 0 of row 1 (no gap), then column 0 of row 2 from a cursor inside row 1 (a gap)
    assert [k[0] for k in kinds([(0, 33, 1, 2, 2), (0, 1, 9, 2, 2), (0, 1, 17, 2, 2)])] == ["header", "gap", "staging", "staging", "gap", "staging", "tail"]


def assemble(call, oracle):
    """the new files put together from the pieces: old bytes, the new files' records, and the new files' line tables"""
    want = call.want(oracle)[0]
    out = []
    for i, s in enumerate(call.sources):
        mine = [p for p in call.pieces(oracle) if p.image == i]
        if [p.kind for p in mine] == ["file"]:
            out.append(s.raw)
            continue
        new_recs = records(want[i])
        got = bytearray()
        for p in mine:
            if p.kind == "staging":
                got += want[i][new_recs[p.lo[1]][0]:new_recs[p.hi[1]][0] + new_recs[p.hi[1]][1]]
            else:
                old_recs = records(s.raw)
                at = {"file_start": lambda b: 0, "file_end": lambda b: len(s.raw), "rec_start": lambda b: old_recs[b[1]][0],
                      "rec_end": lambda b: sum(old_recs[b[1]]),
                      "row": lambda b: old_recs[b[1] * -(-s.w // call.bw)][0] if b[1] * -(-s.w // call.bw) < len(old_recs) else len(s.raw)}
                lo, hi = at[p.lo[0]](p.lo), at[p.hi[0]](p.hi)
                assert hi - lo == p.length
                got += s.raw[lo:hi]
        rows = -(-s.h // call.bh)
        got[26:26 + 4 * rows] = want[i][26:26 + 4 * rows]
        out.append(bytes(got))
    return out


SHAPES = {"many": S.many_pieces, "tall": S.tall, "tall every row": S.tall_every_row, "wrapping": S.wrapping, "flagged": S.flagged}
SHAPE_CONFIGS = {"many": ("rgb-by", "rgba-directional"), "tall": ("rgb-directional", "rgba-by"), "tall every row": ("rgb-by", "rgba-directional"),
                 "wrapping": tuple(S.SPLICE_CONFIGS), "flagged": ("rgb-by", "rgba-directional")}
SHAPE_CASES = [(s, c) for s in SHAPES for c in SHAPE_CONFIGS[s]]


@pytest.mark.parametrize("shape,config", SHAPE_CASES + [("windowed", None)])
def test_the_pieces_rebuild_the_models_files(oracle, product, shape, config):
    """splice_pieces with the record tables' lengths is the splice: old spans and new records in its order are the model's files.
    The windows of every call pass pxz_patch_check."""
    call = S.windowed(oracle) if shape == "windowed" else SHAPES[shape](oracle, config)
    product.patch_check(call.sizes, [r + (0, 0) for r in call.rects], call.bw, call.bh)
    assert assemble(call, oracle) == call.want(oracle)[0]
    assert S.piece_offsets(call.pieces(oracle))[-1] == sum(len(f) for f in call.want(oracle)[0])


# ---- the overlay sweep -----------------------------------------------------------------------------------------------------------

def sweep_rows(oracle, geom, c):
    """every Part of both placements of a geometry (the classes depend on neither the mode nor the pixels)"""
    call = S.overlay_call(oracle, geom, c, pm.DIRECTIONAL)
    parts = []
    for v in S.VARIANTS[geom]:
        windows, _ = S.place(call.specs, call.sizes[0], call.bw, call.bh, c, call.patches, v)
        for w in windows:
            parts += S.overlay_parts(call.sizes[0], call.bw, call.bh, c, w)
    return parts


@pytest.mark.parametrize("c", (3, 4))
def test_overlay_sweep_reaches_its_classes(oracle, product, c):
    parts = sweep_rows(oracle, S.SMALL, c) + sweep_rows(oracle, S.LONG, c)
    rows = [r for p in parts for r in p.rows]
    agree, other = [r for r in rows if r.same], [r for r in rows if not r.same]
    print(f"C={c}: {len(parts)} parts, {len(agree)} agreeing rows, {len(other)} others")
    if c == 3:
        assert {r.head for r in agree} == {0, 1, 2, 3}
        assert any(r.head == r.row_bytes == 3 and r.at & 3 == 1 for r in agree)  # head is the whole row: one RGB pixel
    else:
        # RGBA: at = (row * w + cx0) * 4 is a multiple of 4, so an agreeing row has no head and no tail; there is nothing else to reach
        assert {r.head for r in agree} == {0} and {r.tail for r in agree} == {0} and all(r.at & 3 == 0 for r in rows)
    if c == 3:
        assert any(r.body == 0 and r.tail > 0 for r in agree)
        assert {r.tail for r in agree} == {0, 1, 2, 3}
    assert any(1 <= r.body <= 64 for r in agree) and any(r.body > 64 for r in agree)
    assert any(r.row_bytes <= 64 for r in other) and any(64 < r.row_bytes <= 256 for r in other) and any(r.row_bytes > 256 for r in other)
    assert any(p.n_rows == 1 for p in parts) and any(2 <= p.n_rows <= 3 for p in parts) and any(p.n_rows > 4 for p in parts)
    assert any(p.whole for p in parts) and any(p.interior for p in parts)
    # both paths within one part, and a source class that changes from row to row
    assert any({r.same for r in p.rows} == {True, False} for p in parts)


@pytest.mark.parametrize("c", (3, 4))
def test_small_rows_placement_takes_all_sixteen_classes(oracle, c):
    call = S.overlay_call(oracle, S.SMALL, c, pm.DIRECTIONAL)
    windows, buf = S.place(call.specs, call.sizes[0], call.bw, call.bh, c, call.patches)
    assert {(w[6] & 3, w[5] & 3) for w in windows[:16]} == {(o, p) for o in range(4) for p in range(4)}
    assert {w[1] % 16 for w in windows[:16]} == {0, 1, 2, 3} and {w[3] for w in windows[:16]} == {1, 2, 3, 4, 5, 6}
    heights = {w[4] for w in windows}
    assert 1 in heights and heights & {2, 3} and heights & {5, 6, 7, 8} and max(heights) > 8
    assert any(w[1] % 16 + w[3] == 16 for w in windows) and any(w[1] % 16 + w[3] > 16 and w[1] // 16 < 6 for w in windows)  # to the edge; across a seam
    for (_, x, y, w, h, pitch, off), px in zip(windows, call.patches):  # the pixels stand where the windows say, on poison
        assert pitch >= w * c and (np.lib.stride_tricks.as_strided(buf[off:], (h, w, c), (pitch, c, 1)) == px).all()
    assert (buf == S.POISON).sum() >= S.GUARD * (len(windows) + 1)


@pytest.mark.parametrize("geom", GEOMS)
def test_long_rows_fit_the_reshrink_and_windows_are_disjoint(oracle, product, geom):
    W, H, bw, bh = GEOMS[geom]
    for mode in MODES.values():
        assert 0 < product.reshrink_lds_bytes(bw, bh, mode, pm.LANCZOS3) <= LDS_LIMIT
        assert 0 < product.reshrink_lds_bytes(bw, bh, mode, pm.NEAREST) <= LDS_LIMIT
    call = S.overlay_call(oracle, GEOMS[geom], 3, pm.DIRECTIONAL)
    product.patch_check(call.sizes, [r + (0, 0) for r in call.rects], bw, bh)  # pxz_patch_check is the judge
    assert pm.first_overlap(call.rects, bw, bh) is None
    if geom == "long":
        widths = [r[3] for r in call.rects]
        assert any(65 <= w <= 96 for w in widths) and 96 in widths and 65 in widths


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("c", (3, 4))
@pytest.mark.parametrize("geom", GEOMS)
def test_overlay_sweep_tiles_are_stored_at_full_size(oracle, geom, c, mode):
    """noise under noise at NOISE_FACTOR: every covered tile's stored slot is the tile image, before and after the patch"""
    call = S.overlay_call(oracle, GEOMS[geom], c, MODES[mode])
    W, H, bw, bh = GEOMS[geom]
    cols = -(-W // bw)
    d_old, d_new = oracle.decode_container(call.sources[0].raw), oracle.decode_container(call.want(oracle)[0][0])
    n = 0
    for r in call.rects:
        for t in pm.covered_tiles(r[1:], (W, H), bw, bh):
            full = (min(bw, W - t % cols * bw), min(bh, H - t // cols * bh))
            assert (int(d_old["tw"][t]), int(d_old["th"][t])) == full and (int(d_new["tw"][t]), int(d_new["th"][t])) == full, (r, t)
            n += 1
    _, tw, th, _ = call.want(oracle)[1]
    assert len(tw) == n
    # ... and the patched image IS in the stored slots: the new pixels of the first window can be read back from its first tile
    x, y, w, h = call.rects[0][1:]
    t = pm.covered_tiles(call.rects[0][1:], (W, H), bw, bh)[0]
    tx, ty = t % cols, t // cols
    fw = min(bw, W - tx * bw)
    slot = d_new["slots"][t][:fw * min(bh, H - ty * bh) * c].reshape(-1, fw, c)
    if c == 3:  # (RGBA goes through premultiply and back; RGB bytes are stored as they are)
        ph, pw = min(h, slot.shape[0] - (y - ty * bh)), min(w, fw - (x - tx * bw))
        assert (slot[y - ty * bh:y - ty * bh + ph, x - tx * bw:x - tx * bw + pw] == call.patches[0][:ph, :pw]).all()


def test_fixture_factor_call_covers_resampled_tiles(oracle):
    for c, mode in ((3, pm.SHRINK_BY), (4, pm.DIRECTIONAL)):
        call = S.overlay_call(oracle, S.SMALL, c, mode, fixtures_factors=True)
        _, tw, th, _ = call.want(oracle)[1]
        small = sum(int(a) * int(b) < 16 * 8 and (int(a), int(b)) not in ((5, 8), (16, 3), (5, 3)) for a, b in zip(tw, th))
        d = oracle.decode_container(call.sources[0].raw)
        print(f"C={c}: {small} of {len(tw)} covered tiles are stored small after the patch")
        assert small >= 3 and (d["tw"] < 16).sum() >= 10


# ---- the splice: piece-list shapes -----------------------------------------------------------------------------------------------

def scan_per(n):
    return -(-n // 1024)  # splice_scan_kernel's pieces per thread


@pytest.mark.parametrize("config", SHAPE_CONFIGS["many"])
def test_many_pieces_is_many(oracle, config):
    call = S.many_pieces(oracle, config)
    pieces = call.pieces(oracle)
    n, per = len(pieces), scan_per(len(pieces))
    print(f"{config}: {n} pieces, {per} per thread, {-(-n // per)} busy threads, the last with {n - (-(-n // per) - 1) * per}")
    assert n > 2048 and per >= 2 and n % per != 0 and -(-n // per) < 1024  # a short last thread and idle ones behind it
    assert sum(len(pm.covered_tiles(r[1:], call.sizes[r[0]], S.B, S.B)) for r in call.rects) > 256
    file_order = sorted(call.rects, key=lambda r: (r[0], r[2] // S.B, r[1] // S.B))
    assert call.rects != file_order and [r[0] for r in call.rects] != sorted(r[0] for r in call.rects)
    assert {(r[3], r[4]) for r in call.rects} == {(w, h) for w in (1, 2, 3) for h in (1, 2, 3)}
    assert len({p.length for p in pieces if p.kind == "staging"}) > 4 and len({p.length for p in pieces if p.kind == "gap"}) > 4


@pytest.mark.parametrize("config", SHAPE_CONFIGS["tall"])
def test_tall_reaches_the_line_sums_second_and_third_trip(oracle, config):
    call = S.tall(oracle, config)
    cols, rows = -(-S.TALL[0] // S.B), -(-S.TALL[1] // S.B)
    assert (cols, rows) == (3, 131)
    touched = sorted({r[2] // S.B for r in call.rects})
    assert touched == [0, 63, 64, 65, 127, 128, 130]
    at_cols = {r[1] // S.B for r in call.rects}
    assert at_cols == {0, cols - 1}
    # the row bounds the pieces carry: sums over no entry, over exactly one trip of 64 lanes, over one and two entries of a second
    # trip, over exactly two trips and over one entry of a third
    sums = sorted({b[1] for p in call.pieces(oracle) for b in (p.lo, p.hi) if b[0] == "row"})
    assert sums == [0, 64, 65, 66, 128, 129], sums
    raw = call.sources[0].raw
    table = [int.from_bytes(raw[26 + 4 * r:30 + 4 * r], "big") for r in range(rows)]
    assert min(table) > 0 and len(set(table[64:])) > 4  # no entry is 0, so a sum that drops one is another sum
    every = S.tall_every_row(oracle, config if config in SHAPE_CONFIGS["tall every row"] else SHAPE_CONFIGS["tall every row"][0])
    assert len({(r[0], r[2] // S.B) for r in every.rects}) == 262 and {r[1] // S.B for r in every.rects} == {0, 1, 2}
    sums = {b[1] for p in every.pieces(oracle) for b in (p.lo, p.hi) if b[0] == "row"}
    assert len(sums) > 40 and max(sums) > 128


@pytest.mark.parametrize("config", SHAPE_CONFIGS["wrapping"])
def test_wrapping_reaches_its_piece_shapes(oracle, config):
    call = S.wrapping(oracle, config)
    pieces = call.pieces(oracle)
    cols = 5
    by_lo = {p.lo: p for p in pieces}
    gap = by_lo[("rec_end", 1 * cols + 1)]  # behind tile (1, 1), up to its neighbour (2, 1)
    assert gap.kind == "gap" and gap.hi == ("rec_start", 1 * cols + 2) and gap.length == 0
    gap = by_lo[("rec_end", 4 * cols + 0)]  # the one-row window at column 0 of row 4, then the tall one from column 1
    assert gap.hi == ("rec_start", 4 * cols + 1) and gap.length == 0
    kinds = [p.kind for p in pieces]
    assert kinds[:2] == ["header", "staging"]  # column 0 of row 0
    k = pieces.index(by_lo[("stage", 2 * cols)])  # column 0 of row 2 behind a window that ended in the last column of row 1
    assert pieces[k - 1].kind == "staging" and pieces[k - 1].hi == ("stage_end", 1 * cols + 4)
    assert kinds[-1] == "staging" and "tail" not in kinds
    row1 = [p for p in pieces if p.kind == "staging" and p.lo[1] // cols == 1]
    assert len(row1) == 3
    assert [p.lo[1] // cols for p in pieces if p.kind == "staging" and p.hi[1] - p.lo[1] == 1] == [3, 4, 5]  # the three-row window
    assert sum(p.length == 0 for p in pieces) == 2 and all(p.length > 0 for p in pieces if p.kind != "gap")


@pytest.mark.parametrize("config", SHAPE_CONFIGS["flagged"])
def test_flagged_file_has_a_run_of_pieces(oracle, config):
    call = S.flagged(oracle, config)
    pieces = call.pieces(oracle)
    mine = [k for k, p in enumerate(pieces) if p.image == 2]
    assert len(mine) >= 7 and mine == list(range(mine[0], mine[-1] + 1)) and 0 < mine[0] and mine[-1] < len(pieces) - 1
    assert call.rects[S.FLAGGED_WINDOW][0] == 2 and len(pm.covered_tiles(call.rects[S.FLAGGED_WINDOW][1:], call.sizes[2], S.B, S.B)) == 1
    assert [p.kind for p in pieces if p.image == 3] == ["header", "staging"]  # a file of one covered tile: no gap, no tail


# ---- the splice: chunk, alignment and capacity sweeps ----------------------------------------------------------------------------

def test_windowed_file_has_every_kind_of_piece(oracle):
    call = S.windowed(oracle)
    pieces = call.pieces(oracle)
    assert [p.kind for p in pieces] == ["header", "staging", "gap", "staging", "tail"]  # (the corner is the image's: rows 0..1 from column 0)
    assert all(p.length > 17 for p in pieces) and S.piece_offsets(pieces)[-1] == len(call.want(oracle)[0][0])
    assert call.want(oracle)[0][0] != call.sources[0].raw


def test_filler_is_a_valid_file_with_padding_in_its_span(oracle, product):
    f = S.windowed(oracle).fixture
    small = S.filler(oracle, f.c, f.bw, f.bh, S.min_filler(oracle))
    assert product.file_header(small.raw)[:5] == (4, 4, f.bw, f.bh, f.c)
    d = oracle.decode_container(small.raw)
    assert (int(d["tw"][0]), int(d["th"][0])) != (0, 0) and len(records(small.raw)) == 1
    big = S.filler(oracle, f.c, f.bw, f.bh, 20000)
    assert len(big.raw) == 20000 and big.raw[:len(small.raw)] == small.raw and len(set(big.raw[len(small.raw):])) > 100
    call = S.behind_filler(oracle, 20000)
    assert [p.kind for p in call.pieces(oracle)][:2] == ["file", "header"] and call.pieces(oracle)[0].length == 20000
    assert call.want(oracle)[0] == [big.raw, S.windowed(oracle).want(oracle)[0][0]]


@pytest.mark.parametrize("d", S.SEAM_DELTAS)
@pytest.mark.parametrize("which", S.SEAM_BOUNDARIES)
def test_seam_fillers_land_the_boundary(oracle, which, d):
    call = S.behind_filler(oracle, S.seam_filler_length(oracle, which, d))
    pieces = call.pieces(oracle)
    offs = S.piece_offsets(pieces)
    k = {"file start": 1, "staging start": [p.kind for p in pieces].index("staging"),
         "staging end": len(pieces) - 1 - [p.kind for p in pieces][::-1].index("staging") + 1}[which]
    assert pieces[k - 1].kind == {"file start": "file", "staging start": "header", "staging end": "staging"}[which]
    assert offs[k] % S.CHUNK == d % S.CHUNK and offs[k] - d > 0
    spans = S.copy_spans(offs)
    assert pieces[k - 1].length > 17 and pieces[k].length > 17
    if d == 0:  # the boundary ON a chunk's end: the chunk ends with the piece before it, the next begins with the piece behind
        assert any(p == k - 1 and b == offs[k] for (p, a, b, *_) in spans) and not any(p == k and a < offs[k] + 1 < b and a != offs[k] for (p, a, b, *_) in spans)
        assert any(p == k and a == offs[k] and head == 0 for (p, a, b, head, body, tail) in spans)
    if d > 0:   # the piece before the boundary is cut by the chunk, and its last span has d bytes
        assert (k - 1, offs[k] - d, offs[k], 0, d >> 4, d & 15) in spans
    if d < 0:   # the piece behind it has its first -d bytes in this chunk
        assert any(p == k and a == offs[k] and b == offs[k] - d for (p, a, b, *_) in spans)


def test_seam_sweep_sees_every_head_and_tail_length_at_a_chunks_ends(oracle):
    seen_head, seen_tail, seen_bytes = set(), set(), set()
    for which in S.SEAM_BOUNDARIES:
        for d in S.SEAM_DELTAS:
            offs = S.piece_offsets(S.behind_filler(oracle, S.seam_filler_length(oracle, which, d)).pieces(oracle))
            for (p, a, b, head, body, tail) in S.copy_spans(offs):
                if a % S.CHUNK == 0 or b % S.CHUNK == 0:
                    seen_head.add(head), seen_tail.add(tail), seen_bytes.add(b - a)
    assert {1, 15, 16, 17} <= seen_bytes and {0, 1, 15} <= seen_head and {0, 1, 15} <= seen_tail


def test_alignment_sweep_sees_every_destination_alignment(oracle):
    length = S.ALIGN_FILLER
    offs = S.piece_offsets(S.behind_filler(oracle, length).pieces(oracle))
    for skew in range(16):
        heads = {head for (p, a, b, head, body, tail) in S.copy_spans(offs, skew=skew)}
        assert len(heads) >= 4
    starts = {(o + skew) % 16 for o in offs[:-1] for skew in range(16)}
    assert starts == set(range(16))
    # the files' own alignment: with lead in ALIGN_LEADS the old spans start on several classes against each destination
    assert len({(lead + length) % 16 for lead in S.ALIGN_LEADS}) == len(S.ALIGN_LEADS) == 4


def test_capacity_sweep_cuts_head_body_tail_boundary_and_line_table(oracle):
    cap = S.cap_filler(oracle)
    call = S.behind_filler(oracle, cap)
    pieces = call.pieces(oracle)
    offs = S.piece_offsets(pieces)
    longest = max(range(len(pieces)), key=lambda k: pieces[k].length)
    assert offs[longest] % 16 == 1 and longest > 0  # a head of 15 bytes in the longest piece
    caps = S.capacities(oracle, cap)
    assert all(0 <= c <= offs[-1] for c in caps)
    for o in offs[1:-1]:
        assert {o - 1, o, o + 1} <= set(caps)
    assert offs[-1] - 1 in caps and offs[-1] in caps
    cut = {"head": 0, "body": 0, "tail": 0, "boundary": 0, "line table": 0}
    for c in caps:
        full = {s[0]: s for s in S.copy_spans(offs) if s[1] <= c < s[2]}
        if c in offs:
            cut["boundary"] += 1
        for (p, a, b, head, body, tail) in S.copy_spans(offs, capacity=c):
            if b == c and c not in offs:  # the span the capacity ends in, against the same span uncut
                _, fa, fb, fhead, fbody, ftail = full[p]
                where = c - fa
                cut["head" if where < fhead else "body" if where < fhead + 16 * fbody else "tail"] += 1
        if cap + 26 <= c < cap + 26 + 4 * call.sources[1].h // call.bh:
            cut["line table"] += 1
    print(cut)
    assert all(n > 0 for n in cut.values()), cut
    row = pm.covered(call.rects[0][1:5], call.bw, call.bh)[1]
    assert {cap + 26 + 4 * row + b for b in range(5)} <= set(caps)
