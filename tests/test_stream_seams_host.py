"""The position sweeps of tests/stream_seams.py on the CPU, with the oracle alone: the cases are what they claim to be (they
round-trip, literals cost full ops, an eviction costs a literal, a run's length steps at its flushes, the index-walk rows
reach every wanted header offset), so that tests/test_gpu_stream_seams.py compares the kernels on inputs that discriminate."""
import numpy as np
import pytest

import stream_seams as S

CASES_64 = [(w, h, c, fam) for (w, h, _) in S.SIZES_64 for c in (4, 3) for fam in S.families_of(c)]
CASES_128 = [(w, h, c, fam, k) for (w, h, _) in S.SIZES_128 for c in (4, 3) for fam in S.FAMILIES_128[c]
             for k in range(len(S.parts_of(w, h, 128 * 128 * c)))]


def round_trip(oracle, fr, what):
    d = oracle.decode_container(fr.encode(oracle))
    assert (d["tw"] == fr.tw).all() and (d["th"] == fr.th).all(), what
    assert (d["values"].view(np.uint32) == fr.values.view(np.uint32)).all(), what
    bad = (d["slots"][:, : fr.slots.shape[1]] != fr.slots) & fr.valid()
    assert not bad.any(), f"{what}: tile {int(np.nonzero(bad.any(axis=1))[0][0])}"


@pytest.mark.parametrize("w,h,c,fam", CASES_64, ids=lambda v: str(v).replace(" ", "_"))
def test_sweeps_of_64x64_slots_round_trip_through_the_oracle(oracle, w, h, c, fam):
    round_trip(oracle, S.sweep_frame(fam, w, h, 64, c, S.positions_of(w, h)), f"{fam} {w}x{h} c{c}")


@pytest.mark.parametrize("w,h,c,fam,k", CASES_128, ids=lambda v: str(v).replace(" ", "_"))
def test_sweeps_of_128x128_slots_round_trip_through_the_oracle(oracle, w, h, c, fam, k):
    round_trip(oracle, S.sweep_frame(fam, w, h, 128, c, S.parts_of(w, h, 128 * 128 * c)[k]), f"{fam} {w}x{h} c{c} part {k}")


@pytest.mark.parametrize("c", [4, 3])
def test_mixed_frame_round_trips_and_deals_every_sweep(oracle, c):
    fr, labels = S.mixed_frame("odd one", c)
    assert len(labels) == sum(w * h + 1 for (w, h) in S.MIXED_SIZES)
    assert [l[:2] for l in labels[:5]] == S.MIXED_SIZES  # dealt in turn
    for (w, h) in S.MIXED_SIZES:
        assert [k for (a, b, k) in labels if (a, b) == (w, h)] == list(range(w * h + 1))
    round_trip(oracle, fr, f"mixed c{c}")


def test_sweep_positions():
    """every p in 0..n, but for 128x128: 0..600, n-600..n and seven around every multiple of 256"""
    for (w, h, _) in S.SIZES_64 + S.SIZES_128[1:]:
        assert S.positions_of(w, h) == list(range(w * h + 1))
    p = S.positions_of(128, 128)
    assert set(range(601)) <= set(p) and set(range(16384 - 600, 16385)) <= set(p)
    assert all(k * 256 + d in p for k in range(1, 64) for d in range(-3, 4))
    for (w, h, _) in S.SIZES_128:
        for c in (4, 3):
            parts = S.parts_of(w, h, 128 * 128 * c)
            assert sum(parts, []) == S.positions_of(w, h)                      # nothing left out, nothing twice
            assert all(len(q) * 128 * 128 * c <= 128 << 20 for q in parts)     # what one case uploads


def op_bytes(oracle, px, w, h):
    """the op bytes of a tile's QOI stream: without the 14-byte header and the 8-byte end marker"""
    return len(oracle.qoi_encode(px.reshape(h, w, -1))) - 14 - 8


@pytest.mark.parametrize("c", [4, 3])
def test_literal_pixels_cost_a_full_op_each(oracle, c):
    for (w, h) in [(s[0], s[1]) for s in S.SIZES_64 + S.SIZES_128]:
        n = w * h
        assert op_bytes(oracle, S.literals(n, c), w, h) >= n * (c + 1) - 8, (w, h)
    # ... and wherever they start: behind a run of any length the literals still cost a full op each
    w, h = 17, 15
    n = w * h
    tiles = S.sweep("run|lit", n, c, range(n + 1))
    for p in range(1, n):
        assert op_bytes(oracle, tiles[p], w, h) >= (c + 1) + (n - p) * (c + 1), p


@pytest.mark.parametrize("c", [4, 3])
@pytest.mark.parametrize("w,h", [(s[0], s[1]) for s in S.SIZES_64])
def test_an_eviction_costs_a_literal(oracle, w, h, c):
    """pixel p's own colour is evicted at p and due again at p + 3: the intruder and the colour's return are literals where
    the plain cycle has two INDEX ops of one byte -- 2 c bytes more; c more where the tile ends before the colour returns"""
    n = w * h
    tiles = S.sweep("evict", n, c, range(n + 1))
    plain = op_bytes(oracle, tiles[n], w, h)
    assert plain == 3 * (c + 1) + (n - 3)
    got = np.array([op_bytes(oracle, tiles[p], w, h) for p in range(n)])
    assert (got[3:] > plain).all()
    assert (got[3:n - 3] == plain + 2 * c).all() and (got[n - 3:] == plain + c).all()


def runs(k):
    """the bytes of k repeats: one per 62"""
    return -(-k // 62)


@pytest.mark.parametrize("c,fam", [(c, f) for c in (4, 3) for f in S.families_of(c) if f.startswith("run|run")])
@pytest.mark.parametrize("w,h", [(s[0], s[1]) for s in S.SIZES_64 + S.SIZES_128[1:2]])
def test_run_lengths_step_at_the_flushes(oracle, w, h, c, fam):
    """colour A costs one op and p - 1 repeats (opaque black: p repeats of the implicit previous pixel; (0, 0, 0, 0): an INDEX
    hit of one byte and p - 1 repeats), colour B one op and n - p - 1 repeats; repeats cost a byte per 62 started"""
    n = w * h
    tiles = S.sweep(fam, n, c, range(n + 1))
    got = np.array([op_bytes(oracle, tiles[p], w, h) for p in range(n + 1)])
    lit = c + 1
    first = {"run|run": lambda p: lit + runs(p - 1), "run|run black": lambda p: runs(p), "run|run zero": lambda p: 1 + runs(p - 1)}[fam]
    exp = np.array([(first(p) if p else 0) + (lit + runs(n - p - 1) if p < n else 0) for p in range(n + 1)])
    assert (got == exp).all(), np.nonzero(got != exp)[0][:8]
    assert len(set(np.diff(got[1:n]))) > 1 or n < 64  # it does step


def test_index_walk_rows_reach_every_header_offset(oracle):
    for which in (1, 2):
        fr, seam = S.walk_frame(oracle, which)
        assert fr.rows == len(S.SEAM_OFFSETS) and fr.T == fr.m
        recs = S.records_of(fr.encode(oracle), fr.cols, fr.rows)
        starts = [recs[r * fr.cols + seam][0] for r in range(fr.rows)]
        assert starts == [which * S.CHUNK + d for d in S.SEAM_OFFSETS]
        assert starts[0] == which * 8192 - 40 and starts[-1] == which * 8192 + 8
        if which == 2:
            assert all(recs[r * fr.cols + 2][0] == S.CHUNK for r in range(fr.rows))  # the second chunk starts here
        round_trip(oracle, fr, f"walk rows {which}")


@pytest.mark.parametrize("cols", S.BATCH_COLS)
def test_batch_rows_round_trip(oracle, cols):
    fr = S.batch_frame(cols)
    assert fr.T == fr.m == 3 * cols and (fr.tw == 1).all() and (fr.th == 1).all()
    assert len(np.unique(fr.slots[:, :4], axis=0)) == fr.T
    round_trip(oracle, fr, f"{cols} columns")
    wins, cover = S.seam_windows(fr, S.batch_seams(cols))
    assert cover and all(0 <= a <= b < cols for (_, a, b) in cover)
    ends = {b for (_, _, b) in cover}
    assert cols - 1 in ends and all(s in ends and s - 1 in ends for s in (64, 128, 192) if s < cols)
