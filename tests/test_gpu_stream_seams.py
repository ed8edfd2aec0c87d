"""The device .pixlzr writer (qoi_tiles_kernel, qoi_splice_kernel) and reader (the index pass, qoi_decode_kernel) on the position
sweeps of tests/stream_seams.py: one event at EVERY pixel position of a stored size, one tile per position, so that every seam
between two segments of the writer, whatever the segmentation of that size is, meets a run's end, a run's start, a flush at 62,
a run of one, an index eviction and the end of the tile -- and every 8-byte window alignment and refill of the reader meets the
change between ops of no bytes and ops of five.  The reader's index pass gets rows whose records are sized (lengths measured
with the oracle's encoder) so that a record header starts at every offset around the end of its first and of its second staged
chunk, and rows of 63 .. 200 records around its batches of 64.

Every comparison is byte for byte (values as bits) against the oracle: oracle.encode_container for the writer; for the reader the
ORACLE's bytes go in, so it does not depend on the writer being right.  A failure names the family, the stored size, p and the
first differing byte.  No kernel constant is imported; the sizes are literal lists in tests/stream_seams.py, each with its why.

A sweep is built once (module-scoped `case`) and used by the writer and the reader test in turn."""
import numpy as np
import pytest

import stream_seams as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu(product):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    h = product.Handle(0)
    yield h
    h.close()


# ---- the cases ---------------------------------------------------------------------------------------------------------

CASES = [("64", w, h, c, fam, 0) for (w, h, _) in S.SIZES_64 for c in (4, 3) for fam in S.families_of(c)]
CASES += [("128", w, h, c, fam, k) for (w, h, _) in S.SIZES_128 for c in (4, 3) for fam in S.FAMILIES_128[c]
          for k in range(len(S.parts_of(w, h, 128 * 128 * c)))]
CASES += [("mixed", 0, 0, c, fam, 0) for c in (4, 3) for fam in S.families_of(c)]
# the reader at byte offsets 1..7 as well: one family (and channel count) per stored size
SHIFTED = dict(zip([(w, h) for (w, h, _) in S.SIZES_64], [("run|lit", 4), ("lit|run", 3), ("evict", 4), ("grad|run", 3), ("odd one", 4),
                                                           ("run|run", 3), ("run|run zero", 4)]))
SHIFTED.update({(w, h): ("run|lit", 4) for (w, h, _) in S.SIZES_128})
assert len(SHIFTED) == len(S.SIZES_64) + len(S.SIZES_128)


def case_id(v):
    kind, w, h, c, fam, k = v
    return f"{kind}-{w}x{h}-c{c}-{fam.replace(' ', '_')}-{k}"


class Case:
    """one frame: its tiles, the oracle's file, and both on the device"""

    def __init__(self, oracle, frame, what, label, param=None):
        import torch
        self.fr, self.what, self.label, self.param = frame, what, label, param
        self.raw = frame.encode(oracle)
        self.slots = torch.from_numpy(frame.slots).cuda()
        self.tw = torch.from_numpy(frame.tw.astype(np.int32)).cuda()
        self.th = torch.from_numpy(frame.th.astype(np.int32)).cuda()
        self.vals = torch.from_numpy(frame.values).cuda()
        self.ref = torch.frombuffer(bytearray(self.raw), dtype=torch.uint8).cuda()  # exactly as long as the file
        self.shape = (1, frame.H, frame.W, frame.c)

    def first_bad_record(self, got):
        """the first tile whose record in `got` (a file as the device wrote it) is not the oracle's: both files are walked by
        their own length fields, so a record of another length does not hide what comes behind the line table"""
        fr, ref = self.fr, np.frombuffer(self.raw, np.uint8)
        pg = pr = 26 + 4 * fr.rows
        for t in range(fr.T):
            if pg + 13 > got.size:
                return f"tile {t} ({self.label(t)}): the file ends before its record"
            lg = 13 + int.from_bytes(got[pg + 9:pg + 13].tobytes(), "big")
            lr = 13 + int.from_bytes(ref[pr + 9:pr + 13].tobytes(), "big")
            a, b = got[pg:pg + lg], ref[pr:pr + lr]
            k = min(a.size, b.size)
            diff = np.nonzero(a[:k] != b[:k])[0]
            if diff.size or lg != lr:
                at = int(diff[0]) if diff.size else k
                return (f"tile {t} ({self.label(t)}): record of {lg} bytes, oracle {lr}; first differing byte {at} of the record"
                        + (f": {int(a[at])}, oracle {int(b[at])}" if at < k else ""))
            pg, pr = pg + lg, pr + lr
        return "every record equal: the file header or the line table differs"


def sweep_label(fam, w, h, positions):
    return lambda t: f"{fam} {w}x{h} p={positions[t]}" if t < len(positions) else "spare 1x1"


def build_case(oracle, v):
    kind, w, h, c, fam, k = v
    if kind == "mixed":
        fr, labels = S.mixed_frame(fam, c)
        return Case(oracle, fr, case_id(v), lambda t: f"{fam} {labels[t][0]}x{labels[t][1]} p={labels[t][2]}" if t < len(labels) else "spare 1x1", v)
    slot = int(kind)
    positions = S.parts_of(w, h, slot * slot * c)[k] if slot == 128 else S.positions_of(w, h)
    return Case(oracle, S.sweep_frame(fam, w, h, slot, c, positions), case_id(v), sweep_label(fam, w, h, positions), v)


@pytest.fixture(scope="module", params=CASES, ids=case_id)
def case(request, oracle):
    import torch
    yield build_case(oracle, request.param)
    torch.cuda.empty_cache()


# ---- the checks ----------------------------------------------------------------------------------------------------------

def check_writer(gpu, cs):
    import torch
    fr = cs.fr
    offs, buf = gpu.encode_frames_device(cs.shape, fr.bw, fr.bh, cs.vals, cs.tw, cs.th, cs.slots)
    torch.cuda.synchronize()
    offs = offs.cpu().numpy().tolist()
    n = len(cs.raw)
    got = buf[: min(n, buf.numel())]
    if offs != [0, n] or got.numel() != n or not torch.equal(got, cs.ref):
        g = buf[: offs[1] if 0 <= offs[1] <= buf.numel() else buf.numel()].cpu().numpy()
        r = np.frombuffer(cs.raw, np.uint8)
        k = min(g.size, r.size)
        diff = np.nonzero(g[:k] != r[:k])[0]
        raise AssertionError(f"{cs.what}: offsets {offs}, oracle [0, {n}]; first differing byte of the file: "
                             f"{int(diff[0]) if diff.size else k}; {cs.first_bad_record(g)}")


def check_reader(gpu, cs, files, what):
    """decode_frames_device on `files` (the oracle's bytes, wherever they lie): value bits, sizes, the valid bytes of every slot"""
    import torch
    fr = cs.fr
    offs = torch.tensor([0, len(cs.raw)], dtype=torch.int64).cuda()
    vals, ow, oh, slots = gpu.decode_frames_device(files, offs, cs.shape, fr.bw, fr.bh)
    torch.cuda.synchronize()
    assert gpu.decode_status() == 0, f"{cs.what} {what}: status {gpu.decode_status()}"
    bad_size = (ow[0] != cs.tw) | (oh[0] != cs.th)
    if bad_size.any():
        t = int(torch.nonzero(bad_size)[0])
        raise AssertionError(f"{cs.what} {what}: tile {t} ({cs.label(t)}) read as {int(ow[0, t])}x{int(oh[0, t])}")
    bad_val = vals[0].view(torch.int32) != cs.vals.view(torch.int32)
    assert not bad_val.any(), f"{cs.what} {what}: value bits of tile {int(torch.nonzero(bad_val)[0])}"
    valid = torch.arange(slots.shape[-1], device=slots.device)[None, :] < (cs.tw.long() * cs.th.long() * fr.c)[:, None]
    bad = (slots[0] != cs.slots) & valid
    if bad.any():
        t = int(torch.nonzero(bad.any(dim=1))[0])
        b = int(torch.nonzero(bad[t])[0])
        raise AssertionError(f"{cs.what} {what}: tile {t} ({cs.label(t)}): first differing byte {b} (pixel {b // fr.c}): "
                             f"{int(slots[0, t, b])}, stored {int(cs.slots[t, b])}")


def shifted(ref, shift):
    """the same bytes `shift` bytes into an allocation of their own, ending with the tensor"""
    import torch
    whole = torch.zeros(shift + ref.numel(), dtype=torch.uint8, device="cuda")
    whole[shift:] = ref
    return whole[shift:]


# ---- writer and reader on every sweep -----------------------------------------------------------------------------------

def test_device_writer_on_a_sweep(gpu, case):
    """The tiles of one sweep (one stored size: one class per call, beside the 1x1 spares) as one frame through encode_frames_device: file offsets
    and bytes equal oracle.encode_container.  The image is cols*bw x rows*bh, spare tiles of the last row are 1x1.  The 64x64
    sweeps hold 4097 tiles: they also cross the 4096-tile blocks of the binning and of the scan of the record lengths (the pack
    scans).  The `mixed` cases deal the 64x64, 40x25, 50x41, 13x10 and 9x7 sweeps of one family tile by tile into one call:
    partly filled units, a class change inside the permutation, 7344 tiles."""
    check_writer(gpu, case)


def test_device_reader_on_a_sweep(gpu, case):
    """decode_frames_device on the ORACLE's file of the sweep, the buffer exactly as long as the file: status 0, value bits,
    sizes and the valid bytes of every slot equal what the generator made.  For one family per stored size (SHIFTED) the same
    with the file 1 .. 7 bytes into its allocation: every alignment of the decoder's 8-byte windows and of the index pass's
    16-byte granules."""
    check_reader(gpu, case, case.ref, "at offset 0")
    kind, w, h, c, fam, k = case.param
    if kind != "mixed" and SHIFTED[(w, h)] == (fam, c):
        for shift in range(1, 8):
            check_reader(gpu, case, shifted(case.ref, shift), f"shifted by {shift}")


ENDS = [(slot, w, h, c) for slot, sizes in ((64, S.SIZES_64), (128, S.SIZES_128)) for (w, h, _) in sizes for c in (4, 3)]


@pytest.mark.parametrize("slot,w,h,c", ENDS)
def test_device_reader_when_the_buffer_ends_with_literals(gpu, oracle, slot, w, h, c):
    """The run|lit sweep from p = n down to p = 0 (of the largest sizes: its last part), spare tiles copies of the last one: the
    last record of the file, which ends with the buffer, is a tile of literals alone -- the decoder's window requests run up to
    the last window of the files while five bytes per pixel are still being consumed."""
    positions = S.parts_of(w, h, slot * slot * c)[0][::-1]
    assert positions[-1] == 0
    fr = S.sweep_frame("run|lit", w, h, slot, c, positions, spare=len(positions) - 1)
    assert fr.tw[-1] == w and fr.th[-1] == h and (fr.slots[-1, : w * h * c].reshape(-1, c) == S.literals(w * h, c)).all()
    cs = Case(oracle, fr, f"run|lit reversed {w}x{h} c{c}", lambda t: f"run|lit {w}x{h} p={positions[min(t, len(positions) - 1)]}")
    assert cs.ref.numel() == len(cs.raw)
    check_reader(gpu, cs, cs.ref, "exactly sized")
    check_reader(gpu, cs, shifted(cs.ref, 3), "exactly sized, shifted by 3")


# ---- the index pass: chunk ends, batches, windows ---------------------------------------------------------------------------

def check_against_oracle_decode(gpu, product, oracle, fr, seams, what):
    """decode_frames_device == oracle.decode_container on the oracle's file; then decode_windows_device over windows that end
    before, at and behind every seam record and start on either side of it: each equals the same tiles of the whole-file decode"""
    import torch
    raw = fr.encode(oracle)
    d = oracle.decode_container(raw)
    n = fr.slots.shape[1]
    assert (d["tw"] == fr.tw).all() and (d["th"] == fr.th).all()
    valid = fr.valid()
    for shift in (0, 5):
        files = shifted(torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda(), shift)
        offs = torch.tensor([0, len(raw)], dtype=torch.int64).cuda()
        vals, ow, oh, slots = gpu.decode_frames_device(files, offs, (1, fr.H, fr.W, fr.c), fr.bw, fr.bh)
        torch.cuda.synchronize()
        assert gpu.decode_status() == 0, f"{what} shift {shift}: status {gpu.decode_status()}"
        ow, oh, got = ow.cpu().numpy()[0], oh.cpu().numpy()[0], slots.cpu().numpy()[0]
        bad = (ow != d["tw"]) | (oh != d["th"]) | (vals.cpu().numpy()[0].view(np.uint32) != d["values"].view(np.uint32))
        bad |= ((got != d["slots"][:, :n]) & valid).any(axis=1)
        assert not bad.any(), f"{what} shift {shift}: tiles (row, column) {[divmod(int(t), fr.cols) for t in np.nonzero(bad)[0][:8]]}"
        wins, cover = S.seam_windows(fr, seams)
        assert wins
        to, wv, ww, wh, ws = gpu.decode_windows_device(files, offs, [(fr.W, fr.H)], wins, fr.c, fr.bw, fr.bh)
        torch.cuda.synchronize()
        assert gpu.decode_status() == 0, f"{what} shift {shift}: windows: status {gpu.decode_status()}"
        wv, ww, wh, ws = wv.cpu().numpy(), ww.cpu().numpy(), wh.cpu().numpy(), ws.cpu().numpy()
        assert int(to[-1]) == sum(c1 - c0 + 1 for (_, c0, c1) in cover)
        for k, (r, c0, c1) in enumerate(cover):
            a, t0 = int(to[k]), r * fr.cols + c0
            for j in range(c1 - c0 + 1):
                t = t0 + j
                ok = ww[a + j] == d["tw"][t] and wh[a + j] == d["th"][t] and wv.view(np.uint32)[a + j] == d["values"].view(np.uint32)[t]
                ok = ok and (ws[a + j][valid[t]] == d["slots"][t, :n][valid[t]]).all()
                assert ok, f"{what} shift {shift}: window over row {r}, columns {c0}..{c1}: column {c0 + j} differs from the whole-file decode"


@pytest.mark.parametrize("which", [1, 2])
def test_index_walk_at_every_offset_around_a_chunk_end(gpu, product, oracle, which):
    """Rows of 32x32-slot tiles, one per offset d = -40 .. 8: the seam record's header starts at 8192 + d (which = 1) or, behind
    a record that starts at 8192 exactly, at 16384 + d (which = 2) from the row's first byte -- its 23 bytes lie in the chunk,
    straddle its end or start the next one.  tests/test_stream_seams_host.py asserts the offsets from the oracle's record lengths."""
    fr, seam = S.walk_frame(oracle, which)
    check_against_oracle_decode(gpu, product, oracle, fr, [seam], f"chunk end {which}")


@pytest.mark.parametrize("cols", S.BATCH_COLS)
def test_index_walk_around_batches_of_64_records(gpu, product, oracle, cols):
    """Rows of 1x1 stored tiles in 8x8 slots, 63 .. 200 to a row: the records the index pass takes at a time end before, with
    and behind the row; windows end and start around records 64, 128 and 192 and around the row's last."""
    fr = S.batch_frame(cols)
    check_against_oracle_decode(gpu, product, oracle, fr, S.batch_seams(cols), f"{cols} columns")
