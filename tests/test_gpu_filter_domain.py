"""process() and tree::process on the ends of the pixel-value domain: the frames of tests/filter_patterns.py -- sparse 0/255 and
low-alpha tiles that are pixelised at every size from "unchanged" to 1x1, beside the edge, stripe, impulse and alpha tiles of
tests/value_patterns.py -- through pxz_process_frames_device and both forms of pxz_tree_process_frames_device (the per-level
grids, and the rectangle lists of pxz_tree.hip with their own copies of the fir arithmetic), with every filter on each side,
RGBA and RGB, and into output views whose pitch and frame stride are not the packed ones.  Everything is equality with
oracle.process_image / oracle.tree_process_image, pixel for pixel; a difference is reported by the pattern and the rectangle it
lies in.  What these inputs make the oracle do (which levels of the recursion pixelise, split and keep, which passes leave
0..255 before their clamp, where un-premultiply gets a colour above its alpha) is asserted without a GPU in
tests/test_filter_domain_host.py."""
import numpy as np
import pytest

import filter_patterns as fp

pytestmark = pytest.mark.gpu

CHANNELS = [pytest.param(4, id="c4"), pytest.param(3, id="c3")]
PAIRS = [pytest.param(d, u, id=f"down{d}up{u}") for d, u in fp.FILTER_PAIRS]


def case_id(case):
    return "x".join(str(v) for v in case[:2]) + "".join(f"-{v}" for v in case[2:-2]) + "-edge%dx%d" % case[-2] + ("-subset" if case[-1] else "")


@pytest.fixture(scope="module")
def gpu(product):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    h = product.Handle(0)
    yield h
    h.close()


def upload(frames):
    import torch
    return torch.from_numpy(np.array(frames)).cuda()


def same_image(oracle, got, exp, frame, names, bw, bh, what, census):
    """equality, and on a difference the rectangles that hold it, by pattern (census: called for the model's, then only)"""
    bad = (got != exp).any(axis=2)
    if bad.any():
        entries = fp.rects_of(census()[1], bad)
        y, x = np.argwhere(bad)[0]
        raise AssertionError(f"{what}: {int(bad.sum())} pixels differ, first at ({x}, {y}): got {got[y, x].tolist()}, expected {exp[y, x].tolist()}\n"
                             f"  in {len(entries)} rectangles: {fp.describe(entries, names, frame.shape[1], bw, bh)}")


# ---- process() -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("channels", CHANNELS)
@pytest.mark.parametrize("down,up", PAIRS)
@pytest.mark.parametrize("case", fp.PROCESS_CASES, ids=case_id)
def test_process_on_the_value_domain(gpu, oracle, case, down, up, channels):
    """Blocks of 16, 32 and 64 px (the fused shrink kernels and the fast expand forms), 20x12 (the generic ones) and 128 px; ragged
    edges of 7x5 and 1x1 px; two frames, the second with every tile a place further on."""
    import torch
    bw, bh, edge, sub = case
    frames, names = fp.case_batch(bw, bh, channels, edge, sub)
    out = gpu.process_frames_device(upload(frames), bw, bh, down, up)
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    for n in range(2):
        exp = oracle.process_image(frames[n], bw, bh, down, up)
        same_image(oracle, out[n], exp, frames[n], names[n], bw, bh, f"process {bw}x{bh} c{channels} down {down} up {up} frame {n}",
                   lambda: fp.process(oracle, frames[n], bw, bh, down, up))
    assert gpu.decode_status() == 0


# ---- tree::process -------------------------------------------------------------------------------------------------------------------

def run_tree(gpu, oracle, case, down, up, channels):
    import torch
    bw, bh, mw, mh, edge, sub = case
    frames, names = fp.case_batch(bw, bh, channels, edge, sub)
    dev = upload(frames)
    exp = fp.tree_references(oracle, frames, bw, bh, mw, mh, down, up)
    for thr in fp.THRESHOLDS:
        out = gpu.tree_process_frames_device(dev, bw, bh, thr, mw, mh, down, up)
        torch.cuda.synchronize()
        out = out.cpu().numpy()
        for n in range(2):
            same_image(oracle, out[n], exp[n, thr], frames[n], names[n], bw, bh,
                       f"tree {bw}x{bh} min {mw}x{mh} c{channels} down {down} up {up} threshold {thr} frame {n}",
                       lambda: fp.tree_process(oracle, frames[n], bw, bh, thr, mw, mh, down, up))
    assert gpu.decode_status() == 0


@pytest.mark.parametrize("channels", CHANNELS)
@pytest.mark.parametrize("down,up", PAIRS)
@pytest.mark.parametrize("case", fp.TREE_GRID_CASES, ids=case_id)
def test_tree_grid_on_the_value_domain(gpu, oracle, case, down, up, channels):
    """Blocks that halve evenly, up to 64 px: one regular grid per level (the shrink kernels, tree_decide_kernel, the expand
    kernels' quiet form) -- or, under PXZ_TREE_RECTS, the rectangle lists on the same cases."""
    run_tree(gpu, oracle, case, down, up, channels)


@pytest.mark.parametrize("channels", CHANNELS)
@pytest.mark.parametrize("down,up", PAIRS)
@pytest.mark.parametrize("case", fp.TREE_RECT_CASES, ids=case_id)
def test_tree_rects_on_the_value_domain(gpu, oracle, case, down, up, channels):
    """Blocks whose halvings go odd (50 -> 25 -> 12 + 12 + 1, 37x61, 100x36) and 128-px blocks: tree_rect_kernel, which measures,
    decides and resamples down and up in one launch with its own mul_div_255 / reciprocal / clamp."""
    run_tree(gpu, oracle, case, down, up, channels)


# ---- layout: strided input, an output view with gaps -----------------------------------------------------------------------------------

def strided_input(frames, offset, extra_pitch, gap):
    """the batch as a view into a flat buffer: `offset` bytes in, rows extra_pitch bytes longer than their pixels, `gap` bytes
    between the frames; the bytes between hold 0xEE"""
    import torch
    N, H, W, C = frames.shape
    pitch = W * C + extra_pitch
    stride = pitch * H + gap
    base = torch.full((offset + N * stride,), 0xEE, dtype=torch.uint8).cuda()
    view = base.as_strided((N, H, W, C), (stride, pitch, C, 1), offset)
    view.copy_(torch.from_numpy(np.array(frames)).cuda())
    assert view.data_ptr() == base.data_ptr() + offset and view.stride(1) == pitch and view.stride(0) == stride
    return base, view


def poisoned_output(N, H, W):
    """-> (flat buffer, its bytes on the host, the [N, H, W, 4] view with pitch W * 4 + 16 and frame stride pitch * H + 64,
    bool per byte: inside an image row)"""
    import torch
    pitch = W * 4 + 16
    stride = pitch * H + 64
    poison = ((np.arange(N * stride, dtype=np.uint32) * 37 + 11) & 0xFF).astype(np.uint8)
    base = torch.from_numpy(poison.copy()).cuda()
    view = base.as_strided((N, H, W, 4), (stride, pitch, 4, 1), 0)
    inside = np.zeros(N * stride, bool)
    for n in range(N):
        rows = inside[n * stride:n * stride + pitch * H].reshape(H, pitch)
        rows[:, : W * 4] = True
    return base, poison, view, inside


def check_layout(base, poison, view, inside, out, exp, what):
    import torch
    torch.cuda.synchronize()
    assert out.data_ptr() == view.data_ptr() and out.stride() == view.stride()
    after = base.cpu().numpy()
    touched = (after != poison) & ~inside
    assert not touched.any(), f"{what}: {int(touched.sum())} bytes outside the image rows were written, first at byte {int(np.argmax(touched))}"
    got = view.cpu().numpy()
    for n in range(len(exp)):
        bad = (got[n] != exp[n]).any(axis=2)
        assert not bad.any(), f"{what} frame {n}: {int(bad.sum())} pixels differ, first at {np.argwhere(bad)[0][::-1].tolist()}"


def test_process_reads_a_strided_batch_and_writes_a_view_with_gaps(gpu, oracle):
    frames, _ = fp.case_batch(32, 32, 4, (7, 5), False)
    _, view = strided_input(frames, 0, 16, 48)
    N, H, W, _ = frames.shape
    for down, up in ((4, 0), (2, 4)):
        base, poison, out_view, inside = poisoned_output(N, H, W)
        out = gpu.process_frames_device(view, 32, 32, down, up, out=out_view)
        check_layout(base, poison, out_view, inside, out, [oracle.process_image(frames[n], 32, 32, down, up) for n in range(N)],
                     f"process down {down} up {up}")


def test_grid_tree_reads_a_strided_batch_and_writes_a_view_with_gaps(gpu, oracle):
    """every level writes through the output's pitch: the expand kernels' quiet form the pixelised tiles, tree_decide_kernel the
    kept ones, the widening copy the whole frame when the block is at the minimum"""
    frames, _ = fp.case_batch(32, 32, 3, (7, 5), False)
    _, view = strided_input(frames, 0, 5, 31)
    N, H, W, _ = frames.shape
    for bw, thr, down, up in ((32, 0.16, 4, 0), (32, 0.0, 2, 4), (32, -0.16, 1, 2), (4, 0.16, 4, 0)):
        base, poison, out_view, inside = poisoned_output(N, H, W)
        out = gpu.tree_process_frames_device(view, bw, bw, thr, 4, 4, down, up, out=out_view)
        check_layout(base, poison, out_view, inside, out, [oracle.tree_process_image(frames[n], bw, bw, thr, 4, 4, down, up) for n in range(N)],
                     f"grid tree {bw}x{bw} threshold {thr} down {down} up {up}")
    frames, _ = fp.case_batch(32, 32, 4, (1, 1), False)
    _, view = strided_input(frames, 0, 16, 48)
    N, H, W, _ = frames.shape
    base, poison, out_view, inside = poisoned_output(N, H, W)
    out = gpu.tree_process_frames_device(view, 32, 32, 0.08, 4, 4, 4, 0, out=out_view)
    check_layout(base, poison, out_view, inside, out, [oracle.tree_process_image(frames[n], 32, 32, 0.08, 4, 4, 4, 0) for n in range(N)],
                 "grid tree 32x32 rgba")


def test_rect_tree_reads_an_odd_offset_batch_and_writes_a_view_with_gaps(gpu, oracle):
    """RGB at an odd byte offset with an odd pitch; then RGBA: pixelised, split and kept rectangles all store through dst_pitch"""
    for channels, offset, extra, gap in ((3, 1, 7, 33), (4, 0, 16, 48)):
        frames, _ = fp.case_batch(50, 50, channels, (7, 5), False)
        base_in, view = strided_input(frames, offset, extra, gap)
        assert view.data_ptr() % 2 == offset
        N, H, W, _ = frames.shape
        for thr, down, up in ((0.16, 4, 0), (0.03, 2, 4), (-0.16, 3, 1)):
            base, poison, out_view, inside = poisoned_output(N, H, W)
            out = gpu.tree_process_frames_device(view, 50, 50, thr, 4, 4, down, up, out=out_view)
            check_layout(base, poison, out_view, inside, out, [oracle.tree_process_image(frames[n], 50, 50, thr, 4, 4, down, up) for n in range(N)],
                         f"rect tree c{channels} threshold {thr} down {down} up {up}")


def test_out_views_are_checked(gpu):
    import torch
    frames = upload(fp.case_batch(16, 16, 4, (7, 5), False)[0])
    N, H, W, _ = frames.shape
    for bad in (torch.empty((N, H, W, 3), dtype=torch.uint8).cuda(), torch.empty((N, H, W + 1, 4), dtype=torch.uint8).cuda(),
                torch.empty((N, H, W, 8), dtype=torch.uint8).cuda()[..., ::2]):
        with pytest.raises(AssertionError):
            gpu.process_frames_device(frames, 16, 16, out=bad)
        with pytest.raises(AssertionError):
            gpu.tree_process_frames_device(frames, 16, 16, 0.1, out=bad)
