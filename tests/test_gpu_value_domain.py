"""The shrink kernels on the ends of the pixel-value domain: the pattern tiles of tests/value_patterns.py -- 0/255 edges, stripes,
impulses, alpha in 0..3 / 127, 128 / 254, 255 -- through every single-geometry path, the factor ladder, and the varied and archive
kernels' own copies of the reciprocal arithmetic.  Everything is equality with oracle.shrink_image: values as bit patterns, sizes,
the valid bytes of every slot.  What the patterns make the oracle do (which clamps fire, where un-premultiply saturates, which
stored sizes a pattern reaches) is asserted without a GPU in tests/test_value_domain_host.py; here the classes are asserted
again from the device's results, and the kernel choice through Handle.state(), so that a run that took another path fails."""
import functools

import numpy as np
import pytest

import value_patterns as vp
from test_gpu_handle_reuse import craft_transparency
from test_gpu_parity import assert_same_tiles

pytestmark = pytest.mark.gpu

NEAREST, TRIANGLE, CATMULLROM, GAUSSIAN, LANCZOS3 = range(5)
# the alpha tiles, repeated up to the number of opaque ones: both lists then lay out as the same grid (one launch signature)
ALPHA_PADDED = vp.ALPHA + vp.ALPHA[: len(vp.OPAQUE) - len(vp.ALPHA)]
KINDS = {"opaque": vp.OPAQUE, "alpha": ALPHA_PADDED, "all": vp.OPAQUE + vp.ALPHA, "mixed": tuple(vp.interleave(vp.ALPHA, vp.OPAQUE))}


@pytest.fixture(scope="module")
def gpu(product):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    h = product.Handle(0)
    yield h
    h.close()


# ---- frames, factors and references: made once, shared by every test, never written to --------------------------------------------

@functools.lru_cache(maxsize=None)
def pattern_frame(bw, bh, channels, kind):
    img, names = vp.frame(bw, bh, channels, KINDS[kind])
    img.setflags(write=False)
    return img, tuple(names), tuple(vp.full_tiles(img, bw, bh))


_factors, _expected = {}, {}


def kept_factors(oracle, bw, bh, channels, kind, mode, cap=None):
    key = (bw, bh, channels, kind, mode)
    if key not in _factors:
        _factors[key] = vp.factors(oracle, pattern_frame(bw, bh, channels, kind)[0], bw, bh, mode)
    ks = _factors[key]
    if cap is not None and len(ks) > cap:  # evenly over the walk, both ends kept
        ks = [ks[round(i * (len(ks) - 1) / (cap - 1))] for i in range(cap)]
    return ks


def expected(oracle, bw, bh, channels, kind, mode, filt, k):
    key = (bw, bh, channels, kind, mode, filt, k)
    if key not in _expected:
        _expected[key] = oracle.shrink_image(pattern_frame(bw, bh, channels, kind)[0], bw, bh, mode, filt, k, nthreads=4)
    return _expected[key]


def fetch(out, n=0):
    vals, ow, oh, slots = out
    return (vals[n].cpu().numpy(), ow[n].cpu().numpy().astype(np.uint32), oh[n].cpu().numpy().astype(np.uint32), slots[n].cpu().numpy())


def same_tiles(got, exp, channels, what, names):
    """assert_same_tiles, and on a difference the patterns of the tiles that differ: each pattern is a case of its own"""
    try:
        assert_same_tiles(got, exp, channels, what)
    except AssertionError as e:
        valid = exp[1].astype(np.int64) * exp[2] * channels
        inside = np.arange(exp[3].shape[1])[None, :] < valid[:, None]
        bad = (got[1] != exp[1]) | (got[2] != exp[2]) | (got[0].view(np.uint32) != exp[0].view(np.uint32)) | ((got[3] != exp[3]) & inside).any(axis=1)
        tiles = [f"{names[t]} (tile {t}, stored {int(exp[1][t])}x{int(exp[2][t])})" for t in np.nonzero(bad)[0][:12]]
        raise AssertionError(f"{e}\n  patterns: {', '.join(tiles)}") from None


def upload(img, rows="packed"):
    """[1, H, W, C] on the device.  rows = "packed": one contiguous block (an RGB pitch of 3 W bytes, odd for these frames:
    the library widens such a batch to RGBA and narrows the slots back).  rows = "aligned": the view [:, :, :W] of a tensor
    whose width is the next multiple of four pixels, so that every row starts on a 4-byte boundary -- what the native RGB
    instances of the fast kernels ask for."""
    import torch
    H, W, C = img.shape
    if rows == "packed":
        return torch.from_numpy(np.array(img))[None].cuda()
    assert rows == "aligned"
    wide = torch.zeros((1, H, (W + 3) & ~3, C), dtype=torch.uint8).cuda()
    frames = wide[:, :, :W]
    frames.copy_(torch.from_numpy(np.array(img))[None])
    assert frames.data_ptr() % 4 == 0 and (frames.stride(1) * frames.element_size()) % 4 == 0 and tuple(frames.shape) == (1, H, W, C)
    return frames


def run_factors(gpu, oracle, bw, bh, channels, kind, mode, filt, hint=False, cap=None, seen=None, rows="packed", after=None):
    """the frame at every kept factor against the oracle; -> {pattern: stored sizes of its full tiles}, from the device's results.
    after(k): called behind every launch, before its results are compared"""
    import torch
    img, names, full = pattern_frame(bw, bh, channels, kind)
    frames = upload(img, rows)
    seen = {} if seen is None else seen
    for k in kept_factors(oracle, bw, bh, channels, kind, mode, cap):
        out = gpu.shrink_frames_device(frames, bw, bh, mode, filt, k, transparency_hint=hint)
        torch.cuda.synchronize()
        if after is not None:
            after(k)
        got = fetch(out)
        same_tiles(got, expected(oracle, bw, bh, channels, kind, mode, filt, k), channels,
                   f"{kind} {bw}x{bh} c{channels} rows {rows} mode {mode} filter {filt} hint {hint} k={k}", names)
        for name, cl in vp.classes_by_pattern(names, got[1], got[2], full).items():
            seen.setdefault(name, set()).update(cl)
    return seen


def assert_classes(seen, bw, bh, mode, what):
    for name, got in seen.items():
        need, only = vp.required_classes(name, bw, bh, mode)
        assert need <= got, f"{what}: {name} was never stored at {sorted(need - got)}"
        assert not only or got == need, f"{what}: {name} was also stored at {sorted(got - need)}"


# ---- opaque fast paths ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("filt", [NEAREST, TRIANGLE, CATMULLROM, GAUSSIAN, LANCZOS3])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("channels,rows", [(4, "packed"), (3, "aligned"), (3, "packed")])
@pytest.mark.parametrize("block", [16, 32, 64])
def test_opaque_patterns_on_the_fast_paths(gpu, oracle, block, channels, rows, mode, filt):
    """shrink16 / shrink32 / shrink64_kernel on saturated opaque content: every pattern at every stored size it reaches -- the
    two-pass matrix-core and narrow forms (square classes), the dot2 form (n x 1, 1 x n, n x 2), the one-pass classes (dithered
    stripes), the clone, 1x1 -- with each form's own clamp text deciding bytes in both passes.
    RGBA: the frame's rows are no 16-byte multiples (a 7 px last column); the library re-pitches it and runs the RGBA instances.
    RGB, rows "aligned": pointer and pitch are multiples of four bytes (asserted in upload()), which is what selects the native
    RGB instances with their 12-byte loads and their own output packs.  RGB, rows "packed": an odd pitch; the batch is widened
    to RGBA, run there and narrowed back, or goes to the generic kernel where the filter's tables do not keep alpha 255."""
    seen = run_factors(gpu, oracle, block, block, channels, "opaque", mode, filt, rows=rows)
    assert set(seen) == set(vp.OPAQUE)
    assert_classes(seen, block, block, mode, f"{block}x{block} c{channels} rows {rows} mode {mode}")


# ---- alpha fast paths -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("filt", [TRIANGLE, CATMULLROM, LANCZOS3])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("block", [32, 64])
def test_alpha_patterns_hinted_and_not(product, oracle, block, mode, filt):
    """With PXZ_HINT_TRANSPARENCY the handle sets the full tiles with transparency aside for shrink32a_kernel /
    shrink64_kernel<MODE, true> (premultiplied matrix-core convolution of four planes, un-premultiply with the wave-ballot
    shortcut); without it this small frame stays on the generic kernel.  Same bits either way, equal to the oracle.
    Behind EVERY launch the handle's state is read: alpha_kernel is the choice the launch was set up with (it follows the
    hint here, as no launch of this size can report 2048 transparent tiles), never alpha_first."""
    h = product.Handle(0)  # (a handle of its own: what state() reports is this test's launches alone)
    try:
        seen = {}
        for hint in (True, False):
            launches = []

            def check_state(k, hint=hint, launches=launches):
                s = h.state()
                assert s["alpha_kernel"] == hint and not s["alpha_first"], f"hint {hint}, k={k}: {s}"
                launches.append(k)

            run_factors(h, oracle, block, block, 4, "alpha", mode, filt, hint=hint, seen=seen, after=check_state)
            assert launches == kept_factors(oracle, block, block, 4, "alpha", mode)
    finally:
        h.close()
    assert set(seen) == set(vp.ALPHA)
    assert_classes(seen, block, block, mode, f"alpha {block}x{block} mode {mode}")


def assert_batch_of_one_frame(out, exp, channels, what, names):
    """every frame of a batch of N copies of one frame equals that frame's expectation (compared on the device)"""
    import torch
    vals, ow, oh, slots = out
    ev, ew, eh, es = exp
    dev = vals.device
    tv = torch.from_numpy(ev.view(np.int32)).to(dev)
    tw, th = torch.from_numpy(ew.astype(np.int32)).to(dev), torch.from_numpy(eh.astype(np.int32)).to(dev)
    ts = torch.from_numpy(es).to(dev)
    inside = torch.arange(es.shape[1], device=dev)[None, :] < (tw.long() * th.long() * channels)[:, None]
    bad = (vals.view(torch.int32) != tv[None]).any(dim=1) | (ow != tw[None]).any(dim=1) | (oh != th[None]).any(dim=1) | \
          ((slots != ts[None]) & inside[None]).any(dim=2).any(dim=1)
    if bool(bad.any()):
        n = int(torch.nonzero(bad)[0])
        same_tiles(fetch(out, n), exp, channels, f"{what}: {int(bad.sum())} of {vals.shape[0]} frames differ, frame {n}", names)
        raise AssertionError(f"{what}: frame {n} differs")


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("block", [32, 64])
def test_patterns_with_the_four_plane_kernel_first(product, oracle, block, mode):
    """alpha_first: once a launch of this signature has listed at least 2048 full tiles with transparency, and half of all tiles,
    the four-plane kernel takes every tile of the next one.  A fresh handle; batches of 128 copies of one pattern frame (16 full
    tiles each: exactly 2048, the smallest batch that can flip the state).  The signature a count is trusted under includes the
    factor's bits, so the sequence runs once per factor: a primer whose full tiles all carry transparency (the opaque patterns
    under the alpha patterns' alpha; alpha_first is off, nothing of this signature has run), then the alpha patterns (on,
    from the primer's count), then the opaque patterns (still on, from the alpha patterns' count: the statistic is one launch
    behind, so the opaque tiles go through the premultiplying kernel).  Under shrink_by the detector copies the tiles that are
    stored whole and nobody looks at their alpha again, so there the factors are those at which the oracle stores no full tile
    of the primer or of the alpha patterns whole.  Everything equals the oracle."""
    import torch
    h = product.Handle(0)
    try:
        a_img, a_names, full = pattern_frame(block, block, 4, "alpha")
        o_img, o_names, _ = pattern_frame(block, block, 4, "opaque")
        assert a_img.shape == o_img.shape
        n_frames = -(-2048 // sum(full))
        assert n_frames * sum(full) == 2048 and 2048 >= n_frames * len(full) // 2
        alpha = upload(a_img).expand(n_frames, -1, -1, -1).contiguous()
        opaque = upload(o_img).expand(n_frames, -1, -1, -1).contiguous()
        primer = craft_transparency(opaque, alpha, 2048, block, np.random.default_rng(block + mode))
        p_img = primer[0].cpu().numpy()
        assert bool((primer == primer[:1]).all())
        cols = -(-p_img.shape[1] // block)
        for img in (p_img, a_img):  # every full tile of the primer and of the alpha patterns carries transparency
            for t, f in enumerate(full):
                r, c = divmod(t, cols)
                assert not f or (img[r * block:(r + 1) * block, c * block:(c + 1) * block, 3] != 255).any()
        p_names = tuple(f"{o} under the alpha of {a}" for o, a in zip(o_names, a_names))

        def stores_whole(img, k):
            _, ew, eh, _ = oracle.shrink_image(img, block, block, mode, LANCZOS3, k, want_pixels=False)
            return bool(((ew == block) & (eh == block) & np.array(full)).any())

        ks = [k for k in kept_factors(oracle, block, block, 4, "alpha", mode)
              if mode == 1 or not (stores_whole(p_img, k) or stores_whole(a_img, k))]
        assert len(ks) >= 4, ks
        ks = [ks[round(i * (len(ks) - 1) / 3)] for i in range(4)]
        for k in ks:
            for frames, exp, names, what, first in (
                    (primer, oracle.shrink_image(p_img, block, block, mode, LANCZOS3, k, nthreads=4), p_names, "primer", False),
                    (alpha, expected(oracle, block, block, 4, "alpha", mode, LANCZOS3, k), a_names, "alpha patterns", True),
                    (opaque, expected(oracle, block, block, 4, "opaque", mode, LANCZOS3, k), o_names, "opaque patterns", True)):
                out = h.shrink_frames_device(frames, block, block, mode, LANCZOS3, k)
                torch.cuda.synchronize()
                s = h.state()
                assert s["alpha_first"] == first and s["alpha_kernel"] == first, f"{what} at k={k}: {s}"
                assert_batch_of_one_frame(out, exp, 4, f"{what} {block}x{block} mode {mode} k={k}", names)
    finally:
        h.close()


# ---- 16x16 groups -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("filt", [TRIANGLE, CATMULLROM, LANCZOS3])
@pytest.mark.parametrize("mode", [0, 1])
def test_groups_of_16x16_tiles_mix_alpha_and_opaque_patterns(gpu, oracle, mode, filt):
    """alpha and opaque patterns by turns: every 2x2 group of shrink16_kernel holds tiles it resamples itself and tiles it
    hands on because they carry transparency"""
    img, names, _ = pattern_frame(16, 16, 4, "mixed")
    cols = -(-img.shape[1] // 16)
    for r in range(0, img.shape[0] // 16 - 1, 2):
        for c in range(0, img.shape[1] // 16 - 1, 2):
            group = [names[(r + dr) * cols + c + dc] for dr in (0, 1) for dc in (0, 1)]
            assert any(n in vp.ALPHA for n in group) and any(n in vp.OPAQUE for n in group), group
    seen = {}
    for hint in (False, True):
        run_factors(gpu, oracle, 16, 16, 4, "mixed", mode, filt, hint=hint, seen=seen)
    assert set(seen) == set(vp.OPAQUE + vp.ALPHA)
    assert_classes(seen, 16, 16, mode, f"16x16 mode {mode}")


# ---- generic kernel ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("filt", [LANCZOS3, GAUSSIAN])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("channels", [4, 3])
@pytest.mark.parametrize("bw,bh", [(48, 20), (24, 24)])
def test_patterns_on_the_generic_kernel(gpu, oracle, bw, bh, channels, mode, filt):
    """tile sizes without a fast path: clamp_fixed / clamp_fixed_v and the generic kernel's un-premultiply, opaque and alpha
    patterns (RGB: the opaque ones), at odd stored sizes (3x2, 6x3, 12x5, ...)"""
    kind = "all" if channels == 4 else "opaque"
    seen = run_factors(gpu, oracle, bw, bh, channels, kind, mode, filt)
    assert set(seen) == set(KINDS[kind])
    assert_classes(seen, bw, bh, mode, f"{bw}x{bh} c{channels} mode {mode}")


def test_patterns_in_tiles_beyond_lds_residency(gpu, oracle):
    """192x192 tiles (the image stays in HBM between the passes), the patterns generated at that size, three factors: two under
    the directional detector (one-pass classes, one side at 1, squares) and one under the Oklab detector"""
    names = pattern_frame(192, 192, 4, "all")[1]
    frames = upload(pattern_frame(192, 192, 4, "all")[0])
    sizes = set()
    for mode, k in ((1, 64.0), (1, 1.0), (0, 0.125)):
        got = fetch(gpu.shrink_frames_device(frames, 192, 192, mode, LANCZOS3, k))
        same_tiles(got, expected(oracle, 192, 192, 4, "all", mode, LANCZOS3, k), 4, f"192x192 mode {mode} k={k}", names)
        sizes |= set(zip(got[1].tolist(), got[2].tolist()))
    for cl in ((192, 192), (96, 96), (48, 48), (192, 24), (24, 192), (1, 96), (96, 1), (2, 48), (1, 1)):
        assert cl in sizes, (cl, sorted(sizes))


# ---- factor ladder ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("hint", [False, True])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("block", [32, 64])
def test_ladder_rungs_on_the_patterns(gpu, oracle, block, mode, hint):
    """pxz_shrink_ladder_frames_device (shrink_by: ladder_kernel and its alpha tail; directional: a call per rung) over at most
    16 of the kept factors: each rung equals its single call and the oracle"""
    import torch
    img, names, _ = pattern_frame(block, block, 4, "all")
    frames = upload(img)
    ks = kept_factors(oracle, block, block, 4, "all", mode, cap=16)
    assert 8 <= len(ks) <= 16
    lad = gpu.shrink_ladder_frames_device(frames, block, block, mode, LANCZOS3, ks, transparency_hint=hint)
    torch.cuda.synchronize()
    for r, k in enumerate(ks):
        rung = fetch(tuple(x[r] for x in lad))
        one = fetch(gpu.shrink_frames_device(frames, block, block, mode, LANCZOS3, k, transparency_hint=hint))
        same_tiles(rung, one, 4, f"ladder {block} mode {mode} hint {hint} rung {r} (k={k}) vs single", names)
        same_tiles(rung, expected(oracle, block, block, 4, "all", mode, LANCZOS3, k), 4,
                   f"ladder {block} mode {mode} hint {hint} rung {r} (k={k}) vs oracle", names)


# ---- the varied and archive kernels' own copies of the reciprocal arithmetic --------------------------------------------------------

@pytest.mark.parametrize("mode", [0, 1])
def test_varied_batch_over_the_alpha_patterns(gpu, product, oracle, mode):
    """pxz_shrink_varied_frames_device at 32x32 on two differently sized alpha pattern frames (pxz_varied.hip and
    pxz_varied_tile.h un-premultiply for themselves), poisoned outputs, Lanczos3 and CatmullRom"""
    from test_gpu_varied import tiles_of, upload as upload_images, varied
    a, a_names, _ = pattern_frame(32, 32, 4, "alpha")
    b, b_names = vp.frame(32, 32, 4, vp.ALPHA[::-1])
    assert a.shape != b.shape
    buf, geoms = upload_images([a, b], 4, pad=12, misalign=3)
    for filt in (LANCZOS3, CATMULLROM):
        for k in kept_factors(oracle, 32, 32, 4, "alpha", mode, cap=8):
            res = varied(gpu, product, buf, geoms, 4, 32, 32, mode, filt, k)
            same_tiles(tiles_of(res, 0), expected(oracle, 32, 32, 4, "alpha", mode, filt, k), 4, f"varied mode {mode} filter {filt} k={k} image 0", a_names)
            same_tiles(tiles_of(res, 1), oracle.shrink_image(b, 32, 32, mode, filt, k), 4, f"varied mode {mode} filter {filt} k={k} image 1", b_names)


@pytest.mark.parametrize("mode", [0, 1])
def test_reshrink_over_the_alpha_patterns(gpu, oracle, mode):
    """pxz_reshrink_varied_frames_device at 32x32, out of place: the alpha pattern frame stored whole and stored as the oracle
    shrinks it at a middle factor (its tiles then hold un-premultiplied low alpha themselves), expanded with Lanczos3 and
    shrunk again -- pxz_reshrink.hip's expand and shrink both un-premultiply with their own text.  Equal to the oracle's
    expand_image + shrink_image."""
    import torch
    from test_gpu_varied_decode import poisoned
    img, names, _ = pattern_frame(32, 32, 4, "alpha")
    H, W, _ = img.shape
    ks = kept_factors(oracle, 32, 32, 4, "alpha", mode)
    stored = [oracle.shrink_image(img, 32, 32, mode, LANCZOS3, k) for k in (ks[0], ks[len(ks) // 2])]
    assert (stored[0][1] * stored[0][2]).sum() > (stored[1][1] * stored[1][2]).sum() > len(names)
    for s, (_, tw, th, slots) in enumerate(stored):
        back = oracle.expand_image(W, H, 32, 32, 4, LANCZOS3, tw, th, slots)
        dev = (torch.from_numpy(tw.astype(np.int32)).cuda(), torch.from_numpy(th.astype(np.int32)).cuda(), torch.from_numpy(slots).cuda())
        for k in vp.factors(oracle, back, 32, 32, mode)[::3]:
            out, flags = poisoned(len(names), 32 * 32 * 4, 1)
            gpu.reshrink_varied_frames_device([(W, H)], 4, 32, 32, mode, LANCZOS3, k, LANCZOS3, *dev, out=out, image_flags=flags)
            torch.cuda.synchronize()
            assert gpu.decode_status() == 0 and int(flags[0]) == 0
            got = (out[0].cpu().numpy(), out[1].cpu().numpy().astype(np.uint32), out[2].cpu().numpy().astype(np.uint32), out[3].cpu().numpy())
            same_tiles(got, oracle.shrink_image(back, 32, 32, mode, LANCZOS3, k), 4, f"re-shrink of store {s}, mode {mode} k={k}", names)
