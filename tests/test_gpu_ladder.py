"""The factor ladder (pxz_shrink_ladder_frames_device / pxz_shrink_image_ladder): every rung equals the single-factor call
at its factor -- values as u32 bits, reduced sizes, valid slot bytes -- and the oracle, on the ladder kernel's geometries and
on the ones that fall back to a call per rung; the rung sets are a batch to the device writer; a ladder between single
calls on one handle changes none of them."""
import ctypes as C
import os

import numpy as np
import pytest
from PIL import Image

from test_gpu_parity import assert_same_tiles

pytestmark = pytest.mark.gpu

FILTERS = (0, 1, 2, 3, 4)
SHRINK_BY_FACTORS = [0.5, 0.125, 0.125, 2.0, 0.0, -0.5, 1e-6]  # unsorted, repeated, zero, negative, everything to 1x1
DIRECTIONAL_FACTORS = [16.0, 4.0, 64.0]


@pytest.fixture(scope="module")
def gpu(product):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    h = product.Handle(0)
    yield h
    h.close()


def host(out, r, f=0):
    vals, ow, oh, slots = out
    return (vals[r, f].cpu().numpy(), ow[r, f].cpu().numpy().astype(np.uint32), oh[r, f].cpu().numpy().astype(np.uint32),
            None if slots is None else slots[r, f].cpu().numpy())


def host1(out, f=0):
    vals, ow, oh, slots = out
    return (vals[f].cpu().numpy(), ow[f].cpu().numpy().astype(np.uint32), oh[f].cpu().numpy().astype(np.uint32),
            None if slots is None else slots[f].cpu().numpy())


def check_rungs(gpu, oracle, frames, bw, bh, mode, filt, factors, imgs=None, hint=False, what=""):
    """ladder == single call per factor (every frame) and == the oracle (frames given in imgs)"""
    import torch
    C_ = frames.shape[3]
    lad = gpu.shrink_ladder_frames_device(frames, bw, bh, mode, filt, factors, transparency_hint=hint)
    torch.cuda.synchronize()
    for r, k in enumerate(factors):
        one = gpu.shrink_frames_device(frames, bw, bh, mode, filt, k, transparency_hint=hint)
        torch.cuda.synchronize()
        for f in range(frames.shape[0]):
            assert_same_tiles(host(lad, r, f), host1(one, f), C_, f"{what} rung {r} (k={k}) frame {f} vs single")
        if imgs is not None:
            for f, img in enumerate(imgs):
                exp = oracle.shrink_image(img, bw, bh, mode, filt, k, nthreads=8)
                assert_same_tiles(host(lad, r, f), exp, C_, f"{what} rung {r} (k={k}) frame {f} vs oracle")
    return lad


@pytest.mark.parametrize("c", [4, 3])
@pytest.mark.parametrize("block", [16, 32, 64])
@pytest.mark.parametrize("w,h", [(1000, 600), (333, 257)])
def test_rungs_equal_single_calls_and_oracle(gpu, product, oracle, w, h, block, c):
    import torch
    imgs = [oracle.synth_frame(w, h, c, 3 + f, (f % 2) if c == 4 else 0) for f in range(2)]
    frames = torch.from_numpy(np.stack(imgs)).cuda()
    for filt in FILTERS:
        check_rungs(gpu, oracle, frames, block, block, 0, filt, SHRINK_BY_FACTORS, imgs, what=f"shrink_by {w}x{h} {block} c{c} f{filt}")
    if h % block == 1:  # a 1-px-high edge row: the directional detector refuses it, as the single call does
        with pytest.raises(product.PxzError) as e:
            gpu.shrink_ladder_frames_device(frames, block, block, 1, 4, DIRECTIONAL_FACTORS)
        assert e.value.code == -4
        return
    for filt in (0, 4):
        check_rungs(gpu, oracle, frames, block, block, 1, filt, DIRECTIONAL_FACTORS, imgs, what=f"directional {w}x{h} {block} c{c} f{filt}")


def test_reference_pinned_decisions_on_big_ruscher(gpu, product, oracle, golden_dir):
    """The 0.125 rung's sizes are the 2040 decisions of the reference's own file; payloads against the oracle (the fixture's
    fir bits are not pinned)."""
    img = np.ascontiguousarray(np.asarray(Image.open(os.path.join(golden_dir, "Big-Ruscher.png"))))
    assert img.shape[2] == 3
    factors = [0.5, 0.125, 2.0]
    vals, ow, oh, slots = gpu.shrink_image_ladder(img, 32, 32, 0, 4, factors)
    for r, k in enumerate(factors):
        exp = oracle.shrink_image(img, 32, 32, 0, 4, k, nthreads=8)
        assert_same_tiles((vals[r], ow[r], oh[r], slots[r]), exp, 3, f"Big-Ruscher rung {r}")
    data = open(os.path.join(golden_dir, "Big-Ruscher.pix"), "rb").read()
    L = product.load_library()
    u = [C.c_uint32() for _ in range(6)]
    buf = C.create_string_buffer(data, len(data))
    gpu._check(L.pxz_decode_file(gpu._h, buf, len(data), *[C.byref(x) for x in u], None, None, None, None))
    W, H, bw, bh, ch = (x.value for x in u[:5])
    cols, rows = product.grid(W, H, bw, bh)
    assert (W, H, bw, bh, ch) == (img.shape[1], img.shape[0], 32, 32, 3) and cols * rows == 2040
    tv = np.zeros(cols * rows, np.float32)
    tw = np.zeros(cols * rows, np.uint32)
    th = np.zeros(cols * rows, np.uint32)
    ts = np.zeros((cols * rows, bw * bh * ch), np.uint8)
    gpu._check(L.pxz_decode_file(gpu._h, buf, len(data), *[C.byref(x) for x in u], tv.ctypes.data, tw.ctypes.data,
                                 th.ctypes.data, ts.ctypes.data))
    assert (ow[1] == tw).all() and (oh[1] == th).all()


@pytest.mark.parametrize("hint", [False, True])
def test_transparency(gpu, oracle, hint):
    """DIST_ALPHA frames and a batch that mixes them with opaque ones, 32x32, with and without PXZ_HINT_TRANSPARENCY"""
    import torch
    alpha = [oracle.synth_frame(800, 480, 4, 40 + f, 1) for f in range(2)]
    mixed = [oracle.synth_frame(800, 480, 4, 50, 0), oracle.synth_frame(800, 480, 4, 51, 1)]
    for imgs, name in ((alpha, "alpha"), (mixed, "mixed")):
        frames = torch.from_numpy(np.stack(imgs)).cuda()
        for filt in (1, 4):
            check_rungs(gpu, oracle, frames, 32, 32, 0, filt, [1.0, 0.25, 4.0, 0.25], imgs, hint=hint, what=f"{name} f{filt}")


def test_fallback_geometries(gpu, oracle):
    """48x40 tiles, 300x200 tiles (beyond LDS residency: one call per rung), an unaligned RGBA view"""
    import torch
    imgs = [oracle.synth_frame(500, 330, 4, 60 + f, f % 2) for f in range(2)]
    frames = torch.from_numpy(np.stack(imgs)).cuda()
    check_rungs(gpu, oracle, frames, 48, 40, 0, 4, [0.5, 2.0, 0.125], imgs, what="48x40")
    check_rungs(gpu, oracle, frames, 300, 200, 0, 2, [0.5, 2.0], imgs, what="300x200")
    check_rungs(gpu, oracle, frames, 300, 200, 1, 4, [16.0, 2.0], imgs, what="300x200 directional")
    wide = torch.from_numpy(np.stack([oracle.synth_frame(503, 330, 4, 70 + f, f % 2) for f in range(2)])).cuda()
    view = wide[:, :, 1:501]  # rows start 4 bytes into a 2012-byte pitch
    base = [np.ascontiguousarray(view[f].cpu().numpy()) for f in range(2)]
    for block in (32, 64):
        check_rungs(gpu, oracle, view, block, block, 0, 4, [0.5, 0.125, 2.0], base, what=f"unaligned {block}")
    rgb = torch.from_numpy(np.stack([oracle.synth_frame(501, 330, 3, 80 + f, 0) for f in range(2)])).cuda()[:, :, 1:]
    check_rungs(gpu, oracle, rgb, 32, 32, 0, 3, [0.5, 2.0], [np.ascontiguousarray(rgb[f].cpu().numpy()) for f in range(2)], what="unaligned rgb")


def test_rung_sets_are_a_batch_to_the_writer(gpu, oracle):
    """encode_frames_device over the K*N rung sets at once == the K*N files of the single calls; one case == the oracle writer"""
    import torch
    for c, mode, factors in ((4, 0, [0.5, 0.125, 2.0]), (3, 0, [1.0, 0.25]), (4, 1, [16.0, 4.0])):
        imgs = [oracle.synth_frame(672, 416, c, 20 + f, (f % 2) if c == 4 else 0) for f in range(2)]
        frames = torch.from_numpy(np.stack(imgs)).cuda()
        N, H, W, _ = frames.shape
        K = len(factors)
        vals, ow, oh, slots = gpu.shrink_ladder_frames_device(frames, 32, 32, mode, 4, factors)
        T = vals.shape[2]
        offs, buf = gpu.encode_frames_device((K * N, H, W, c), 32, 32, vals.view(K * N, T), ow.view(K * N, T), oh.view(K * N, T),
                                             slots.view(K * N, T, -1))
        torch.cuda.synchronize()
        offs = offs.cpu().numpy()
        data = buf[: offs[-1]].cpu().numpy().tobytes()
        for r, k in enumerate(factors):
            v1, w1, h1, s1 = gpu.shrink_frames_device(frames, 32, 32, mode, 4, k)
            o1, b1 = gpu.encode_frames_device((N, H, W, c), 32, 32, v1, w1, h1, s1)
            torch.cuda.synchronize()
            o1 = o1.cpu().numpy()
            d1 = b1[: o1[-1]].cpu().numpy().tobytes()
            for f in range(N):
                i = r * N + f
                assert data[offs[i]:offs[i + 1]] == d1[o1[f]:o1[f + 1]], (c, mode, k, f)
            if c == 4 and mode == 0 and r == 1:
                v, w, h, s = oracle.shrink_image(imgs[0], 32, 32, mode, 4, k, nthreads=8)
                assert data[offs[N]:offs[N + 1]] == oracle.encode_container(W, H, 32, 32, c, 0, v, None, w, h, s)


def test_values_only_and_errors(gpu, product, oracle):
    import torch
    imgs = [oracle.synth_frame(640, 360, 4, 90 + f, f % 2) for f in range(2)]
    frames = torch.from_numpy(np.stack(imgs)).cuda()
    for block, mode, factors in ((32, 0, SHRINK_BY_FACTORS), (64, 0, [0.5, 2.0]), (48, 0, [0.5, 2.0]), (32, 1, DIRECTIONAL_FACTORS)):
        full = gpu.shrink_ladder_frames_device(frames, block, block, mode, 4, factors)
        lean = gpu.shrink_ladder_frames_device(frames, block, block, mode, 4, factors, want_pixels=False)
        torch.cuda.synchronize()
        assert lean[3] is None
        assert (full[0].view(torch.int32) == lean[0].view(torch.int32)).all()
        assert (full[1] == lean[1]).all() and (full[2] == lean[2]).all()
    for bad in ([], [1.0] * 17, [0.5, float("nan")], [float("inf")]):
        with pytest.raises(product.PxzError) as e:
            gpu.shrink_ladder_frames_device(frames, 32, 32, 0, 4, bad)
        assert e.value.code == -1, bad
        with pytest.raises(product.PxzError) as e:
            gpu.shrink_image_ladder(imgs[0], 32, 32, 0, 4, bad)
        assert e.value.code == -1, bad
    gpu.shrink_ladder_frames_device(frames, 32, 32, 0, 4, [1.0] * 16)  # the maximum is allowed
    edge = torch.from_numpy(oracle.synth_frame(33, 40, 4, 0, 0)[None].copy()).cuda()  # a 1-px-wide edge tile
    with pytest.raises(product.PxzError) as e:
        gpu.shrink_ladder_frames_device(edge, 32, 32, 1, 4, [16.0, 4.0])
    assert e.value.code == -4
    with pytest.raises(product.PxzError) as e:
        gpu.shrink_ladder_frames_device(edge, 32, 32, 0, 9, [1.0])
    assert e.value.code == -1
    gpu.shrink_ladder_frames_device(edge, 32, 32, 0, 4, [1.0, 0.5])  # shrink_by has no such restriction
    torch.cuda.synchronize()


def test_one_handle_over_a_mixed_sequence(product, oracle):
    """single(k0) -> ladder -> single(k1) -> ladder at another tile size -> single(k0), queued on one handle into poisoned buffers,
    each equal to a fresh handle's result"""
    import torch
    imgs = [oracle.synth_frame(1280, 720, 4, 100 + f, 1 if f < 2 else 0) for f in range(3)]
    frames = torch.from_numpy(np.stack(imgs)).cuda()
    N = frames.shape[0]

    def poisoned(shape_lead, T, slot):
        vals = torch.empty(shape_lead + (T,), dtype=torch.float32, device="cuda")
        vals.view(torch.int32).fill_(-1)
        ow = torch.full(shape_lead + (T,), -1, dtype=torch.int32, device="cuda")
        oh = torch.full(shape_lead + (T,), -1, dtype=torch.int32, device="cuda")
        slots = torch.full(shape_lead + (T, slot), 0xA5, dtype=torch.uint8, device="cuda")
        return vals, ow, oh, slots

    T32, T64 = product.grid(1280, 720, 32, 32), product.grid(1280, 720, 64, 64)
    T32, T64 = T32[0] * T32[1], T64[0] * T64[1]
    lad_a, lad_b = [0.5, 0.125, 2.0], [0.25, 1.0]
    steps = [("single", 32, 0.5), ("ladder", 32, lad_a), ("single", 32, 0.125), ("ladder", 64, lad_b), ("single", 32, 0.5)]
    h = product.Handle(0)
    outs = []
    for kind, block, k in steps:
        T = T32 if block == 32 else T64
        if kind == "single":
            o = poisoned((N,), T, block * block * 4)
            h.shrink_frames_device(frames, block, block, 0, 4, k, out=o)
        else:
            o = poisoned((len(k), N), T, block * block * 4)
            h.shrink_ladder_frames_device(frames, block, block, 0, 4, k, out=o)
        outs.append(o)
    torch.cuda.synchronize()
    h.close()
    for (kind, block, k), o in zip(steps, outs):
        fresh = product.Handle(0)
        if kind == "single":
            ref = fresh.shrink_frames_device(frames, block, block, 0, 4, k)
            torch.cuda.synchronize()
            for f in range(N):
                assert_same_tiles(host1(o, f), host1(ref, f), 4, f"{kind} {block} {k} frame {f}")
        else:
            ref = fresh.shrink_ladder_frames_device(frames, block, block, 0, 4, k)
            torch.cuda.synchronize()
            for r in range(len(k)):
                for f in range(N):
                    assert_same_tiles(host(o, r, f), host(ref, r, f), 4, f"{kind} {block} rung {r} frame {f}")
        fresh.close()
    for f in range(N):
        exp = oracle.shrink_image(imgs[f], 32, 32, 0, 4, 0.125, nthreads=8)
        assert_same_tiles(host(outs[1], 1, f), exp, 4, f"ladder rung 1 frame {f} vs oracle")


def test_full_size_five_rungs(gpu):
    """8 x 7680x4320 RGBA, 32x32, Lanczos3, shrink_by at 5 factors: every rung equals its single call.  The rung sets hold
    5.3 GB of slots: rungs 1.. lie beyond 4 GiB."""
    import torch
    factors = [1.0, 0.5, 0.25, 2.0, 0.125]
    frames = gpu.synth_frames_device(8, 4320, 7680, 4, first_frame=0, dist=0)
    lv, lw, lh, ls = gpu.shrink_ladder_frames_device(frames, 32, 32, 0, 4, factors)
    assert ls.numel() > (4 << 30)
    one = None
    for r, k in enumerate(factors):
        one = gpu.shrink_frames_device(frames, 32, 32, 0, 4, k, out=one)
        torch.cuda.synchronize()
        sv, sw, sh, ss = one
        assert (lv[r].view(torch.int32) == sv.view(torch.int32)).all(), f"rung {r}: values"
        assert (lw[r] == sw).all() and (lh[r] == sh).all(), f"rung {r}: sizes"
        valid = (sw.long() * sh.long() * 4).reshape(-1)
        a, b = ls[r].reshape(valid.numel(), -1), ss.reshape(valid.numel(), -1)
        lane = torch.arange(a.shape[1], device=a.device)[None, :]
        chunk = (256 << 20) // a.shape[1]
        bad = 0
        for t0 in range(0, a.shape[0], chunk):
            t1 = min(a.shape[0], t0 + chunk)
            bad += int(((a[t0:t1] != b[t0:t1]) & (lane < valid[t0:t1, None])).sum())
        assert bad == 0, f"rung {r}: {bad} payload bytes differ"


def test_host_buffer_ladder_equals_device_call(gpu, oracle):
    import torch
    for c, block, mode, factors in ((4, 32, 0, [0.5, 0.125, 2.0]), (3, 64, 0, [1.0, 0.25]), (4, 16, 1, [16.0, 2.0])):
        img = oracle.synth_frame(700, 420, c, 7, 1 if c == 4 else 0)
        got = gpu.shrink_image_ladder(img, block, block, mode, 4, factors)
        dev = gpu.shrink_ladder_frames_device(torch.from_numpy(img[None].copy()).cuda(), block, block, mode, 4, factors)
        torch.cuda.synchronize()
        for r in range(len(factors)):
            assert_same_tiles((got[0][r], got[1][r], got[2][r], got[3][r]), host(dev, r), c, f"host ladder c{c} {block} rung {r}")
