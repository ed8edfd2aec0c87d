"""Batches of differently sized images (pxz_shrink_varied_frames_device, pxz_encode_varied_frames_device,
pxz_encode_varied_images): every image's tiles and file equal the single-geometry call on that image alone and the oracle,
bit for bit -- value bits, sizes, the valid slot bytes, file bytes -- with every output poisoned before each call."""
import os

import numpy as np
import pytest
from PIL import Image

from test_gpu_parity import assert_same_tiles

pytestmark = pytest.mark.gpu

POISON = 0xA5


@pytest.fixture(scope="module")
def gpu(product):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    h = product.Handle(0)
    yield h
    h.close()


def make_image(rng, w, h, c, alpha):
    img = rng.integers(0, 256, (h, w, c), dtype=np.uint8)
    # smooth areas too, so that tiles land on many levels
    yy, xx = np.mgrid[0:h, 0:w]
    smooth = ((xx * 3 + yy * 5) % 256).astype(np.uint8)
    mask = ((xx // 23 + yy // 17) % 3) == 0
    for ch in range(3):
        img[..., ch] = np.where(mask, smooth, img[..., ch])
    if c == 4:
        if alpha == "opaque":
            img[..., 3] = 255
        elif alpha == "clear":
            img[..., 3] = 0
        else:
            img[..., 3] = np.where(((xx // 9 + yy // 7) % 2) == 0, 255, img[..., 3])
    return img


def upload(images, c, pad=0, misalign=0):
    """one CUDA buffer holding every image at an odd offset (misalign) and with padded rows (pad bytes) -> (buf, geoms)"""
    import torch
    geoms, chunks, off = [], [], 0
    for k, img in enumerate(images):
        h, w, _ = img.shape
        pitch = w * c + (pad * (k % 3))
        lead = (misalign * (k % 5)) if misalign else 0
        block = np.zeros(lead + pitch * h, np.uint8)
        rows = block[lead:].reshape(h, pitch)
        rows[:, :w * c] = img.reshape(h, w * c)
        chunks.append(block)
        geoms.append((w, h, pitch, off + lead))
        off += block.size
    buf = torch.from_numpy(np.concatenate(chunks)).cuda()
    return buf, geoms


def poisoned(T, slot, dev):
    import torch
    vals = torch.full((T,), 0, dtype=torch.int32, device=dev).fill_(0x7F7F7F7F).view(torch.float32)
    ow = torch.full((T,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    oh = torch.full((T,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    slots = torch.full((T, slot), POISON, dtype=torch.uint8, device=dev)
    return vals, ow, oh, slots


def varied(gpu, product, buf, geoms, c, bw, bh, mode, filt, factor):
    import torch
    offs = product.varied_layout(geoms, bw, bh)
    out = poisoned(int(offs[-1]), bw * bh * c, buf.device)
    res = gpu.shrink_varied_frames_device(buf, bw, bh, mode, filt, factor, descs=geoms, channels=c, out=out)
    torch.cuda.synchronize()
    return res


def tiles_of(res, i):
    offs, vals, ow, oh, slots = res
    a, b = int(offs[i]), int(offs[i + 1])
    return (vals[a:b].cpu().numpy(), ow[a:b].cpu().numpy().astype(np.uint32), oh[a:b].cpu().numpy().astype(np.uint32),
            None if slots is None else slots[a:b].cpu().numpy())


def single(gpu, buf, geom, c, bw, bh, mode, filt, factor):
    """pxz_shrink_frames_device on one image of the buffer, in place (same pitch and offset)"""
    import torch
    w, h, pitch, off = geom
    frame = torch.as_strided(buf, (1, h, w, c), (pitch * h, pitch, c, 1), off)
    vals, ow, oh, slots = gpu.shrink_frames_device(frame, bw, bh, mode, filt, factor)
    torch.cuda.synchronize()
    return (vals[0].cpu().numpy(), ow[0].cpu().numpy().astype(np.uint32), oh[0].cpu().numpy().astype(np.uint32),
            slots[0].cpu().numpy())


def check_batch(gpu, product, oracle, images, c, bw, bh, mode, filt, factor, pad=0, misalign=0, with_oracle=True, what=""):
    buf, geoms = upload(images, c, pad, misalign)
    res = varied(gpu, product, buf, geoms, c, bw, bh, mode, filt, factor)
    for i, img in enumerate(images):
        got = tiles_of(res, i)
        assert_same_tiles(got, single(gpu, buf, geoms[i], c, bw, bh, mode, filt, factor), c, f"{what} image {i} {img.shape} vs single")
        if with_oracle:
            exp = oracle.shrink_image(np.ascontiguousarray(img), bw, bh, mode, filt, factor, nthreads=8)
            assert_same_tiles(got, exp, c, f"{what} image {i} {img.shape} vs oracle")
    return buf, geoms, res


def random_sizes(rng, n, lo, hi):
    return [(int(rng.integers(lo, hi + 1)), int(rng.integers(lo, hi + 1))) for _ in range(n)]


TILES = [(16, 16), (32, 32), (64, 64), (48, 20), (37, 61)]


@pytest.mark.parametrize("mode,factor", [(0, 1.0), (1, 16.0)])
@pytest.mark.parametrize("filt", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("tile", TILES, ids=lambda t: f"{t[0]}x{t[1]}")
def test_random_batches_equal_single_calls_and_oracle(gpu, product, oracle, mode, factor, filt, tile):
    bw, bh = tile
    seed = hash((mode, filt, bw, bh)) & 0xffff
    rng = np.random.default_rng(seed)
    c = 4 if (filt + bw) % 2 == 0 else 3
    lo = 2 if mode == 1 else 1
    sizes = random_sizes(rng, int(rng.integers(1, 9)), lo, 300) + [(lo, lo), (bw - 1 if bw > lo else bw, bh)]
    if mode == 1:  # directional: every edge at least 2 px
        sizes = [(w if w % bw != 1 else w + 1, h if h % bh != 1 else h + 1) for (w, h) in sizes]
    alphas = ["opaque", "partial", "clear"]
    images = [make_image(rng, w, h, c, alphas[k % 3]) for k, (w, h) in enumerate(sizes)]
    check_batch(gpu, product, oracle, images, c, bw, bh, mode, filt, factor, pad=4 * (seed % 3) + 3, misalign=seed % 7 + 1,
                what=f"mode {mode} filter {filt} {bw}x{bh} C{c}")


@pytest.mark.parametrize("mode,factor", [(0, 0.5), (1, 8.0)])
@pytest.mark.parametrize("c", [4, 3])
def test_every_edge_width_of_one_tile_size(gpu, product, oracle, mode, factor, c):
    bw = bh = 32
    rng = np.random.default_rng(7 + c + mode)
    first = 2 if mode == 1 else 1
    images = [make_image(rng, 2 * bw + e, bh + e, c, "partial") for e in range(first, bw + 1)]
    check_batch(gpu, product, oracle, images, c, bw, bh, mode, 4, factor, misalign=1, what="edges")


def test_n_images_1_equals_the_single_call(gpu, product, oracle):
    rng = np.random.default_rng(3)
    for (w, h, c, bw, bh, mode) in [(333, 217, 4, 32, 32, 0), (640, 360, 3, 64, 64, 1), (17, 5, 4, 16, 16, 0)]:
        img = make_image(rng, w, h, c, "partial")
        check_batch(gpu, product, oracle, [img], c, bw, bh, mode, 4, 1.0 if mode == 0 else 16.0, what="n=1")


def test_equal_geometries_equal_the_frames_call(gpu, product):
    import torch
    for mode, factor in ((0, 1.0), (1, 16.0)):
        frames = gpu.synth_frames_device(6, 360, 640, 4, dist=product.DIST_ALPHA)
        torch.cuda.synchronize()
        buf = frames.reshape(-1)
        geoms = [(640, 360, 640 * 4, k * 640 * 360 * 4) for k in range(6)]
        res = varied(gpu, product, buf, geoms, 4, 32, 32, mode, 4, factor)
        vals, ow, oh, slots = gpu.shrink_frames_device(frames, 32, 32, mode, 4, factor)
        torch.cuda.synchronize()
        for f in range(6):
            exp = (vals[f].cpu().numpy(), ow[f].cpu().numpy().astype(np.uint32), oh[f].cpu().numpy().astype(np.uint32),
                   slots[f].cpu().numpy())
            assert_same_tiles(tiles_of(res, f), exp, 4, f"mode {mode} frame {f}")


def test_golden_images_in_a_batch_and_the_base_file(gpu, product, oracle, golden_dir):
    import torch
    base = np.array(Image.open(os.path.join(golden_dir, "base.png")).convert("RGBA"))
    big = np.array(Image.open(os.path.join(golden_dir, "Big-Ruscher.png")).convert("RGBA"))
    rng = np.random.default_rng(11)
    images = [make_image(rng, 97, 61, 4, "partial"), base, make_image(rng, 5, 3, 4, "opaque"), big, make_image(rng, 640, 200, 4, "clear")]
    for mode, factor in ((0, 1.0), (1, 16.0)):
        buf, geoms, res = check_batch(gpu, product, oracle, images, 4, 64, 64, mode, 4, factor, what=f"golden mode {mode}")
        offs, vals, ow, oh, slots = res
        sizes = [(g[0], g[1]) for g in geoms]
        foffs, fbuf = gpu.encode_varied_frames_device(sizes, 4, 64, 64, vals, ow, oh, slots)
        torch.cuda.synchronize()
        fo = foffs.cpu().numpy()
        data = fbuf.cpu().numpy()
        for i, img in enumerate(images):
            mine = data[fo[i]:fo[i + 1]].tobytes()
            ev, ew, eh, es = oracle.shrink_image(np.ascontiguousarray(img), 64, 64, mode, 4, factor, nthreads=8)
            exp = oracle.encode_container(img.shape[1], img.shape[0], 64, 64, 4, 0, ev, None, ew, eh, es)
            assert mine == exp, f"mode {mode} image {i}: file differs from the oracle writer's"


def test_varied_writer_equals_the_frames_writer(gpu, product):
    import torch
    rng = np.random.default_rng(5)
    for c, (bw, bh) in ((4, (32, 32)), (3, (16, 16)), (4, (48, 20))):
        sizes = random_sizes(rng, 12, 1, 260) + [(1, 1), (bw, bh)]
        images = [make_image(rng, w, h, c, "partial") for (w, h) in sizes]
        buf, geoms = upload(images, c)
        res = varied(gpu, product, buf, geoms, c, bw, bh, 0, 4, 1.0)
        offs, vals, ow, oh, slots = res
        foffs, fbuf = gpu.encode_varied_frames_device(sizes, c, bw, bh, vals, ow, oh, slots)
        torch.cuda.synchronize()
        fo = foffs.cpu().numpy()
        data = fbuf.cpu().numpy()
        assert fo[0] == 0
        for i, (w, h) in enumerate(sizes):
            a, b = int(offs[i]), int(offs[i + 1])
            one = gpu.encode_frames_device((1, h, w, c), bw, bh, vals[a:b].contiguous(), ow[a:b].contiguous(), oh[a:b].contiguous(),
                                           slots[a:b].contiguous())
            torch.cuda.synchronize()
            o1 = one[0].cpu().numpy()
            exp = one[1].cpu().numpy()[o1[0]:o1[1]].tobytes()
            assert data[fo[i]:fo[i + 1]].tobytes() == exp, f"C{c} {bw}x{bh} image {i} ({w}x{h})"
        # truncated: the offsets stay exact, nothing is written past the capacity
        cap = int(fo[len(sizes) // 2]) + 7
        out_offs = torch.empty(len(sizes) + 1, dtype=torch.int64, device=vals.device)
        small = torch.full((cap + 64,), POISON, dtype=torch.uint8, device=vals.device)
        gpu.encode_varied_frames_device(sizes, c, bw, bh, vals, ow, oh, slots, out=(out_offs, small[:cap]))
        torch.cuda.synchronize()
        assert (out_offs.cpu().numpy() == fo).all()
        assert (small[cap:].cpu().numpy() == POISON).all()


def test_host_form_equals_the_oracle_per_image(gpu, product, oracle):
    rng = np.random.default_rng(9)
    for c, mode, factor in ((4, 0, 1.0), (3, 1, 16.0)):
        sizes = random_sizes(rng, 10, 2, 400) + [(2, 2)]
        sizes = [(w if w % 32 != 1 else w + 1, h if h % 32 != 1 else h + 1) for (w, h) in sizes]
        images = [make_image(rng, w, h, c, "partial") for (w, h) in sizes]
        files = gpu.encode_varied_images(images, 32, 32, mode, 2, factor)
        for i, img in enumerate(images):
            ev, ew, eh, es = oracle.shrink_image(img, 32, 32, mode, 2, factor, nthreads=8)
            assert files[i] == oracle.encode_container(img.shape[1], img.shape[0], 32, 32, c, 0, ev, None, ew, eh, es), i


def test_single_varied_single_sequence_on_one_handle_equals_fresh_handles(gpu, product):
    import torch
    rng = np.random.default_rng(21)
    frames = gpu.synth_frames_device(2, 300, 520, 4, dist=product.DIST_ALPHA)
    torch.cuda.synchronize()
    imgs_a = [make_image(rng, w, h, 4, "partial") for (w, h) in random_sizes(rng, 6, 1, 200)]
    imgs_b = [make_image(rng, w, h, 4, "opaque") for (w, h) in random_sizes(rng, 6, 1, 200)]
    buf_a, geo_a = upload(imgs_a, 4, misalign=3)
    buf_b, geo_b = upload(imgs_b, 4, pad=16)

    steps = [("single", None), ("varied", (buf_a, geo_a, 32, 32)), ("single", None), ("varied", (buf_b, geo_b, 64, 64)), ("single", None)]

    def run(h, step):
        """-> a list of (values, w, h, slots) host tuples: one per frame, or the whole varied batch"""
        kind, arg = step
        if kind == "single":
            vals, ow, oh, slots = h.shrink_frames_device(frames, 32, 32, 0, 4, 1.0)
            torch.cuda.synchronize()
            return [(vals[f].cpu().numpy(), ow[f].cpu().numpy().astype(np.uint32), oh[f].cpu().numpy().astype(np.uint32),
                     slots[f].cpu().numpy()) for f in range(frames.shape[0])]
        b, g, bw, bh = arg
        _, vals, ow, oh, slots = h.shrink_varied_frames_device(b, bw, bh, 0, 4, 1.0, descs=g, channels=4)
        torch.cuda.synchronize()
        return [(vals.cpu().numpy(), ow.cpu().numpy().astype(np.uint32), oh.cpu().numpy().astype(np.uint32), slots.cpu().numpy())]

    shared = [run(gpu, s) for s in steps]
    for k, (s, got) in enumerate(zip(steps, shared)):
        fresh = product.Handle(0)
        try:
            exp = run(fresh, s)
        finally:
            fresh.close()
        for g, e in zip(got, exp):
            assert_same_tiles(g, e, 4, f"step {k} ({s[0]}) on a used handle vs a fresh one")


def test_errors_name_the_image_and_write_nothing(gpu, product):
    import torch
    rng = np.random.default_rng(2)
    images = [make_image(rng, w, h, 4, "opaque") for (w, h) in [(40, 40), (33, 20), (50, 60)]]
    buf, geoms = upload(images, 4)
    T = int(product.varied_layout(geoms, 16, 16)[-1])
    cases = [
        (1, 16, 16, [geoms[0], geoms[1], (geoms[2][0], geoms[2][1], geoms[2][2], geoms[2][3])], -4, "image 1"),  # 33 = 2*16 + 1
        (0, 16, 16, [geoms[0], (geoms[1][0], geoms[1][1], 4, geoms[1][3]), geoms[2]], -1, "image 1"),           # pitch < row
        (0, 16, 16, [geoms[0], geoms[1], (0, 10, 40, 0)], -1, "image 2"),                                       # empty image
        (0, 16, 16, [geoms[0], geoms[1], geoms[2] + (1,)], -1, "image 2"),                                     # reserved
    ]
    for mode, bw, bh, g, code, name in cases:
        out = poisoned(T, bw * bh * 4, buf.device)
        with pytest.raises(product.PxzError) as e:
            gpu.shrink_varied_frames_device(buf, bw, bh, mode, 4, 1.0, descs=g, channels=4, out=out)
        assert e.value.code == code
        assert name in product.binding.load_library().pxz_last_error(gpu._h).decode()
        torch.cuda.synchronize()
        vals, ow, oh, slots = out
        assert (vals.view(torch.int32) == 0x7F7F7F7F).all() and (ow == 0x5A5A5A5A).all() and (oh == 0x5A5A5A5A).all()
        assert (slots == POISON).all()
    # a tile image beyond this path's LDS limit
    with pytest.raises(product.PxzError) as e:
        gpu.shrink_varied_frames_device(buf, 160, 160, 0, 4, 1.0, descs=geoms, channels=4)
    assert e.value.code == -5


def test_full_size_frames_mixed_with_hundreds_of_small_images(gpu, product):
    import torch
    rng = np.random.default_rng(99)
    for mode, factor in ((0, 1.0), (1, 16.0)):
        big = gpu.synth_frames_device(3, 4320, 7680, 4, dist=product.DIST_ALPHA)
        torch.cuda.synchronize()
        sizes = [(w if w % 64 != 1 else w + 1, h if h % 64 != 1 else h + 1) for (w, h) in random_sizes(rng, 300, 2, 120)]
        small = [make_image(rng, w, h, 4, "partial") for (w, h) in sizes]
        sbuf, sgeo = upload(small, 4, misalign=1)
        buf = torch.cat([big.reshape(-1), sbuf])
        n_big = 3
        frame_bytes = 7680 * 4320 * 4
        geoms = [(7680, 4320, 7680 * 4, k * frame_bytes) for k in range(n_big)]
        geoms += [(w, h, p, n_big * frame_bytes + o) for (w, h, p, o) in sgeo]
        order = list(range(len(geoms)))
        rng.shuffle(order)
        geoms = [geoms[k] for k in order]
        res = varied(gpu, product, buf, geoms, 4, 64, 64, mode, 4, factor)
        for i, g in enumerate(geoms):
            if g[0] == 7680 or i % 10 == 0:
                assert_same_tiles(tiles_of(res, i), single(gpu, buf, g, 4, 64, 64, mode, 4, factor), 4, f"mode {mode} image {i} {g[:2]}")
        del big, buf
        torch.cuda.empty_cache()
