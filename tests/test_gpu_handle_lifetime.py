"""What a handle owns, over its lifetime: the pinned staging blocks of the ladder's factors and of the varied per-image table
across pxz_trim, the bounded table caches (tree, varied, varied expand: 16 sets each) past their bound, and handles created,
used and destroyed beside each other.  Every result is compared with the oracle.  The images are tiny on purpose: what can go
wrong here is ownership, not arithmetic."""
import numpy as np
import pytest

from test_gpu_ladder import host
from test_gpu_parity import assert_same_tiles
from test_gpu_varied import make_image, poisoned, tiles_of, upload
from test_gpu_varied_decode import oracle_tiles

pytestmark = pytest.mark.gpu

CACHE_BOUND = 16  # sets per bounded cache
N_BATCHES = CACHE_BOUND + 2  # the bound, one more to force the eviction, and one more


@pytest.fixture
def handle(product):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    h = product.Handle(0)
    yield h
    h.close()


def oracle_file(oracle, img, bw, bh, mode, filt, factor):
    h, w, c = img.shape
    ev, ew, eh, es = oracle.shrink_image(np.ascontiguousarray(img), bw, bh, mode, filt, factor, nthreads=8)
    return oracle.encode_container(w, h, bw, bh, c, 0, ev, None, ew, eh, es)


def oracle_image(oracle, raw, size, bw, bh, c, filt):
    _, tw, th, slots = oracle_tiles(oracle, raw)
    return oracle.expand_image(size[0], size[1], bw, bh, c, filt, tw, th, slots[:, : bw * bh * c].copy())


def test_pinned_staging_across_a_trim(handle, product, oracle):
    """ladder (3 factors) -> trim -> ladder (5) -> host encode of 3 images -> trim -> of 5 images (the pinned per-image table
    is made anew, then again larger) -> host decode -> trim -> host decode; nothing synchronises but the calls themselves"""
    import torch
    bw = bh = 32
    imgs = [oracle.synth_frame(96, 80, 4, 3 + f, f % 2) for f in range(2)]  # 80 = 2 * 32 + 16: a ragged last tile row
    frames = torch.from_numpy(np.stack(imgs)).cuda()
    lad3, lad5 = [0.5, 0.125, 2.0], [1.0, 0.25, 0.5, 4.0, 0.06]
    rng = np.random.default_rng(41)
    three = [make_image(rng, w, h, 4, "partial") for (w, h) in [(70, 45), (32, 32), (101, 64)]]
    five = [make_image(rng, w, h, 4, a) for (w, h), a in zip([(33, 90), (64, 1), (5, 7), (97, 31), (40, 66)],
                                                            ["opaque", "partial", "clear", "partial", "opaque"])]

    out3 = handle.shrink_ladder_frames_device(frames, bw, bh, 0, 4, lad3)
    handle.trim()
    out5 = handle.shrink_ladder_frames_device(frames, bw, bh, 0, 4, lad5)
    files3 = handle.encode_varied_images(three, bw, bh, 0, 4, 1.0)
    handle.trim()
    files5 = handle.encode_varied_images(five, bw, bh, 0, 4, 1.0)
    back_a, flags_a = handle.decode_varied_files(files5, 4, bw, bh, 4)
    handle.trim()
    back_b, flags_b = handle.decode_varied_files(files5, 4, bw, bh, 4)
    torch.cuda.synchronize()

    for factors, out, name in ((lad3, out3, "3 rungs"), (lad5, out5, "5 rungs after a trim")):
        for r, k in enumerate(factors):
            for f, img in enumerate(imgs):
                exp = oracle.shrink_image(img, bw, bh, 0, 4, k, nthreads=8)
                assert_same_tiles(host(out, r, f), exp, 4, f"ladder of {name}, rung {r} frame {f}")
    for images, files, name in ((three, files3, "3 images"), (five, files5, "5 images after a trim")):
        assert len(files) == len(images)
        for i, img in enumerate(images):
            assert files[i] == oracle_file(oracle, img, bw, bh, 0, 4, 1.0), f"encode of {name}: file {i}"
    for back, flags, name in ((back_a, flags_a, "decode"), (back_b, flags_b, "decode after a trim")):
        assert (flags == 0).all()
        for i, img in enumerate(five):
            exp = oracle_image(oracle, files5[i], (img.shape[1], img.shape[0]), bw, bh, 4, 4)
            assert (back[i] == exp).all(), f"{name}: image {i}"


def test_bounded_varied_caches_evict_and_rebuild(handle, product, oracle):
    """18 batches whose sets of tile sides all differ, then the first again, through the shrinker (queued back to back) and
    through the host decode: the caches of 16 table sets are emptied on the way and every batch still equals the oracle"""
    import torch
    bw = bh = 32
    c, filt = 4, 4
    rng = np.random.default_rng(43)
    batches = []
    for k in range(N_BATCHES):
        sizes = [(34 + k, 40), (50, 35 + k)]  # tile sides {32, 2 + k, 8, 18, 3 + k}: another set for every k, every edge >= 2
        batches.append([make_image(rng, w, h, c, ["partial", "opaque"][(k + j) % 2]) for j, (w, h) in enumerate(sizes)])
    order = list(range(N_BATCHES)) + [0]
    expected = [[oracle.shrink_image(np.ascontiguousarray(img), bw, bh, 0, filt, 1.0, nthreads=8) for img in b] for b in batches]

    uploaded = [upload(b, c) for b in batches]
    results = []
    for k in order:
        buf, geoms = uploaded[k]
        T = int(product.varied_layout(geoms, bw, bh)[-1])
        results.append(handle.shrink_varied_frames_device(buf, bw, bh, 0, filt, 1.0, descs=geoms, channels=c,
                                                          out=poisoned(T, bw * bh * c, buf.device)))
    torch.cuda.synchronize()
    for n, k in enumerate(order):
        for i in range(2):
            assert_same_tiles(tiles_of(results[n], i), expected[k][i], c, f"shrink call {n} (batch {k}) image {i}")

    files = [[oracle.encode_container(img.shape[1], img.shape[0], bw, bh, c, 0, e[0], None, e[1], e[2], e[3])
              for img, e in zip(b, exp)] for b, exp in zip(batches, expected)]
    images = [[oracle_image(oracle, raw, (img.shape[1], img.shape[0]), bw, bh, c, filt) for img, raw in zip(b, fs)]
              for b, fs in zip(batches, files)]
    for n, k in enumerate(order):
        back, flags = handle.decode_varied_files(files[k], c, bw, bh, filt)
        assert (flags == 0).all()
        for i in range(2):
            assert (back[i] == images[k][i]).all(), f"decode call {n} (batch {k}) image {i}"


def test_bounded_tree_cache_evicts_and_rebuilds(handle, oracle):
    """tree::process on rectangle lists (50 -> 25 -> 12) over 18 frame widths, then the first again"""
    order = list(range(N_BATCHES)) + [0]
    frames = [handle.synth_frames_device(1, 60, 100 + k, 4, first_frame=17 + k, dist=0) for k in range(N_BATCHES)]
    outs = [handle.tree_process_frames_device(frames[k], 50, 50, 0.03, 4, 4, 4, 0) for k in order]
    for n, k in enumerate(order):
        exp = oracle.tree_process_image(frames[k].cpu().numpy()[0], 50, 50, 0.03, 4, 4, 4, 0)
        assert (outs[n].cpu().numpy()[0] == exp).all(), f"call {n} (width {100 + k})"
    assert handle.decode_status() == 0


def test_create_use_destroy_twice_over(product, oracle):
    """two handles alive at once; the first is closed and the second goes on; a third is made after both are gone"""
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    rng = np.random.default_rng(47)
    img = make_image(rng, 75, 41, 4, "partial")
    batch = [make_image(rng, w, h, 4, "partial") for (w, h) in [(70, 45), (9, 33)]]
    exp_tiles = oracle.shrink_image(img, 32, 32, 0, 4, 1.0, nthreads=8)
    exp_files = [oracle_file(oracle, b, 32, 32, 0, 4, 1.0) for b in batch]

    def use(h, what):
        assert_same_tiles(h.shrink_image(img, 32, 32, 0, 4, 1.0), exp_tiles, 4, f"{what}: shrink_image")
        assert h.encode_varied_images(batch, 32, 32, 0, 4, 1.0) == exp_files, f"{what}: encode_varied_images"

    first, second = product.Handle(0), product.Handle(0)
    try:
        use(first, "first of two")
        use(second, "second of two")
        first.close()
        use(second, "second, the first closed")
    finally:
        first.close()
        second.close()
    third = product.Handle(0)
    try:
        use(third, "third")
    finally:
        third.close()
