"""The varied ladder (pxz_shrink_varied_ladder_frames_device, pxz_rate_distortion_varied_images): a batch of differently sized
images at several factors in one launch.  Rung r equals pxz_shrink_varied_frames_device at factors[r] and the oracle, bit for
bit -- value bits, sizes, the valid slot bytes -- with every output poisoned before each call and a guard rung behind the last
one that must stay untouched.

The kernel stages a tile once and resamples it once per distinct pair of levels, so it can go wrong where the single-factor
kernel cannot: a later pair reading a source an earlier pair overwrote, a clone stored after the premultiply, one axis taking
the other's table, a small block's images overrunning their LDS.  The first test asserts from the single-factor results that
each of its cases holds tiles on which these would show."""
import os

import numpy as np
import pytest
from PIL import Image

from test_gpu_distortion import expected_tiles
from test_gpu_parity import assert_same_tiles
from test_gpu_varied import make_image, single, upload

pytestmark = pytest.mark.gpu

POISON = 0xA5
POISON_VAL, POISON_DIM = 0x7F7F7F7F, 0x5A5A5A5A
INVALID_ARG, TILE_TOO_SMALL, UNSUPPORTED = -1, -4, -5
# unsorted on purpose: a rung's place in the list must not matter
FACTORS = {0: [1, .5, .25, .125, 2, .05, .02, .01], 1: [16, 8, 4, 2, 1, .5, 32, .1]}
TILES = [(32, 32), (64, 64), (16, 16), (48, 20), (37, 61)]
# per tile size: a main image of several tiles, one smaller than a block, two with other edge widths (no edge of 1 px, either
# way round: directional batches hold every image and its transpose)
SIZES = {(32, 32): [(100, 70), (20, 9), (77, 45), (66, 35)],
         (64, 64): [(130, 67), (40, 30), (150, 100), (70, 131)],
         (16, 16): [(50, 34), (9, 5), (83, 61), (35, 20)],
         (48, 20): [(100, 38), (30, 11), (150, 63), (52, 45)],
         (37, 61): [(100, 70), (20, 40), (113, 125), (76, 64)]}
ALPHAS = ["partial", "clear", "opaque"]


@pytest.fixture(scope="module")
def gpu(product):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    h = product.Handle(0)
    yield h
    h.close()


def batch_images(tile, mode, filt):
    """-> (images, channels, alpha kind per image) of one case of the first test"""
    c = 4 if (filt + TILES.index(tile)) % 2 == 0 else 3
    rng = np.random.default_rng(1000 * mode + 10 * filt + TILES.index(tile))
    sizes = SIZES[tile]
    if mode == 0:
        sizes = sizes + [(1, 1), (57, 1)]
    else:
        sizes = sizes[:3]
    kinds = [ALPHAS[k % 3] for k in range(len(sizes))]
    images = [make_image(rng, w, h, c, kinds[k]) for k, (w, h) in enumerate(sizes)]
    if mode == 1:
        # rows of one colour each under a little noise: a strong gradient down, a weak one across, so that one axis keeps its
        # size on rungs where the other shrinks
        img = images[2]
        rows = rng.integers(0, 256, (img.shape[0], 1, 3))
        img[..., :3] = np.clip(rows + rng.integers(-2, 3, img[..., :3].shape), 0, 255).astype(np.uint8)
        # each image with its transpose: what is H-only in the one is V-only in the other
        images = [x for img in images for x in (img, np.ascontiguousarray(img.transpose(1, 0, 2)))]
        kinds = [k for k in kinds for _ in range(2)]
    return images, c, kinds


def tile_geometry(geoms, bw, bh):
    """full size, owner and edge flag of every tile of a batch, in the varied layout"""
    fw, fh, owner = [], [], []
    for i, (w, h, _, _) in enumerate(geoms):
        cols, rows = -(-w // bw), -(-h // bh)
        for ty in range(rows):
            for tx in range(cols):
                fw.append(min(bw, w - tx * bw))
                fh.append(min(bh, h - ty * bh))
                owner.append(i)
    fw, fh = np.array(fw, np.uint32), np.array(fh, np.uint32)
    return fw, fh, np.array(owner), (fw < bw) | (fh < bh)


def hazards(rungs, geoms, bw, bh):
    """what the single-factor results (one (values, w, h, slots) per rung) say about the tiles of a batch"""
    fw, fh, owner, edge = tile_geometry(geoms, bw, bh)
    ow = np.stack([r[1] for r in rungs]).astype(np.int64)
    oh = np.stack([r[2] for r in rungs]).astype(np.int64)
    clone = (ow == fw) & (oh == fh)
    code = ow * 65536 + oh
    reduced = np.array([len(set(code[~clone[:, t], t].tolist())) for t in range(fw.size)])
    sizes = np.array([len(set(code[:, t].tolist())) for t in range(fw.size)])
    return dict(clone_and_3_reduced=clone.any(0) & (reduced >= 3), clone_and_reduced=clone.any(0) & (~clone).any(0), owner=owner,
                h_only=((ow < fw) & (oh == fh)).any(), v_only=((ow == fw) & (oh < fh)).any(), h_and_v=((ow < fw) & (oh < fh)).any(),
                edge_2_sizes=(edge & (sizes >= 2)).any(), sizes=sizes)


def host(t):
    vals, ow, oh, slots = t
    return (vals.cpu().numpy(), ow.cpu().numpy().astype(np.uint32), oh.cpu().numpy().astype(np.uint32),
            None if slots is None else slots.cpu().numpy())


def poisoned(shape, slot, dev, want_pixels=True):
    import torch
    vals = torch.full(shape, POISON_VAL, dtype=torch.int32, device=dev).view(torch.float32)
    ow = torch.full(shape, POISON_DIM, dtype=torch.int32, device=dev)
    oh = torch.full(shape, POISON_DIM, dtype=torch.int32, device=dev)
    slots = torch.full(shape + (slot,), POISON, dtype=torch.uint8, device=dev) if want_pixels else None
    return vals, ow, oh, slots


def still_poisoned(out):
    import torch
    vals, ow, oh, slots = out
    return bool((vals.view(torch.int32) == POISON_VAL).all() and (ow == POISON_DIM).all() and (oh == POISON_DIM).all() and
                (slots is None or (slots == POISON).all()))


def ladder(gpu, product, buf, geoms, c, bw, bh, mode, filt, factors, want_pixels=True, h=None):
    """one varied-ladder call into poisoned outputs with a guard rung behind the last -> a host (values, w, h, slots) per rung"""
    import torch
    K = len(factors)
    T = int(product.varied_layout(geoms, bw, bh)[-1])
    full = poisoned((K + 1, T), bw * bh * c, buf.device, want_pixels)
    out = tuple(None if x is None else x[:K] for x in full)
    (h or gpu).shrink_varied_ladder_frames_device(buf, bw, bh, mode, filt, factors, want_pixels=want_pixels, descs=geoms, channels=c, out=out)
    torch.cuda.synchronize()
    assert still_poisoned(tuple(None if x is None else x[K:] for x in full)), "the guard behind the last rung was written"
    vals, ow, oh, slots = host(out)
    return [(vals[r], ow[r], oh[r], None if slots is None else slots[r]) for r in range(K)]


def varied(gpu, product, buf, geoms, c, bw, bh, mode, filt, factor, h=None):
    """the single-factor varied call on the same buffer, into poisoned outputs -> host (values, w, h, slots)"""
    import torch
    T = int(product.varied_layout(geoms, bw, bh)[-1])
    out = poisoned((T,), bw * bh * c, buf.device)
    (h or gpu).shrink_varied_frames_device(buf, bw, bh, mode, filt, factor, descs=geoms, channels=c, out=out)
    torch.cuda.synchronize()
    return host(out)


def image_tiles(product, geoms, bw, bh, rung, i):
    offs = product.varied_layout(geoms, bw, bh)
    a, b = int(offs[i]), int(offs[i + 1])
    return tuple(None if x is None else x[a:b] for x in rung)


def check_rungs(gpu, product, buf, geoms, c, bw, bh, mode, filt, factors, what=""):
    """every rung of one varied-ladder call against the single-factor varied call -> (ladder rungs, single-factor rungs)"""
    got = ladder(gpu, product, buf, geoms, c, bw, bh, mode, filt, factors)
    exp = [varied(gpu, product, buf, geoms, c, bw, bh, mode, filt, k) for k in factors]
    for r, k in enumerate(factors):
        assert_same_tiles(got[r], exp[r], c, f"{what} rung {r} (factor {k}) vs the varied call")
    return got, exp


# ---- 1. rungs equal single-factor varied calls and the oracle ---------------------------------------------------------------

@pytest.mark.parametrize("mode", [0, 1], ids=["shrink_by", "directional"])
@pytest.mark.parametrize("filt", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("tile", TILES, ids=lambda t: f"{t[0]}x{t[1]}")
def test_rungs_equal_single_factor_calls_and_the_oracle(gpu, product, oracle, mode, filt, tile):
    bw, bh = tile
    factors = FACTORS[mode]
    images, c, kinds = batch_images(tile, mode, filt)
    seed = 10 * filt + TILES.index(tile) + mode
    buf, geoms = upload(images, c, pad=4 * (seed % 3) + 3, misalign=seed % 7 + 1)
    what = f"mode {mode} filter {filt} {bw}x{bh} C{c}"
    got, exp = check_rungs(gpu, product, buf, geoms, c, bw, bh, mode, filt, factors, what)
    for i, img in enumerate(images):
        for r, k in enumerate(factors):
            ref = oracle.shrink_image(np.ascontiguousarray(img), bw, bh, mode, filt, k, nthreads=8)
            assert_same_tiles(image_tiles(product, geoms, bw, bh, got[r], i), ref, c, f"{what} image {i} {img.shape} factor {k} vs oracle")
    # the tiles this case must hold for the comparison above to say anything about the kernel's own hazards
    hz = hazards(exp, geoms, bw, bh)
    assert hz["clone_and_3_reduced"].any(), "no tile with a clone rung and three reduced sizes: the staged tile is not re-read"
    if c == 4 and filt != 0:
        translucent = np.array([kinds[i] != "opaque" for i in hz["owner"]])
        assert (hz["clone_and_reduced"] & translucent).any(), "no translucent tile with a clone rung and a convolved rung"
    if mode == 1:
        assert hz["h_only"] and hz["v_only"] and hz["h_and_v"], "directional: H-only, V-only and H+V pairs must all occur"
    assert hz["edge_2_sizes"], "no edge tile with two sizes"


# ---- 2. small odd slots -----------------------------------------------------------------------------------------------------

def small_images(c, bw, mode, sizes):
    """plain noise, alpha included (make_image's smooth areas are wider than these images: every tile would be flat)"""
    rng = np.random.default_rng(50 + bw + mode)
    return [rng.integers(0, 256, (h, w, c), dtype=np.uint8) for (w, h) in sizes]


@pytest.mark.parametrize("c,bw,bh,sizes,mode", [(3, 5, 3, [(23, 11), (7, 5)], 0), (3, 5, 3, [(23, 11), (7, 5)], 1), (4, 3, 3, [(7, 7)], 0)],
                         ids=["5x3-rgb-shrink_by", "5x3-rgb-directional", "3x3-rgba-shrink_by"])
@pytest.mark.parametrize("filt", [0, 2, 4])
def test_small_odd_blocks(gpu, product, oracle, c, bw, bh, sizes, mode, filt):
    # a 45-byte slot puts the rungs' slots on every byte alignment; blocks this small are where I and F outgrow the tile
    images = small_images(c, bw, mode, sizes)
    buf, geoms = upload(images, c, misalign=1)
    factors = FACTORS[mode]
    got, exp = check_rungs(gpu, product, buf, geoms, c, bw, bh, mode, filt, factors, f"{bw}x{bh} C{c} mode {mode}")
    for i, img in enumerate(images):
        for r, k in enumerate(factors):
            ref = oracle.shrink_image(img, bw, bh, mode, filt, k, nthreads=1)
            assert_same_tiles(image_tiles(product, geoms, bw, bh, got[r], i), ref, c, f"{bw}x{bh} image {i} factor {k} vs oracle")
    assert (hazards(exp, geoms, bw, bh)["sizes"] >= 3).any(), "no tile with three sizes"


# ---- 3. the largest block ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", [0, 1], ids=["shrink_by", "directional"])
def test_largest_block(gpu, product, oracle, mode):
    # 128x129 leaves a 1 px edge, which the directional detector refuses: that mode takes 128x130
    rng = np.random.default_rng(128 + mode)
    images = [make_image(rng, 130, 130, 4, "partial"), make_image(rng, 128, 129 if mode == 0 else 130, 4, "partial")]
    buf, geoms = upload(images, 4, pad=4)
    factors = FACTORS[mode]
    got, exp = check_rungs(gpu, product, buf, geoms, 4, 128, 128, mode, 4, factors, f"128x128 mode {mode}")
    for i, img in enumerate(images):
        for r, k in enumerate(factors):
            ref = oracle.shrink_image(img, 128, 128, mode, 4, k, nthreads=8)
            assert_same_tiles(image_tiles(product, geoms, 128, 128, got[r], i), ref, 4, f"128x128 image {i} factor {k} vs oracle")
    assert hazards(exp, geoms, 128, 128)["clone_and_3_reduced"].any()


def test_a_block_beyond_the_limit_is_unsupported(gpu, product):
    import torch
    rng = np.random.default_rng(129)
    buf, geoms = upload([make_image(rng, 130, 130, 4, "partial")], 4)
    T = int(product.varied_layout(geoms, 129, 128)[-1])
    out = poisoned((2, T), 129 * 128 * 4, buf.device)
    with pytest.raises(product.PxzError) as e:
        gpu.shrink_varied_ladder_frames_device(buf, 129, 128, 0, 4, [1.0, 0.5], descs=geoms, channels=4, out=out)
    assert e.value.code == UNSUPPORTED
    torch.cuda.synchronize()
    assert still_poisoned(out)


# ---- 4. rung handling -------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def small_batch(product):
    rng = np.random.default_rng(4)
    images = [make_image(rng, w, h, 4, ALPHAS[k % 3]) for k, (w, h) in enumerate([(100, 70), (20, 9), (77, 45), (1, 1)])]
    buf, geoms = upload(images, 4, pad=5, misalign=3)
    return images, buf, geoms


def test_one_rung_equals_the_varied_call(gpu, product, small_batch):
    _, buf, geoms = small_batch
    for mode, k in ((0, 0.25), (1, 4.0)):
        g = geoms[:3]  # (directional: no 1x1 image)
        got, _ = check_rungs(gpu, product, buf, g, 4, 32, 32, mode, 4, [k], f"K=1 mode {mode}")
        for i in range(len(g)):  # and the single-geometry call on each image alone
            assert_same_tiles(image_tiles(product, g, 32, 32, got[0], i), single(gpu, buf, g[i], 4, 32, 32, mode, 4, k), 4, f"K=1 mode {mode} image {i}")


def test_32_rungs(gpu, product, small_batch):
    _, buf, geoms = small_batch
    factors = [float(2.0 ** (1.5 - 0.25 * r)) for r in range(32)]
    assert len(factors) == product.VARIED_LADDER_MAX_RUNGS
    _, exp = check_rungs(gpu, product, buf, geoms, 4, 32, 32, 0, 4, factors, "K=32")
    assert (hazards(exp, geoms, 32, 32)["sizes"] >= 4).any()


def test_repeated_and_reordered_factors(gpu, product, small_batch):
    _, buf, geoms = small_batch
    for mode in (0, 1):
        g = geoms if mode == 0 else geoms[:3]
        base = FACTORS[mode]
        first = ladder(gpu, product, buf, g, 4, 32, 32, mode, 4, base)
        rep = [base[0], base[3], base[0], base[3], base[3], base[1]]
        got = ladder(gpu, product, buf, g, 4, 32, 32, mode, 4, rep)
        for r, k in enumerate(rep):
            assert_same_tiles(got[r], first[base.index(k)], 4, f"mode {mode} repeated factor {k} at rung {r}")
        order = [5, 2, 7, 0, 3, 6, 1, 4]
        got = ladder(gpu, product, buf, g, 4, 32, 32, mode, 4, [base[j] for j in order])
        for r, j in enumerate(order):
            assert_same_tiles(got[r], first[j], 4, f"mode {mode} reordered: rung {r} is factor {base[j]}")


def test_null_pixels_give_the_same_values_and_sizes(gpu, product, small_batch):
    _, buf, geoms = small_batch
    for mode in (0, 1):
        g = geoms if mode == 0 else geoms[:3]
        full = ladder(gpu, product, buf, g, 4, 32, 32, mode, 4, FACTORS[mode])
        bare = ladder(gpu, product, buf, g, 4, 32, 32, mode, 4, FACTORS[mode], want_pixels=False)
        for r in range(len(full)):
            assert bare[r][3] is None
            assert_same_tiles(bare[r], full[r][:3] + (None,), 4, f"mode {mode} rung {r} without pixels")


# ---- 5. equal geometries ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("block", [32, 64])
def test_equal_images_equal_the_single_geometry_ladder(gpu, product, block):
    import torch
    N, H, W = 3, 200, 328
    frames = gpu.synth_frames_device(N, H, W, 4, dist=product.DIST_ALPHA)
    torch.cuda.synchronize()
    geoms = [(W, H, W * 4, k * W * H * 4) for k in range(N)]
    factors = FACTORS[0]
    got = ladder(gpu, product, frames.reshape(-1), geoms, 4, block, block, 0, 4, factors)
    vals, ow, oh, slots = host(gpu.shrink_ladder_frames_device(frames, block, block, 0, 4, factors))
    torch.cuda.synchronize()
    T = vals.shape[2]
    for r in range(len(factors)):
        exp = (vals[r].reshape(-1), ow[r].reshape(-1), oh[r].reshape(-1), slots[r].reshape(N * T, -1))
        assert_same_tiles(got[r], exp, 4, f"{block}x{block} rung {r} vs the single-geometry ladder")


# ---- 6. downstream calls take the layout ------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", [0, 1], ids=["shrink_by", "directional"])
def test_the_writer_takes_the_rungs_as_a_varied_batch(gpu, product, oracle, small_batch, mode):
    import torch
    images, buf, geoms = small_batch
    if mode == 1:
        images, geoms = images[:3], geoms[:3]
    factors = FACTORS[mode][:5]
    K, n = len(factors), len(images)
    T = int(product.varied_layout(geoms, 32, 32)[-1])
    out = poisoned((K, T), 32 * 32 * 4, buf.device)
    gpu.shrink_varied_ladder_frames_device(buf, 32, 32, mode, 4, factors, descs=geoms, channels=4, out=out)
    vals, ow, oh, slots = out
    sizes = [(g[0], g[1]) for g in geoms] * K
    foffs, fbuf = gpu.encode_varied_frames_device(sizes, 4, 32, 32, vals.reshape(-1), ow.reshape(-1), oh.reshape(-1), slots.reshape(K * T, -1))
    torch.cuda.synchronize()
    fo, data = foffs.cpu().numpy(), fbuf.cpu().numpy()
    for r, k in enumerate(factors):
        for i, img in enumerate(images):
            ev, ew, eh, es = oracle.shrink_image(img, 32, 32, mode, 4, k, nthreads=4)
            exp = oracle.encode_container(img.shape[1], img.shape[0], 32, 32, 4, 0, ev, None, ew, eh, es)
            assert data[fo[r * n + i]:fo[r * n + i + 1]].tobytes() == exp, f"mode {mode} factor {k} image {i}: file differs from the oracle's"


@pytest.mark.parametrize("mode,factors", [(1, [16.0, 64.0, 1.0]), (0, [0.5, 2.0, 0.03])], ids=["directional", "shrink_by"])
def test_rate_distortion_of_a_folder_equals_the_single_image_call_and_the_oracle(gpu, product, oracle, golden_dir, mode, factors):
    whole = np.ascontiguousarray(np.asarray(Image.open(os.path.join(golden_dir, "image.png")).convert("RGBA")))
    crop = np.ascontiguousarray(np.asarray(Image.open(os.path.join(golden_dir, "base.png")).convert("RGBA"))[:150, :200])
    images = [whole, crop] + ([np.array([[[9, 200, 31, 77]]], np.uint8)] if mode == 0 else [])  # (directional refuses 1 px tiles)
    block, down, up = 64, 4, 2
    file_bytes, sse = gpu.rate_distortion_varied_images(images, block, block, mode, down, up, factors)
    assert file_bytes.shape == (len(factors), len(images)) and sse.shape == (len(factors), len(images), 4)
    for i, img in enumerate(images):
        fb1, sse1 = gpu.rate_distortion_image(img, block, block, mode, down, up, factors)
        assert (file_bytes[:, i] == fb1).all() and (sse[:, i] == sse1).all(), f"image {i} vs rate_distortion_image"
        h, w, c = img.shape
        for r, k in enumerate(factors):
            ev, ew, eh, es = oracle.shrink_image(img, block, block, mode, down, k, nthreads=8)
            assert int(file_bytes[r, i]) == len(oracle.encode_container(w, h, block, block, c, 0, ev, None, ew, eh, es)), f"image {i} factor {k}"
            exp = expected_tiles(oracle, img, block, block, up, ew, eh, es).sum(axis=0)
            assert (sse[r, i].astype(np.int64) == exp).all(), f"image {i} factor {k}: squared error"


# ---- 7. handle state --------------------------------------------------------------------------------------------------------

def test_a_used_handle_gives_what_fresh_handles_give(gpu, product):
    import torch
    rng = np.random.default_rng(21)
    frames = gpu.synth_frames_device(2, 300, 520, 4, dist=product.DIST_ALPHA)
    torch.cuda.synchronize()
    imgs_a = [make_image(rng, w, h, 4, "partial") for (w, h) in [(100, 70), (33, 200), (9, 9), (150, 64)]]
    imgs_b = [make_image(rng, w, h, 4, "opaque") for (w, h) in [(130, 67), (64, 64), (200, 20)]]
    buf_a, geo_a = upload(imgs_a, 4, misalign=3)
    buf_b, geo_b = upload(imgs_b, 4, pad=16)
    fac = FACTORS[0]
    steps = [("single",), ("vladder", buf_a, geo_a, 32), ("single",), ("vladder", buf_b, geo_b, 64), ("ladder",), ("varied", buf_a, geo_a, 32),
             ("single",), ("trim",), ("vladder", buf_a, geo_a, 32), ("single",)]

    def run(h, step):
        """-> a list of host (values, w, h, slots) tuples"""
        if step[0] == "trim":
            h._check(h._L.pxz_trim(h._h))
            return []
        if step[0] == "single":
            vals, ow, oh, slots = host(h.shrink_frames_device(frames, 32, 32, 0, 4, 1.0))
            return [(vals.reshape(-1), ow.reshape(-1), oh.reshape(-1), slots.reshape(-1, slots.shape[-1]))]
        if step[0] == "ladder":
            vals, ow, oh, slots = host(h.shrink_ladder_frames_device(frames, 32, 32, 0, 4, fac))
            return [(vals.reshape(-1), ow.reshape(-1), oh.reshape(-1), slots.reshape(-1, slots.shape[-1]))]
        _, b, g, blk = step
        if step[0] == "varied":
            return [varied(gpu, product, b, g, 4, blk, blk, 0, 4, 0.25, h=h)]
        return ladder(gpu, product, b, g, 4, blk, blk, 0, 4, fac, h=h)

    shared = [run(gpu, s) for s in steps]
    for k, (s, got) in enumerate(zip(steps, shared)):
        if s[0] == "trim":
            continue
        fresh = product.Handle(0)
        try:
            exp = run(fresh, s)
        finally:
            fresh.close()
        assert len(got) == len(exp)
        for g, e in zip(got, exp):
            assert_same_tiles(g, e, 4, f"step {k} ({s[0]}) on a used handle vs a fresh one")


# ---- 8. errors --------------------------------------------------------------------------------------------------------------

def test_errors_write_nothing(gpu, product, small_batch):
    import torch
    _, buf, geoms = small_batch
    g3 = geoms[:3]
    T = int(product.varied_layout(g3, 16, 16)[-1])
    last_error = lambda: product.binding.load_library().pxz_last_error(gpu._h).decode()

    def refused(mode, g, factors, code, n_factors=None, rows=2):
        out = poisoned((rows, T), 16 * 16 * 4, buf.device)
        with pytest.raises(product.PxzError) as e:
            gpu.shrink_varied_ladder_frames_device(buf, 16, 16, mode, 4, factors, descs=g, channels=4, out=out, n_factors=n_factors)
        assert e.value.code == code, (e.value.code, last_error())
        torch.cuda.synchronize()
        assert still_poisoned(out), "an error case wrote its outputs"

    refused(0, g3, None, INVALID_ARG, n_factors=2)           # null factors
    refused(0, g3, [], INVALID_ARG)                          # none
    refused(0, g3, [1.0], INVALID_ARG, n_factors=0)
    refused(0, g3, [1.0] * 33, INVALID_ARG)                  # above the maximum
    refused(0, g3, [0.5, float("nan")], INVALID_ARG)
    refused(0, g3, [float("inf"), 0.5], INVALID_ARG)
    # a bad image in the middle of the batch is named
    refused(0, [g3[0], (g3[1][0], g3[1][1], 4, g3[1][3]), g3[2]], [1.0, 0.5], INVALID_ARG)   # pitch < row
    assert "image 1" in last_error()
    refused(0, [g3[0], (0, 10, 40, 0), g3[2]], [1.0, 0.5], INVALID_ARG)                      # empty image
    assert "image 1" in last_error()
    refused(0, [g3[0], g3[1], g3[2] + (1,)], [1.0, 0.5], INVALID_ARG)                        # reserved
    assert "image 2" in last_error()
    # 77 = 4 * 16 + 13 and 45 = 2 * 16 + 13 are fine; 1x1 and a 33 px wide image leave 1 px tiles
    refused(1, [g3[0], g3[2], geoms[3]], [16.0, 1.0], TILE_TOO_SMALL)
    assert "image 2" in last_error()
    refused(1, [g3[0], (33, 20, g3[0][2], g3[0][3]), g3[2]], [16.0, 1.0], TILE_TOO_SMALL)
    assert "image 1" in last_error()
