"""The directional detector of the 32x32 kernels on pixel quads (sobel32_quads), against the oracle -- value bits, sizes and every
stored byte of every tile.

A lane owns a quad of columns (4j..4j+3) as two pixel pairs; eight groups of eight lanes own four window rows each (the group at
row 28 two), and read two rows beyond them.  Pair B of a quad takes the next quad's first pair from the lane to its right, which
for quad 7 is another group's lane.  What can go wrong there: a window counted twice or not at all at a seam between groups
(rows 3|4, 7|8, ...) or between quads (columns 3|4, ...), the tail group counting rows 32 and 33 (the next plane, or whatever
lies behind the third), quad 7's pair B leaking in, a channel left out, a u16 half that overflows.  Every input below is made so
that one of these changes a detector sum, and with it the stored value bits."""
import numpy as np
import pytest

LANCZOS3, NEAREST = 4, 0
DIRECTIONAL, FACTOR = 1, 16.0  # the benchmark's caller and factor
FILTERS = {"lanczos3": LANCZOS3, "nearest": NEAREST}


@pytest.fixture(scope="module")
def gpu(product):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    h = product.Handle(0)
    yield h
    h.close()


def sizes_of(exp):
    return {(int(w), int(h)) for w, h in zip(exp[1].tolist(), exp[2].tolist())}


def assert_same_tiles(got, exp, what):
    gv, gw, gh, gs = got
    ev, ew, eh, es = exp
    c = es.shape[1] // 1024
    assert gv.shape == ev.shape and gs.shape == es.shape, what
    assert (gw == ew).all() and (gh == eh).all(), f"{what}: sizes differ on tiles {np.nonzero((gw != ew) | (gh != eh))[0][:8].tolist()}"
    gb, eb = gv.view(np.uint32), ev.view(np.uint32)
    assert (gb == eb).all(), f"{what}: value bits differ on tiles {np.nonzero(gb != eb)[0][:8].tolist()}"
    valid = np.arange(es.shape[1])[None, :] < (ew.astype(np.int64) * eh * c)[:, None]
    diff = (gs != es) & valid
    assert not diff.any(), f"{what}: {int(diff.sum())} stored bytes differ in tiles {np.nonzero(diff.any(axis=1))[0][:8].tolist()}"


def put(img, k, cols, tile):
    ty, tx = divmod(k, cols)
    img[ty * 32:ty * 32 + 32, tx * 32:tx * 32 + 32, :tile.shape[2]] = tile


# ---- 1. impulse sweep -------------------------------------------------------------------------------------------------------

def impulse_frame(inverted):
    """96 x 32 tiles, opaque: tile k is 0 (inverted: 255) but for ONE sample of 255 (0) at pixel (k % 32, (k // 32) % 32) of channel
    k // 1024 -- every pixel position of every channel, so every lane, pair, group seam, quad seam and the masked pair of quad 7"""
    lo, hi = (255, 0) if inverted else (0, 255)
    img = np.full((1024, 3072, 4), lo, np.uint8)
    img[..., 3] = 255
    k = np.arange(3072)
    img[(k // 96) * 32 + (k // 32) % 32, (k % 96) * 32 + k % 32, k // 1024] = hi
    return img


@pytest.fixture(scope="module")
def impulses(oracle):
    out = {}
    for inverted in (False, True):
        img = impulse_frame(inverted)
        out[inverted] = img, {f: oracle.shrink_image(img, 32, 32, DIRECTIONAL, f, FACTOR, nthreads=8) for f in FILTERS.values()}
    return out


def test_impulse_frames_are_what_they_claim(impulses):
    """This file's own input (no GPU): one sample per tile differs, and it visits all 3 x 1024 (channel, y, x) positions once."""
    for inverted, (img, _) in impulses.items():
        lo = 255 if inverted else 0
        tiles = img.reshape(32, 32, 96, 32, 4).transpose(0, 2, 1, 3, 4).reshape(3072, 32, 32, 4)
        assert (tiles[..., 3] == 255).all()
        odd = tiles[..., :3] != lo
        assert (odd.reshape(3072, -1).sum(axis=1) == 1).all()
        where = np.argwhere(odd)  # (tile, y, x, channel)
        assert len({(int(c), int(y), int(x)) for _, y, x, c in where}) == 3072
        assert (where[:, 3] == where[:, 0] // 1024).all() and (where[:, 2] == where[:, 0] % 32).all()
        assert (where[:, 1] == (where[:, 0] // 32) % 32).all()


@pytest.mark.gpu
@pytest.mark.parametrize("inverted", [False, True], ids=["one-255", "one-0"])
@pytest.mark.parametrize("filt", list(FILTERS), ids=list(FILTERS))
def test_impulse_sweep(gpu, impulses, filt, inverted):
    img, exp = impulses[inverted]
    got = gpu.shrink_image(img, 32, 32, DIRECTIONAL, FILTERS[filt], FACTOR)
    assert_same_tiles(got, exp[FILTERS[filt]], f"impulse sweep, {filt}, inverted={inverted}")


# ---- 2. leaks across groups and past row 31 -----------------------------------------------------------------------------------

def rim_frame(seed):
    """4 x 2 tiles.  Even tiles: columns 0..3 and 28..31 and rows 0..1 and 30..31 carry independent noise per channel, the interior is
    constant; odd tiles the reverse.  What quad 7's neighbour lane or rows 32, 33 would add is noise of another lane's."""
    rng = np.random.default_rng(seed)
    img = np.empty((64, 128, 4), np.uint8)
    img[..., 3] = 255
    rim = np.ones((32, 32), bool)
    rim[2:30, 4:28] = False
    for k in range(8):
        noise = rng.integers(0, 256, (32, 32, 3), dtype=np.uint8)
        flat = np.broadcast_to(rng.integers(0, 256, 3, dtype=np.uint8), (32, 32, 3))
        noisy = rim if k % 2 == 0 else ~rim
        put(img, k, 4, np.where(noisy[..., None], noise, flat))
    return img


@pytest.mark.gpu
def test_rims_and_a_second_run_over_other_lds_bytes(gpu, oracle):
    img = rim_frame(11)
    between = np.random.default_rng(12).integers(0, 256, img.shape, dtype=np.uint8)
    between[..., 3] = 255
    exp = oracle.shrink_image(img, 32, 32, DIRECTIONAL, LANCZOS3, FACTOR)
    exp_between = oracle.shrink_image(between, 32, 32, DIRECTIONAL, LANCZOS3, FACTOR)
    assert_same_tiles(gpu.shrink_image(img, 32, 32, DIRECTIONAL, LANCZOS3, FACTOR), exp, "rims, first run")
    assert_same_tiles(gpu.shrink_image(between, 32, 32, DIRECTIONAL, LANCZOS3, FACTOR), exp_between, "noise in between")
    assert_same_tiles(gpu.shrink_image(img, 32, 32, DIRECTIONAL, LANCZOS3, FACTOR), exp, "rims, second run")


# ---- 3. dense tiles -----------------------------------------------------------------------------------------------------------

KINDS = ("constant", "vertical-edge", "horizontal-edge", "noise", "soft", "columns", "checker-1", "checker-2")


def tile_of_kind(kind, rng):
    """one 32x32 tile of three colour channels that never share a value stream (the checkerboards: a phase per channel)"""
    t = np.empty((32, 32, 3), np.uint8)
    if kind == "constant":
        t[...] = rng.integers(0, 256, 3, dtype=np.uint8)
    elif kind == "vertical-edge":
        t[:, :13] = rng.integers(0, 256, 3, dtype=np.uint8)
        t[:, 13:] = rng.integers(0, 256, 3, dtype=np.uint8)
    elif kind == "horizontal-edge":
        t[:21] = rng.integers(0, 256, 3, dtype=np.uint8)
        t[21:] = rng.integers(0, 256, 3, dtype=np.uint8)
    elif kind == "noise":
        t[...] = rng.integers(0, 256, (32, 32, 3), dtype=np.uint8)
    elif kind == "soft":
        t[...] = rng.integers(30, 190, 3)[None, None, :] + rng.integers(0, int(rng.choice([28, 56])), (32, 32, 3))
    elif kind == "columns":
        t[...] = np.clip(rng.integers(0, 256, (1, 32, 3)) + rng.integers(0, 4, (32, 1, 3)), 0, 255)
    else:  # full swing per pixel / per 2 px: the largest sums the u16 halves and the accumulators see
        step = 1 if kind == "checker-1" else 2
        y, x = np.mgrid[0:32, 0:32] // step
        phase = rng.integers(0, 2, 3)
        t[...] = (((y + x)[..., None] + phase[None, None, :]) % 2 * 255).astype(np.uint8)
    return t


def dense_frame(kind, channels):
    rng = np.random.default_rng(1000 + KINDS.index(kind))
    img = np.full((96, 128, channels), 255, np.uint8)
    for k in range(12):
        put(img, k, 4, tile_of_kind(kind, rng))
    return img


@pytest.fixture(scope="module")
def dense(oracle):
    out = {}
    for kind in KINDS:
        for c in (4, 3):
            img = dense_frame(kind, c)
            out[kind, c] = img, oracle.shrink_image(img, 32, 32, DIRECTIONAL, LANCZOS3, FACTOR)
    return out


def test_the_inputs_span_size_classes(impulses, dense):
    """The oracle alone (no GPU): over the inputs of parts 1 and 3 at least three size classes occur, so equal sizes say something."""
    one = set().union(*(sizes_of(e) for _, exp in impulses.values() for e in exp.values()))
    three = set().union(*(sizes_of(exp) for _, exp in dense.values()))
    assert len(one | three) >= 3, (one, three)
    assert (32, 32) in three and len(three) >= 3, three


@pytest.mark.gpu
@pytest.mark.parametrize("channels", [4, 3], ids=["rgba", "rgb"])
@pytest.mark.parametrize("kind", KINDS)
def test_dense_tiles(gpu, dense, kind, channels):
    img, exp = dense[kind, channels]
    got = gpu.shrink_image(img, 32, 32, DIRECTIONAL, LANCZOS3, FACTOR)
    assert_same_tiles(got, exp, f"4x3 tiles of {kind}, {channels} channels")


# ---- 4. a ragged frame, and tiles with transparency ----------------------------------------------------------------------------

@pytest.mark.gpu
def test_ragged_frame(gpu, oracle):
    """100 x 70: 3 x 2 full tiles beside a ragged column and row, which the worklist path finishes from sums of its own"""
    rng = np.random.default_rng(70)
    img = np.full((96, 128, 4), 255, np.uint8)
    for k in range(12):
        put(img, k, 4, tile_of_kind(KINDS[k % 6], rng))
    img = np.ascontiguousarray(img[:70, :100])
    exp = oracle.shrink_image(img, 32, 32, DIRECTIONAL, LANCZOS3, FACTOR)
    assert len(sizes_of(exp)) >= 3
    assert_same_tiles(gpu.shrink_image(img, 32, 32, DIRECTIONAL, LANCZOS3, FACTOR), exp, "100x70")


@pytest.mark.gpu
def test_mostly_transparent_frame_through_the_four_plane_kernel(product, oracle):
    """64 x 64, alpha below 255 nearly everywhere, announced as transparent: shrink32a_kernel's detector is the same helper, its
    fourth plane (rows 32, 33 of the third) holds alpha bytes that no sum may see"""
    import torch
    rng = np.random.default_rng(64)
    img = np.empty((64, 64, 4), np.uint8)
    for k, kind in enumerate(("noise", "soft", "vertical-edge", "soft")):
        put(img, k, 2, tile_of_kind(kind, rng))
    img[..., 3] = rng.integers(0, 256, (64, 64), dtype=np.uint8)
    img[::7, ::5, 3] = 255
    exp = oracle.shrink_image(img, 32, 32, DIRECTIONAL, LANCZOS3, FACTOR)
    h = product.Handle(0)
    try:
        vals, ow, oh, slots = h.shrink_frames_device(torch.from_numpy(img[None]).cuda(), 32, 32, DIRECTIONAL, LANCZOS3, FACTOR,
                                                     transparency_hint=True)
        torch.cuda.synchronize()
        assert h.state()["alpha_kernel"], h.state()
        got = (vals[0].cpu().numpy(), ow[0].cpu().numpy().astype(np.uint32), oh[0].cpu().numpy().astype(np.uint32), slots[0].cpu().numpy())
        assert_same_tiles(got, exp, "64x64 with transparency")
    finally:
        h.close()
