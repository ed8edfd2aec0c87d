"""The level decision at its exact breakpoints (operations.rs:145-151: value.log2().round().min(0.).exp2() per axis), on every
kernel path that makes it.  The product never computes a logarithm: it compares integer gradient sums or float bit patterns
against precomputed breakpoints, in about ten places, so a compare that is wrong only AT a breakpoint stores one tile at half
or double size and nothing else notices.  Here the tiles sit on the breakpoints:

  A  directional mode: tiles built so that their integer gradient sum is S - 1, S and S + 1 for every sum S at which the
     oracle's reduced size flips, per tile class (full, right edge, bottom edge, corner), on either axis;
  B  the same frames through the varied batch (float compares against the thresholds) and the factor ladder;
  C  Oklab mode: factors searched so that a noise tile's parsed value IS a threshold's bit pattern, its predecessor or its
     successor, for every level a block can reach, and on the ascending branch of negative factors;
  D  the tree's own test (value >= threshold) ^ is_positive (tree.rs:38-39,56) at thresholds equal to a tile's value.

Every comparison is bit for bit against the oracle on the same pixels (sizes, value bits, the valid slot bytes); there is no
tolerance anywhere.  The breakpoints come from the oracle alone, by bisection over reduce_dims -- never from the product.
All tile construction is CPU work, cached per module.

The kernels that keep a text of the compare of their own -- varied_ladder_kernel, reshrink_kernel, reshrink_ladder_kernel,
retile_kernel, retile_ladder_kernel -- meet the same tiles in tests/test_gpu_archive_breakpoints.py, through the builders of
this module (which imports without a GPU) and the archives of tests/test_archive_breakpoints_host.py."""
import numpy as np
import pytest

from test_gpu_parity import assert_same_tiles

pytestmark = pytest.mark.gpu

EDGE_W, EDGE_H = 13, 7          # ragged edges of every frame here (for 32: width 32 n + 13, height 32 m + 7)
NEAREST, LANCZOS3 = 0, 4
POOL_SEED = 20261019            # the Oklab pool: every (block, k, target) below is hit by one of its tiles (asserted)
_cache = {}


@pytest.fixture(scope="module")
def gpu(product):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    h = product.Handle(0)
    yield h
    h.close()


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def bits(v):
    return int(np.array([v], np.float32).view(np.uint32)[0])


def from_bits(b):
    return np.array([b], np.uint32).view(np.float32)[0]


def host_tiles(out, f):
    vals, ow, oh, slots = out
    return (vals[f].cpu().numpy(), ow[f].cpu().numpy().astype(np.uint32), oh[f].cpu().numpy().astype(np.uint32),
            None if slots is None else slots[f].cpu().numpy())


# ---- directional mode: breakpoints of the integer sum, and tiles with a prescribed sum ------------------------------------

def size_of_sum(oracle, s, w, h, factor, axis):
    """reduced size on `axis` of a (w, h) tile whose gradient sum on that axis is s: the detector's last step
    (operations.rs:253-258: f64 divide by (w-2)(h-2) 4096, to f32), the factor (pixlzr.rs:199), the oracle's reduce_dims"""
    raw = np.float32(np.float64(s) / np.float64((w - 2) * (h - 2) * 4096))
    v = np.float32(raw * np.float32(factor))
    return oracle.reduce_dims(v, v, w, h)[axis]


def flips(oracle, w, h, factor, axis):
    """every sum S with size(S - 1) != size(S), ascending (bisection over the whole range of the sum)"""
    def make():
        top = (w - 2) * (h - 2) * 3 * 1020
        out = []

        def split(lo, slo, hi, shi):
            if slo == shi:
                return
            if hi - lo == 1:
                out.append(hi)
                return
            mid = (lo + hi) // 2
            smid = size_of_sum(oracle, mid, w, h, factor, axis)
            split(lo, slo, mid, smid)
            split(mid, smid, hi, shi)
        split(0, size_of_sum(oracle, 0, w, h, factor, axis), top, size_of_sum(oracle, top, w, h, factor, axis))
        for s in out:
            assert size_of_sum(oracle, s - 1, w, h, factor, axis) != size_of_sum(oracle, s, w, h, factor, axis)
        return out
    return cached(("flips", w, h, factor, axis), make)


def build_tile(oracle, w, h, target):
    """(h, w, 3) tile whose sum_hz (the oracle's own out_sum_hz) is `target`.  Rows alternate in pairs between a and 0, so every
    3x3 window sees |row y+2 - row y| = a four times over: 4 (w-2)(h-2) a per channel.  The rest comes from the top row,
    which only the first band of windows reads: the whole row first (4 (w-2) a step), then single pixels (4, next to a
    corner 3, a corner exactly 1), each move kept only if the oracle's sum moves towards the target."""
    def make():
        area = (w - 2) * (h - 2)
        tot = min(target // (4 * area), 765)
        t = np.zeros((h, w, 3), np.uint8)
        t[(np.arange(h) // 2) % 2 == 0] = [tot // 3 + (1 if k < tot % 3 else 0) for k in range(3)]
        cur = oracle.lod_directional(t)[2]
        assert cur == 4 * area * tot
        moves = [(slice(0, w), 4 * (w - 2))]
        moves += [(slice(x, x + 1), 4) for x in range(2, w - 2)]
        moves += [(slice(x, x + 1), 3) for x in (1, w - 2)] + [(slice(x, x + 1), 1) for x in (0, w - 1)]
        for cols, weight in moves:
            for k in range(3):
                need = target - cur
                if need == 0:
                    return t
                if weight > abs(need):
                    break
                before = t[0, cols, k].copy()
                for sgn in (1, -1):
                    room = 255 - int(before.max()) if sgn > 0 else int(before.min())
                    if room < 1:
                        continue
                    t[0, cols, k] = before + sgn
                    e = oracle.lod_directional(t)[2] - cur
                    if e != 0 and (e > 0) == (need > 0) and abs(e) <= abs(need):
                        d = min(abs(need) // abs(e), room)
                        t[0, cols, k] = before + sgn * d
                        now = oracle.lod_directional(t)[2]
                        if now - cur != e * d:  # (a window changed sign on the way: keep the single step)
                            t[0, cols, k] = before + sgn
                            now = cur + e
                        cur = now
                        break
                    t[0, cols, k] = before
        assert cur == target, (w, h, target, cur)
        return t
    return cached(("tile", w, h, target), make)


def class_tiles(oracle, w, h, factor):
    """the tiles of one class: sum 0, the largest sum of the construction, and S - 1, S, S + 1 on either axis for every flip S
    of that axis -> [(tile, axis | None, sum)]"""
    top = (w - 2) * (h - 2) * 3 * 1020
    tiles = [(build_tile(oracle, w, h, 0), None, 0), (build_tile(oracle, w, h, top), 0, top)]
    for axis in (0, 1):
        for s in flips(oracle, w, h, factor, axis):
            for d in (-1, 0, 1):
                assert 0 <= s + d <= top
                if axis == 0:
                    t = build_tile(oracle, w, h, s + d)
                else:  # sum_vr of a tile is sum_hz of its transpose
                    t = np.ascontiguousarray(build_tile(oracle, h, w, s + d).transpose(1, 0, 2))
                tiles.append((t, axis, s + d))
    return tiles


def lay_out(oracle, bw, bh, factor, shapes):
    """images of n x m full tiles plus the ragged edge column, row and corner ((n, m) cycling through `shapes`), as many as it
    takes to place every tile of every class once; spare places repeat tiles.  Every placed tile's oracle sum is its target."""
    def make():
        sizes = [(bw, bh), (EDGE_W, bh), (bw, EDGE_H), (EDGE_W, EDGE_H)]
        queues = [class_tiles(oracle, w, h, factor) for (w, h) in sizes]
        pos = [0, 0, 0, 0]
        images = []
        while any(pos[c] < len(queues[c]) for c in range(4)):
            n, m = shapes[len(images) % len(shapes)]
            img = np.zeros((m * bh + EDGE_H, n * bw + EDGE_W, 3), np.uint8)
            for ty in range(m + 1):
                for tx in range(n + 1):
                    c = (1 if tx == n else 0) | (2 if ty == m else 0)
                    t, axis, s = queues[c][pos[c] % len(queues[c])]
                    pos[c] += 1
                    place = img[ty * bh:ty * bh + t.shape[0], tx * bw:tx * bw + t.shape[1]]
                    place[...] = t
                    assert place.shape[:2] == (sizes[c][1], sizes[c][0])
                    if axis is not None:
                        assert oracle.lod_directional(place)[2 + axis] == s
            images.append(img)
        return images
    return cached(("layout", bw, bh, factor, tuple(shapes)), make)


def with_form(img, form, bw, bh):
    """rgb: as built; rgba: opaque; alpha: one transparent pixel in every tile (the detector ignores alpha: the sums hold)"""
    if form == "rgb":
        return img
    out = np.concatenate([img, np.full(img.shape[:-1] + (1,), 255, np.uint8)], axis=-1)
    if form == "alpha":
        out[1::bh, 1::bw, 3] = 0
    return out


# the frames of A are built for the factor whose flips they sit on; the factors no sum can cross ride on the frames of 16
FRAME_FACTOR = {16.0: 16.0, -3.0: -3.0, 2.0: 2.0, 1e-3: 16.0, -1e-3: 16.0}


def frames_of(oracle, bw, bh, factor, form):
    return cached(("frames", bw, bh, factor, form),
                  lambda: np.stack([with_form(i, form, bw, bh) for i in lay_out(oracle, bw, bh, factor, [(2, 2)])]))


def expected(oracle, imgs_key, imgs, bw, bh, mode, filt, factor):
    return cached(("exp", imgs_key, bw, bh, mode, filt, factor),
                  lambda: [oracle.shrink_image(np.ascontiguousarray(i), bw, bh, mode, filt, factor, nthreads=8) for i in imgs])


def test_helper_finds_the_known_flips(oracle):
    """the bisection and the tile builder on numbers worked out by hand against the oracle"""
    assert flips(oracle, 32, 32, 16.0, 0) == [10183, 20365, 40730, 81459, 162918]
    assert flips(oracle, 32, 32, -3.0, 0) == [359908, 794354, 1011577, 1120189, 1174495]
    assert flips(oracle, 13, 32, 16.0, 0) == [7468, 14935, 29869, 59737]
    assert len(flips(oracle, 64, 64, 16.0, 0)) == 6 and flips(oracle, 64, 64, 16.0, 0)[0] == 21745
    assert [len(flips(oracle, *g, 0)) for g in ((16, 16, 4.0), (40, 12, 64.0), (24, 24, 1.0))] == [4, 6, 5]
    for s in (0, 1, 2, 3, 10182, 10183, 10184, 2754000):
        assert oracle.lod_directional(build_tile(oracle, 32, 32, s))[2] == s


def check_single(gpu, oracle, bw, bh, form, factors, filters):
    import torch
    hint = form == "alpha_hint"
    form = "alpha" if hint else form
    ch = 3 if form == "rgb" else 4
    for factor in factors:
        key = ("frames", bw, bh, FRAME_FACTOR[factor], form)
        imgs = frames_of(oracle, bw, bh, FRAME_FACTOR[factor], form)
        dev = torch.from_numpy(imgs).cuda()
        for filt in filters:
            got = gpu.shrink_frames_device(dev, bw, bh, 1, filt, factor, transparency_hint=hint)
            torch.cuda.synchronize()
            exp = expected(oracle, key, imgs, bw, bh, 1, filt, factor)
            for f in range(len(imgs)):
                assert_same_tiles(host_tiles(got, f), exp[f], ch, f"{bw}x{bh} {form} hint={hint} k={factor} filter {filt} frame {f}")
                if abs(factor) == 1e-3:  # every break is a sentinel: nothing but 1x1 tiles, or nothing but whole ones
                    ew, eh = exp[f][1], exp[f][2]
                    if factor > 0:
                        assert (ew == 1).all() and (eh == 1).all()
                    else:
                        n, m = imgs.shape[2] // bw, imgs.shape[1] // bh
                        assert (ew.reshape(m + 1, n + 1)[:, :n] == bw).all() and (ew.reshape(m + 1, n + 1)[:, n] == EDGE_W).all()
                        assert (eh.reshape(m + 1, n + 1)[:m] == bh).all() and (eh.reshape(m + 1, n + 1)[m] == EDGE_H).all()


@pytest.mark.parametrize("form", ["rgba", "rgb", "alpha", "alpha_hint"])
@pytest.mark.parametrize("bw,bh", [(32, 32), (16, 16), (64, 64), (24, 24), (40, 12)])
def test_directional_breakpoints(gpu, oracle, bw, bh, form):
    """A: shrink32_kernel / shrink32a_kernel, shrink16_kernel, shrink64_kernel and its alpha instance, shrink_kernel -- every
    class, every flip of either axis at S - 1, S, S + 1; descending (16, 2) and ascending (-3) breaks, and the sentinels"""
    check_single(gpu, oracle, bw, bh, form, (16.0, -3.0, 2.0, 1e-3, -1e-3), (NEAREST, LANCZOS3))


def test_directional_breakpoints_of_a_tile_beyond_lds(gpu, oracle):
    """A: the HBM-resident form of shrink_kernel, 192x192"""
    check_single(gpu, oracle, 192, 192, "rgba", (16.0,), (LANCZOS3,))


@pytest.mark.parametrize("block", [32, 24])
def test_directional_breakpoints_in_a_varied_batch(gpu, oracle, block):
    """B: varied_kernel compares the float values against the thresholds themselves.  The tiles of A in images of three
    different sizes, as many as it takes to hold every tile, in one call per factor.  This pins the detector's sums and the
    side of every threshold a sum's value falls on, but not `<` against `<=` in that compare: the value of a sum S is the
    first float past a threshold, hardly ever the threshold.  test_oklab_thresholds_in_a_varied_batch has values EQUAL to
    the thresholds."""
    import torch
    for factor in (16.0, -3.0, 2.0):
        shapes = [(2, 2), (3, 1), (1, 3)]
        imgs = [with_form(i, "rgba", block, block) for i in lay_out(oracle, block, block, factor, shapes)]
        assert len({i.shape for i in imgs}) == 3
        dev = [torch.from_numpy(i).cuda() for i in imgs]
        for filt in (NEAREST, LANCZOS3):
            offs, vals, ow, oh, slots = gpu.shrink_varied_frames_device(dev, block, block, 1, filt, factor)
            torch.cuda.synchronize()
            exp = expected(oracle, ("varied", block, factor), imgs, block, block, 1, filt, factor)
            for i in range(len(imgs)):
                a, b = int(offs[i]), int(offs[i + 1])
                got = (vals[a:b].cpu().numpy(), ow[a:b].cpu().numpy().astype(np.uint32), oh[a:b].cpu().numpy().astype(np.uint32),
                       slots[a:b].cpu().numpy())
                assert_same_tiles(got, exp[i], 4, f"varied {block} k={factor} filter {filt} image {i}")


@pytest.mark.parametrize("block", [32, 24])
def test_directional_breakpoints_on_the_ladder(gpu, oracle, block):
    """B: the frames of 16, -3 and 2 as one batch, the four factors as one ladder: every rung against the oracle and against
    the single call"""
    import torch
    factors = [16.0, -3.0, 2.0, 1e-3]
    imgs = np.concatenate([frames_of(oracle, block, block, f, "rgba") for f in (16.0, -3.0, 2.0)])
    dev = torch.from_numpy(imgs).cuda()
    lad = gpu.shrink_ladder_frames_device(dev, block, block, 1, LANCZOS3, factors)
    torch.cuda.synchronize()
    for r, factor in enumerate(factors):
        one = gpu.shrink_frames_device(dev, block, block, 1, LANCZOS3, factor)
        torch.cuda.synchronize()
        exp = expected(oracle, ("ladder", block), imgs, block, block, 1, LANCZOS3, factor)
        for f in range(len(imgs)):
            rung = tuple(x[r] for x in lad)
            assert_same_tiles(host_tiles(rung, f), exp[f], 4, f"ladder {block} rung {r} (k={factor}) frame {f} vs oracle")
            assert_same_tiles(host_tiles(rung, f), host_tiles(one, f), 4, f"ladder {block} rung {r} (k={factor}) frame {f} vs single")


# ---- Oklab mode: factors that put a tile's parsed value on a threshold's bit pattern ------------------------------------

def threshold_bits(oracle, k):
    """T_k = the smallest float the oracle's reduce_dims gives level 2^-k, read off the bit patterns around 2^(-k-1/2)"""
    def make():
        side = 1 << 30
        at = bits(np.float32(2.0 ** (-k - 0.5)))
        level = lambda b: oracle.reduce_dims(from_bits(b), from_bits(b), side, side)[0]
        hit = [b for b in range(at - 64, at + 64) if level(b) == side >> k and level(b - 1) == side >> (k + 1)]
        assert len(hit) == 1, (k, hit)
        return hit[0]
    return cached(("T", k), make)


def parsed(v):
    """parse_value (operations.rs:128-138) of a finite value"""
    return v if not np.signbit(v) else max(np.float32(np.float32(1.0) + v), np.float32(0.0))


def factor_onto(oracle, tile, target, negative):
    """a factor (negative: below zero, through parse_value's 1 + v) at which the oracle's parsed value of `tile` has the bit
    pattern `target`: the 128 floats around target / value(1), None if none of them lands on it"""
    goal = float(from_bits(target)) - (1.0 if negative else 0.0)
    start = bits(np.float32(goal / float(oracle.lod_oklab(tile, 1.0))))
    for d in range(-64, 64):
        f = from_bits(start + d)
        v = oracle.lod_oklab(tile, f)
        if bool(np.signbit(v)) == negative and bits(parsed(v)) == target:
            return float(f)
    return None


def attainable(target, negative):
    """whether the parsed value can have the bit pattern `target` at all: the value is fl(fl(x * factor) * 10) (pixlzr.rs:162),
    and ten times a float steps by 1.25 ulp of the product, so one pattern in five is never a product, whatever the tile and
    the factor; behind parse_value's 1 + v the ulp doubles from 0.5 down and every other pattern goes as well"""
    goal = float(from_bits(target)) - (1.0 if negative else 0.0)
    at = bits(np.float32(goal / 10.0))
    for b in range(at - 16, at + 17):
        v = np.float32(from_bits(b) * np.float32(10.0))
        if bool(np.signbit(v)) == negative and bits(parsed(v)) == target:
            return True
    return False


def nearest_attainable(threshold, d, negative):
    """T itself (d = 0), or the nearest pattern below (d = -1) / above (d = +1) it that a value can take -> (target, the
    patterns passed over on the way)"""
    target, skipped = threshold + d, []
    while not attainable(target, negative):
        assert d != 0 and abs(target - threshold) < 8, (hex(threshold), d, negative)
        skipped.append(target)
        target += d
    return target, skipped


def levels_of(block):
    return range(int(np.ceil(np.log2(block))))  # k = 0 .. : every level that still changes a side of `block`


def oklab_frame(block, ch):
    """3 x 3 full tiles of noise at several amplitudes (the pool) and the ragged edges, one of the pool's tiles with noise in
    its alpha"""
    def make():
        rng = np.random.default_rng(POOL_SEED + block)
        img = np.zeros((3 * block + EDGE_H, 3 * block + EDGE_W, 4), np.uint8)
        amps = [3, 8, 20, 48, 96, 128, 12, 64, 30]
        for ty in range(4):
            for tx in range(4):
                amp = amps[(3 * ty + tx) % 9]
                y0, x0 = ty * block, tx * block
                part = img[y0:y0 + block, x0:x0 + block]
                part[..., :3] = np.clip(128 + rng.integers(-amp, amp + 1, part.shape[:2] + (3,)), 0, 255)
                part[..., 3] = 255
        img[2 * block:3 * block, 2 * block:3 * block, 3] = rng.integers(0, 256, (block, block))
        return np.ascontiguousarray(img[..., :ch])
    return cached(("oklab frame", block, ch), make)


def pool_of(block, ch):
    img = oklab_frame(block, ch)
    return [img[ty * block:(ty + 1) * block, tx * block:(tx + 1) * block] for ty in range(3) for tx in range(3)]


def oracle_never_reaches(oracle, pattern, negative):
    """attainable() is this file's own arithmetic; a pattern it rules out must be one the oracle does not reach either.  Which
    patterns are products of ten does not depend on the tile, so each is searched once, on the 18 tiles of the 16-px pools
    (RGBA and RGB), whichever block size asks"""
    return cached(("never", pattern, negative),
                  lambda: all(factor_onto(oracle, t, pattern, negative) is None for ch in (4, 3) for t in pool_of(16, ch)))


def oklab_factors(oracle, block, ch):
    """{(k, d, negative): factor}: some full tile of the frame has, at that factor, a parsed value of exactly T_k (d = 0), of its
    predecessor (d = -1) or its successor (d = +1) among the patterns a value can take at all (nearest_attainable; the oracle
    reaches no pattern passed over: oracle_never_reaches); every target is hit (positive factors at every level of the block, negative ones at k = 0, 1)"""
    def make():
        pool = pool_of(block, ch)
        out = {}
        for negative in (False, True):
            for k in (levels_of(block) if not negative else (0, 1)):
                for d in (-1, 0, 1):
                    target, skipped = nearest_attainable(threshold_bits(oracle, k), d, negative)
                    for b in skipped:
                        assert oracle_never_reaches(oracle, b, negative), (block, ch, k, d, negative, hex(b))
                    hits = (factor_onto(oracle, t, target, negative) for t in pool)
                    f = next((f for f in hits if f is not None), None)
                    assert f is not None, f"no tile of the pool reaches T_{k}{d:+d} (block {block}, {ch} channels, negative {negative})"
                    out[(k, d, negative)] = f
        return out
    return cached(("oklab factors", block, ch), make)


@pytest.mark.parametrize("ch", [4, 3])
@pytest.mark.parametrize("block", [16, 32, 64, 24])
def test_oklab_thresholds_to_the_bit(gpu, oracle, block, ch):
    """C: one call per factor, the whole frame against the oracle.  k = 0 is the "stored at full size" decision that the
    copies-ahead skip and clone_split64_kernel rest on: those calls run again into slots filled with a sentinel byte, where a
    wrongly skipped tile shows."""
    import torch
    img = oklab_frame(block, ch)
    dev = torch.from_numpy(img[None]).cuda()
    for (k, d, negative), factor in oklab_factors(oracle, block, ch).items():
        exp = expected(oracle, ("oklab", block, ch), [img], block, block, 0, LANCZOS3, factor)[0]
        what = f"oklab {block} c{ch} T_{k}{d:+d} negative={negative} k={factor!r}"
        got = gpu.shrink_frames_device(dev, block, block, 0, LANCZOS3, factor)
        torch.cuda.synchronize()
        assert_same_tiles(host_tiles(got, 0), exp, ch, what)
        if k == 0:
            for x in got[:3]:
                x.fill_(0x5A5A5A5A if x.dtype == torch.int32 else 0)
            got[3].fill_(0xA5)
            got = gpu.shrink_frames_device(dev, block, block, 0, LANCZOS3, factor, out=got)
            torch.cuda.synchronize()
            assert_same_tiles(host_tiles(got, 0), exp, ch, what + " into sentinel slots")


@pytest.mark.parametrize("ch", [4, 3])
def test_oklab_thresholds_on_the_ladder(gpu, oracle, ch):
    """C: ladder_level.  The 15 positive factors of the 32x32 frame and a negative one as one 16-rung call: every rung against
    the oracle and against its single call"""
    import torch
    block = 32
    found = oklab_factors(oracle, block, ch)
    factors = [f for (k, d, negative), f in found.items() if not negative] + [found[(0, 0, True)]]
    assert len(factors) == 16
    img = oklab_frame(block, ch)
    dev = torch.from_numpy(img[None]).cuda()
    lad = gpu.shrink_ladder_frames_device(dev, block, block, 0, LANCZOS3, factors)
    torch.cuda.synchronize()
    for r, factor in enumerate(factors):
        exp = expected(oracle, ("oklab", block, ch), [img], block, block, 0, LANCZOS3, factor)[0]
        one = gpu.shrink_frames_device(dev, block, block, 0, LANCZOS3, factor)
        torch.cuda.synchronize()
        rung = tuple(x[r] for x in lad)
        assert_same_tiles(host_tiles(rung, 0), exp, ch, f"oklab ladder c{ch} rung {r} (k={factor!r}) vs oracle")
        assert_same_tiles(host_tiles(rung, 0), host_tiles(one, 0), ch, f"oklab ladder c{ch} rung {r} (k={factor!r}) vs single")


@pytest.mark.parametrize("ch", [4, 3])
@pytest.mark.parametrize("block", [32, 24])
def test_oklab_thresholds_in_a_varied_batch(gpu, oracle, block, ch):
    """C through varied_kernel, whose float compare meets a value EQUAL to a threshold only here (a gradient sum's value is the
    first float past a threshold, hardly the threshold): the frame and two smaller cuts of it as one batch, one call per factor"""
    import torch
    frame = oklab_frame(block, ch)
    imgs = [frame, np.ascontiguousarray(frame[:2 * block + 5, :3 * block]), np.ascontiguousarray(frame[:block, :2 * block + 3])]
    dev = [torch.from_numpy(i).cuda() for i in imgs]
    for (k, d, negative), factor in oklab_factors(oracle, block, ch).items():
        offs, vals, ow, oh, slots = gpu.shrink_varied_frames_device(dev, block, block, 0, LANCZOS3, factor)
        torch.cuda.synchronize()
        exp = expected(oracle, ("oklab varied", block, ch), imgs, block, block, 0, LANCZOS3, factor)
        for i in range(len(imgs)):
            a, b = int(offs[i]), int(offs[i + 1])
            got = (vals[a:b].cpu().numpy(), ow[a:b].cpu().numpy().astype(np.uint32), oh[a:b].cpu().numpy().astype(np.uint32),
                   slots[a:b].cpu().numpy())
            assert_same_tiles(got, exp[i], ch, f"oklab varied {block} c{ch} T_{k}{d:+d} negative={negative} k={factor!r} image {i}")


# ---- the tree's own threshold -------------------------------------------------------------------------------------------

TREE_W, TREE_H = 136, 200


def tree_frame(ch=4):
    def make():
        rng = np.random.default_rng(POOL_SEED)
        yy, xx = np.mgrid[0:TREE_H, 0:TREE_W]
        amp = 4 + 6 * ((xx // 25 + 2 * (yy // 25)) % 7)  # busier and calmer patches, so the recursion has something to decide
        img = np.clip(128 + rng.integers(-64, 65, (TREE_H, TREE_W, 4)) * amp[..., None] // 40, 0, 255).astype(np.uint8)
        img[..., 3] = 255
        return np.ascontiguousarray(img[..., :ch])
    return cached(("tree frame", ch), make)


def tree_value_bits(oracle, bw, bh, ch, t):
    """the value of outermost tile t, as bits: with a negative threshold the tile is pixelised while value >= |threshold|
    (tree.rs:38-39,56), so the value is the largest |threshold| at which it still is -- bisected over the float's bits on the
    oracle's output, where "pixelised" reads: the tile's pixels equal those of a run that pixelises every outermost tile"""
    def make():
        img = tree_frame(ch)
        x0, y0, w, h = oracle.tile_rect(TREE_W, TREE_H, bw, bh, t)
        part = lambda thr: oracle.tree_process_image(img, bw, bh, thr)[y0:y0 + h, x0:x0 + w]
        whole = part(-1e-30)  # value >= 1e-30 everywhere: every outermost tile is pixelised
        lo, hi = bits(np.float32(1e-6)), bits(np.float32(10.0))
        assert (part(-from_bits(lo)) == whole).all() and not (part(-from_bits(hi)) == whole).all()
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if (part(-from_bits(mid)) == whole).all():
                lo = mid
            else:
                hi = mid
        return lo
    return cached(("tree value", bw, bh, ch, t), make)


@pytest.mark.parametrize("ch", [4, 3])
@pytest.mark.parametrize("bw,bh,tiles", [(64, 64, (0, 5, 10)), (50, 50, (0, 6, 11))])
def test_tree_threshold_equal_to_a_tiles_value(gpu, oracle, bw, bh, tiles, ch):
    """D: per-level grids (64x64) and rectangle lists (50x50) at thresholds that ARE the value of an outermost tile, the floats
    next to it, their negatives, and both zeros (-0.0 >= 0.0 is true: tree.rs:38)"""
    import torch
    img = tree_frame(ch)
    cols, rows = oracle.grid(TREE_W, TREE_H, bw, bh)
    thresholds = [0.0, -0.0]
    assert (cols, rows) == (3, 4)
    for t in tiles:  # a full tile and two of the ragged edges (64: 8x64 and 64x8, 50: a full one more and 36x50)
        b = tree_value_bits(oracle, bw, bh, ch, t)
        at = [oracle.tree_process_image(img, bw, bh, -from_bits(x)) for x in (b, b + 1)]
        assert not (at[0] == at[1]).all()
        thresholds += [s * from_bits(x) for x in (b - 1, b, b + 1) for s in (1, -1)]
    dev = torch.from_numpy(img[None]).cuda()
    for thr in thresholds:
        got = gpu.tree_process_frames_device(dev, bw, bh, float(thr)).cpu().numpy()[0]
        exp = oracle.tree_process_image(img, bw, bh, float(thr))
        bad = (got != exp).any(axis=-1)
        assert not bad.any(), f"tree {bw}x{bh} c{ch} threshold {thr!r} ({bits(thr):08x}): {int(bad.sum())} pixels differ"
