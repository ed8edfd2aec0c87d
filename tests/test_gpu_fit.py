"""Fit to a budget on the device (pxz_fit_varied_ladder_device, pxz_gather_varied_rungs_device, pxz_encode_varied_images_fit):
the device's choice equals pxz_fit_select on the same table, the gathered batch equals slices of the ladder's rungs -- value
bits, sizes, the valid slot bytes, and not a byte behind them -- and the host form's files equal, byte for byte,
pxz_encode_varied_images of each image alone at its chosen factor and the oracle.  Every output is poisoned before each call,
with a guard behind it that must stay untouched."""
import ctypes as C

import numpy as np
import pytest

from test_fit_host import FIT_BYTES, FIT_SSE, U64, check_table, directed_tables, random_tables, select
from test_gpu_parity import assert_same_tiles
from test_gpu_varied import make_image, upload
from test_gpu_varied_ladder import FACTORS, POISON, host, poisoned, tile_geometry

pytestmark = pytest.mark.gpu

INVALID_ARG, UNSUPPORTED, BUFFER_TOO_SMALL = -1, -5, -7
POISON32 = 0x5A5A5A5A
# The gather's outputs are poisoned with other bytes than its inputs.  The ladder leaves POISON (0xA5) behind the valid bytes of
# its slots, which are the gather's source: with the same byte in the outputs, a copy that ran on behind the valid bytes would
# write 0xA5 onto 0xA5 and go unseen.
OUT_POISON, OUT_POISON_VAL, OUT_POISON_DIM = 0x3C, 0x3C3C3C3C, 0x69696969


def out_poisoned(shape, slot, want_pixels=True):
    import torch
    vals = torch.full(shape, OUT_POISON_VAL, dtype=torch.int32, device="cuda").view(torch.float32)
    ow = torch.full(shape, OUT_POISON_DIM, dtype=torch.int32, device="cuda")
    oh = torch.full(shape, OUT_POISON_DIM, dtype=torch.int32, device="cuda")
    slots = torch.full(shape + (slot,), OUT_POISON, dtype=torch.uint8, device="cuda") if want_pixels else None
    return vals, ow, oh, slots


def out_still_poisoned(out):
    import torch
    vals, ow, oh, slots = out
    return bool((vals.view(torch.int32) == OUT_POISON_VAL).all() and (ow == OUT_POISON_DIM).all() and (oh == OUT_POISON_DIM).all() and
                (slots is None or (slots == OUT_POISON).all()))


@pytest.fixture(scope="module")
def gpu(product):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    h = product.Handle(0)
    yield h
    h.close()


def last_error(gpu):
    return (gpu._L.pxz_last_error(gpu._h) or b"").decode()


def to_device_u64(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64)).cuda()


# ---- 1. select --------------------------------------------------------------------------------------------------------------

def device_select(gpu, t, guard=3):
    """one table uploaded as the writer's offsets and the distortion call's sums -> host (choice, flags), guard checked"""
    import torch
    fb, ss = t["file_bytes"], t["sse"]
    K, n = fb.shape
    offs = np.concatenate([np.zeros(1, np.uint64), np.cumsum(fb.reshape(-1), dtype=np.uint64)])  # (wraps mod 2^64: so do the differences)
    d_offs, d_sse = to_device_u64(offs), to_device_u64(ss)
    choice = torch.full((n + guard,), POISON32, dtype=torch.int32, device="cuda")
    flags = torch.full((n + guard,), POISON32, dtype=torch.int32, device="cuda")
    gpu.fit_varied_ladder_device(d_offs, d_sse, t["criterion"], t["targets"], out=(choice[:n], flags[:n]))
    torch.cuda.synchronize()
    assert (choice[n:] == POISON32).all() and (flags[n:] == POISON32).all(), (t["name"], "the guard behind an output was written")
    return choice[:n].cpu().numpy().astype(np.uint32), flags[:n].cpu().numpy().astype(np.uint32)


def test_the_device_selects_what_the_host_selects(gpu, product):
    for t in directed_tables() + random_tables():
        choice, flags = device_select(gpu, t)
        h_choice, h_flags = product.fit_select(t["file_bytes"], t["sse"], t["criterion"], t["targets"])
        assert (choice == h_choice).all() and (flags == h_flags).all(), t["name"]
        check_table(t, choice, flags)


# ---- 2. gather against slices -------------------------------------------------------------------------------------------------

GATHER_CASES = [(32, 32, 4, [(100, 70), (20, 9), (77, 45), (66, 35), (131, 40)]),
                (16, 16, 4, [(50, 34), (9, 5), (83, 61), (35, 20)]),
                (48, 20, 3, [(100, 38), (30, 11), (150, 63), (52, 45)]),
                (37, 61, 3, [(100, 70), (20, 40), (113, 125), (76, 64)]),
                (5, 3, 3, [(23, 11), (7, 5), (4, 2), (18, 14)])]  # 45-byte slots: every alignment of source against destination
K = 8


@pytest.fixture(scope="module", params=[(case, mode) for case in GATHER_CASES for mode in (0, 1)],
                ids=lambda p: f"{p[0][0]}x{p[0][1]}-c{p[0][2]}-{'by' if p[1] == 0 else 'dir'}")
def rungs(request, gpu, product):
    """the rung-major result of one varied ladder (device tensors, and on the host), with its geometry"""
    import torch
    (bw, bh, c, sizes), mode = request.param
    rng = np.random.default_rng(bw * 100 + bh + mode)
    if bw * bh < 64:  # (make_image's smooth areas are wider than these images: plain noise)
        images = [rng.integers(0, 256, (h, w, c), dtype=np.uint8) for (w, h) in sizes]
    else:
        images = [make_image(rng, w, h, c, ["partial", "opaque", "clear"][k % 3]) for k, (w, h) in enumerate(sizes)]
    buf, geoms = upload(images, c, pad=3, misalign=5)
    T = int(product.varied_layout(geoms, bw, bh)[-1])
    out = poisoned((K, T), bw * bh * c, buf.device)
    gpu.shrink_varied_ladder_frames_device(buf, bw, bh, mode, 2, FACTORS[mode], descs=geoms, channels=c, out=out)
    torch.cuda.synchronize()
    fw, fh, owner, _ = tile_geometry(geoms, bw, bh)
    assert (fw < bw).any() and (fh < bh).any() and any(w < bw and h < bh for (w, h) in sizes)  # ragged edges, an image below a block
    return dict(bw=bw, bh=bh, c=c, sizes=sizes, T=T, owner=owner, dev=out, host=host(out))


def gather(gpu, r, choice, want_pixels=True, flags=False, guard=3):
    """one gather into poisoned outputs with a guard image's worth of tiles behind them -> host (values, w, h, slots), flags"""
    import torch
    T, slot = r["T"], r["bw"] * r["bh"] * r["c"]
    full = out_poisoned((T + guard,), slot, want_pixels)
    out = tuple(None if x is None else x[:T] for x in full)
    d_choice = torch.from_numpy(np.array(choice, np.uint32).view(np.int32)).cuda()
    n = len(r["sizes"])
    d_flags = torch.full((n + 1,), POISON32, dtype=torch.int32, device="cuda") if flags else None
    vals, ow, oh, slots = r["dev"]
    gpu.gather_varied_rungs_device(r["sizes"], r["c"], r["bw"], r["bh"], K, d_choice, vals, ow, oh, slots, out=out,
                                   image_flags=None if d_flags is None else d_flags[:n])
    torch.cuda.synchronize()
    assert out_still_poisoned(tuple(None if x is None else x[T:] for x in full)), "the guard behind the outputs was written"
    got_flags = None
    if flags:
        assert int(d_flags[n]) == POISON32, "the guard behind the flags was written"
        got_flags = d_flags[:n].cpu().numpy()
    return host(out), got_flags


def check_gather(r, got, rung_of_image):
    """every output tile against the slice of its image's rung; the slot behind the valid bytes still poisoned"""
    vals, ow, oh, slots = r["host"]
    pick = np.array(rung_of_image)[r["owner"]]
    t = np.arange(r["T"])
    gv, gw, gh, gs = got
    assert (gv.view(np.uint32) == vals[pick, t].view(np.uint32)).all(), "value bits"
    assert (gw == ow[pick, t]).all() and (gh == oh[pick, t]).all(), "sizes"
    if gs is not None:
        valid = np.arange(gs.shape[1])[None, :] < (gw.astype(np.int64) * gh * r["c"])[:, None]
        assert (gs[valid] == slots[pick, t][valid]).all(), "valid bytes"
        assert (gs[~valid] == OUT_POISON).all(), "a byte behind the valid ones was written"
        assert valid.any() and (~valid).any()
        # (the source holds another byte there, so a copy that ran on would show)
        assert (slots[pick, t][~valid] == POISON).all() and POISON != OUT_POISON


def test_gather_equals_slices_of_the_rungs(gpu, rungs):
    n = len(rungs["sizes"])
    mixed = [(3 * i + 1) % K for i in range(n)]
    assert len(set(mixed)) == n
    for choice in ([0] * n, [K - 1] * n, mixed):
        got, _ = gather(gpu, rungs, choice)
        check_gather(rungs, got, choice)
    # the rungs differ where it matters: the mixed gather is not the gather of one rung
    ow = rungs["host"][1]
    assert (ow[0] != ow[K - 1]).any() or (rungs["host"][2][0] != rungs["host"][2][K - 1]).any()
    # values and sizes only
    got, _ = gather(gpu, rungs, mixed, want_pixels=False)
    assert got[3] is None
    check_gather(rungs, got, mixed)


def test_a_choice_beyond_the_ladder_reads_the_last_rung_and_is_flagged(gpu, rungs):
    n = len(rungs["sizes"])
    choice = [K, 2 ** 32 - 1] + [(3 * i + 1) % K for i in range(2, n)]
    got, flags = gather(gpu, rungs, choice, flags=True)
    check_gather(rungs, got, [K - 1, K - 1] + choice[2:])
    assert flags.tolist() == [2, 2] + [0] * (n - 2)


# ---- 3. gather across 4 GiB ---------------------------------------------------------------------------------------------------

def test_gather_addresses_slots_beyond_4_gib(gpu, product):
    """128x128 RGBA slots are 2^16 bytes, so slot 2^16 starts at byte 2^32: with 32 rungs of 2116 tiles, every slot of rung 31
    lies beyond it.  A 32-bit slot offset would read slot (index mod 2^16) instead -- those hold other bytes."""
    import torch
    bw = bh = 128
    rungs_n, slot, small = 32, 128 * 128 * 4, 8 * 8 * 4
    sizes = [(40 * bw, 30 * bh), (30 * bw, 30 * bh), (bw, 16 * bh)]
    offs = product.varied_layout([(w, h, w * 4, 0) for (w, h) in sizes], bw, bh)
    T = int(offs[-1])
    assert T == 2116 and (rungs_n - 1) * T * slot >= 2 ** 32
    choice = [rungs_n - 1, 0, rungs_n - 1]
    owner = np.repeat(np.arange(3), np.diff(offs.astype(np.int64)))
    src = torch.from_numpy(np.array(choice)[owner] * T + np.arange(T)).cuda()  # the chosen input tile of every output tile
    assert int((src * slot >= 2 ** 32).sum()) == 1200 + 16
    g = torch.Generator(device="cuda").manual_seed(5)
    slots = torch.empty((rungs_n * T, slot), dtype=torch.uint8, device="cuda")
    decoy = src[src >= 2 ** 16] - 2 ** 16  # same low 32 bits of the byte offset, below 4 GiB
    slots[decoy, :small] = torch.randint(0, 256, (decoy.numel(), small), dtype=torch.uint8, device="cuda", generator=g)
    want = torch.randint(0, 256, (T, small), dtype=torch.uint8, device="cuda", generator=g)
    slots[src, :small] = want
    vals = torch.randint(0, 2 ** 31 - 1, (rungs_n * T,), dtype=torch.int32, device="cuda", generator=g)
    ow = torch.full((rungs_n * T,), 8, dtype=torch.int32, device="cuda")  # stored sizes are small: 256 valid bytes per tile
    oh = torch.full((rungs_n * T,), 8, dtype=torch.int32, device="cuda")
    slots[src, small:small + 64] = 0xC3  # (behind the valid bytes the source holds neither poison: a copy that ran on would show)
    out = out_poisoned((T + 1,), slot)
    gpu.gather_varied_rungs_device(sizes, 4, bw, bh, rungs_n, torch.tensor(choice, dtype=torch.int32, device="cuda"), vals.view(torch.float32),
                                   ow, oh, slots, out=tuple(x[:T] for x in out))
    torch.cuda.synchronize()
    assert out_still_poisoned(tuple(x[T:] for x in out)), "the guard behind the outputs was written"
    o_vals, o_w, o_h, o_slots = out
    assert bool((o_vals[:T].view(torch.int32) == vals[src]).all()) and bool((o_w[:T] == 8).all()) and bool((o_h[:T] == 8).all())
    assert bool((o_slots[:T, :small] == want).all()), "the chosen slots beyond 4 GiB were not the ones read"
    assert bool((o_slots[:T, small:] == OUT_POISON).all()), "a byte behind the valid ones was written"


# ---- 4. the host form ---------------------------------------------------------------------------------------------------------

HOST_SIZES = [(150, 100), (9, 9), (70, 131), (100, 38), (66, 35), (130, 67), (40, 30)]  # (no edge tile of 1 px at 32 or 64)
# unsorted; rungs 1 and 5 are one factor and rungs 2 and 6 another: where a target falls on such a pair, the lower index decides
HOST_FACTORS = {0: [.25, .125, .5, 2, .05, .125, .5, .02], 1: [4, 2, 8, 32, .8, 2, 8, .32]}
DOWN, UP, FILTER_BYTE = 4, 2, 3


def host_images(block, c, mode):
    rng = np.random.default_rng(block + 10 * c + mode)
    images = [make_image(rng, w, h, c, ["partial", "opaque", "clear"][k % 3]) for k, (w, h) in enumerate(HOST_SIZES)]
    # image 0, whose target is 0: a gentle slope under a little noise, so that its tiles shrink at every factor and lose the
    # noise -- no rung of it is free of error, and the target of 0 is missed under either criterion
    h, w = images[0].shape[:2]
    yy, xx = np.mgrid[0:h, 0:w]
    images[0][..., :3] = ((xx + yy) // 4 + 60)[..., None] + rng.integers(0, 3, (h, w, 3))
    if c == 4:
        images[0][..., 3] = 255  # (noise in the alpha channel would keep the tiles whole at the larger factors)
    return images


def targets_from(file_bytes, sse, criterion):
    """per image its third-smallest file length (FIT_BYTES) or error (FIT_SSE); image 0 gets 0, image 1 2^64-1"""
    q = file_bytes if criterion == FIT_BYTES else sse.sum(axis=2)
    t = [int(np.sort(q[:, i])[2]) for i in range(q.shape[1])]
    t[0], t[1] = 0, U64
    return t


@pytest.mark.parametrize("criterion", [FIT_BYTES, FIT_SSE], ids=["bytes", "sse"])
@pytest.mark.parametrize("mode", [0, 1], ids=["shrink_by", "directional"])
@pytest.mark.parametrize("c", [3, 4], ids=["rgb", "rgba"])
@pytest.mark.parametrize("block", [64, 32])
def test_files_equal_todays_composition_and_the_oracle(gpu, product, oracle, block, c, mode, criterion):
    images, factors = host_images(block, c, mode), HOST_FACTORS[mode]
    Kf, n = len(factors), len(images)
    file_bytes, sse = gpu.rate_distortion_varied_images(images, block, block, mode, DOWN, UP, factors)
    targets = targets_from(file_bytes, sse, criterion)
    exp_choice, exp_flags = select(file_bytes.tolist(), sse.tolist(), criterion, targets)
    # what the table must hold for the comparison below to say anything
    total = sse.sum(axis=2)
    assert any(0 < r < Kf - 1 for r in exp_choice), "every expected choice is the first or the last rung"
    assert any(any(q != r and file_bytes[q, i] == file_bytes[r, i] and total[q, i] == total[r, i] for q in range(Kf))
               for i, r in enumerate(exp_choice)), "no choice is decided by the lowest index among equal rungs"
    assert any(exp_flags), "no image misses its target"
    h_choice, h_flags = product.fit_select(file_bytes, sse, criterion, targets)
    assert h_choice.tolist() == exp_choice and h_flags.tolist() == exp_flags

    files, choice, flags, t_bytes, t_sse = gpu.encode_varied_images_fit(images, block, block, mode, DOWN, UP, factors, criterion, targets,
                                                                        filter_byte=FILTER_BYTE, want_table=True)
    assert choice.tolist() == exp_choice and flags.tolist() == exp_flags
    assert (t_bytes == file_bytes).all() and (t_sse == sse).all(), "the table differs from rate_distortion_varied_images'"
    for i, img in enumerate(images):
        k = factors[exp_choice[i]]
        alone = gpu.encode_varied_images([img], block, block, mode, DOWN, k, filter_byte=FILTER_BYTE)[0]
        assert files[i] == alone, f"image {i} at factor {k}: differs from encode_varied_images of the image alone"
        ev, ew, eh, es = oracle.shrink_image(img, block, block, mode, DOWN, k, nthreads=8)
        ref = oracle.encode_container(img.shape[1], img.shape[0], block, block, c, FILTER_BYTE, ev, None, ew, eh, es)
        assert files[i] == ref, f"image {i} at factor {k}: differs from the oracle's file"
        assert len(files[i]) == int(file_bytes[exp_choice[i], i])  # (file_offsets: the binding cuts the files by them)


# ---- 5. and 6. the raw host form: size query, errors ---------------------------------------------------------------------------

class RawFit:
    """pxz_encode_varied_images_fit through ctypes, every output poisoned; fields may be overridden before call()"""

    def __init__(self, gpu, product, images, block_w, block_h, mode, factors, criterion, targets):
        self.gpu, n = gpu, len(images)
        self.images = [np.ascontiguousarray(i) for i in images]
        self.ch = self.images[0].shape[2]
        self.geoms = [(i.shape[1], i.shape[0], i.strides[0], 0) for i in self.images]
        self.block_w, self.block_h, self.mode, self.criterion = block_w, block_h, mode, criterion
        self.fac = np.ascontiguousarray(factors, np.float32)
        self.n_factors = self.fac.size
        self.targets = np.array([int(t) for t in targets], np.uint64)
        self.product = product
        self.offs = np.full(n + 1, U64, np.uint64)
        self.choice, self.flags = np.full(n, POISON32, np.uint32), np.full(n, POISON32, np.uint32)
        kn = max(self.n_factors, 1) * n
        self.t_bytes, self.t_sse = np.full(kn, U64, np.uint64), np.full(kn * self.ch, U64, np.uint64)

    def call(self, out, capacity, null_targets=False, null_factors=False):
        ptr = lambda a: None if a is None else C.c_void_p(a.ctypes.data)  # noqa: E731
        n = len(self.images)
        ptrs = (C.c_void_p * n)(*[i.ctypes.data for i in self.images])
        descs = self.product.image_descs(self.geoms)
        return self.gpu._L.pxz_encode_varied_images_fit(
            self.gpu._h, C.cast(ptrs, C.c_void_p), C.cast(descs, C.c_void_p), n, self.ch, self.block_w, self.block_h, self.mode, DOWN, UP,
            None if null_factors else ptr(self.fac), self.n_factors, self.criterion, None if null_targets else ptr(self.targets), FILTER_BYTE,
            ptr(out), capacity, ptr(self.offs), ptr(self.choice), ptr(self.flags), ptr(self.t_bytes), ptr(self.t_sse))

    def untouched(self):
        return bool((self.offs == U64).all() and (self.choice == POISON32).all() and (self.flags == POISON32).all() and
                    (self.t_bytes == U64).all() and (self.t_sse == U64).all())


def test_size_query_then_exact_capacity(gpu, product):
    images, factors = host_images(32, 4, 0)[:5], HOST_FACTORS[0]
    targets = [0, U64, 2000, 500, 10 ** 6]
    files, choice, flags = gpu.encode_varied_images_fit(images, 32, 32, 0, DOWN, UP, factors, FIT_BYTES, targets, filter_byte=FILTER_BYTE)
    total = sum(len(f) for f in files)
    exp_offs = np.cumsum([0] + [len(f) for f in files]).astype(np.uint64)
    for out, cap in ((None, 0), (None, 10 ** 9), (np.full(total, POISON, np.uint8), total - 1)):
        raw = RawFit(gpu, product, images, 32, 32, 0, factors, FIT_BYTES, targets)
        assert raw.call(out, cap) == BUFFER_TOO_SMALL, (cap, last_error(gpu))
        assert (raw.offs == exp_offs).all() and (raw.choice == choice).all() and (raw.flags == flags).all()
        assert out is None or (out == POISON).all(), "a call that was short of room wrote to out"
    raw = RawFit(gpu, product, images, 32, 32, 0, factors, FIT_BYTES, targets)
    out = np.full(total + 16, POISON, np.uint8)
    assert raw.call(out, total) == 0, last_error(gpu)
    assert out[:total].tobytes() == b"".join(files) and (out[total:] == POISON).all() and (raw.offs == exp_offs).all()


def test_host_form_errors_write_nothing(gpu, product):
    rng = np.random.default_rng(3)
    images, factors = host_images(32, 4, 0)[:4], HOST_FACTORS[0]
    targets = [100] * 4

    def refused(code, text=None, images=images, block=(32, 32), factors=factors, **kw):
        raw = RawFit(gpu, product, images, block[0], block[1], 0, factors, FIT_BYTES, targets)
        call_kw = {}
        for key, v in kw.items():
            if key in ("null_targets", "null_factors"):
                call_kw[key] = v
            else:
                setattr(raw, key, v)
        out = np.full(1 << 20, POISON, np.uint8)
        assert raw.call(out, out.size, **call_kw) == code, (kw, last_error(gpu))
        assert raw.untouched() and (out == POISON).all(), (kw, "an error case wrote its outputs")
        assert text is None or text in last_error(gpu), last_error(gpu)

    refused(INVALID_ARG, criterion=2)
    refused(INVALID_ARG, criterion=2 ** 32 - 1)
    refused(INVALID_ARG, null_targets=True)
    refused(INVALID_ARG, null_factors=True)
    refused(INVALID_ARG, n_factors=0)
    refused(INVALID_ARG, factors=[1.0] * 33)
    refused(INVALID_ARG, factors=[0.5, float("nan")])
    refused(INVALID_ARG, factors=[float("inf"), 0.5])
    refused(INVALID_ARG, images=[rng.integers(0, 256, (20, 20, 5), dtype=np.uint8)] * 4)  # channels of 5
    g = [(i.shape[1], i.shape[0], i.strides[0], 0) for i in images]
    refused(INVALID_ARG, "image 2", geoms=[g[0], g[1], g[2] + (1,), g[3]])  # reserved
    refused(UNSUPPORTED, block=(129, 128))  # 129*128*4 > 65536


def test_device_form_errors_write_nothing(gpu, product):
    import torch
    # the fit
    t = directed_tables()[0]
    K1, n = t["file_bytes"].shape
    offs = to_device_u64(np.concatenate([np.zeros(1, np.uint64), np.cumsum(t["file_bytes"].reshape(-1), dtype=np.uint64)]))
    sse = to_device_u64(t["sse"])

    def fit_refused(**kw):
        out = (torch.full((n,), POISON32, dtype=torch.int32, device="cuda"), torch.full((n,), POISON32, dtype=torch.int32, device="cuda"))
        args = dict(criterion=FIT_BYTES, targets=t["targets"])
        args.update(kw)
        with pytest.raises(product.PxzError) as e:
            gpu.fit_varied_ladder_device(offs, sse, args.pop("criterion"), args.pop("targets"), out=out, **args)
        assert e.value.code == INVALID_ARG, (kw, last_error(gpu))
        torch.cuda.synchronize()
        assert bool((out[0] == POISON32).all() and (out[1] == POISON32).all()), (kw, "an error case wrote its outputs")

    fit_refused(criterion=2)
    fit_refused(targets=None)
    fit_refused(n_factors=0)
    fit_refused(n_factors=33)
    fit_refused(channels=5)
    fit_refused(n_images=0)
    # the gather
    sizes = [(50, 34), (9, 5), (35, 20)]
    T = int(product.varied_layout([(w, h, w * 4, 0) for (w, h) in sizes], 16, 16)[-1])
    src = poisoned((2, T), 16 * 16 * 4, "cuda")
    choice = torch.zeros(3, dtype=torch.int32, device="cuda")

    def gather_refused(code, sizes=sizes, n_factors=2, c=4, block=(16, 16)):
        out = out_poisoned((T,), 16 * 16 * 4)
        flags = torch.full((3,), POISON32, dtype=torch.int32, device="cuda")
        with pytest.raises(product.PxzError) as e:
            gpu.gather_varied_rungs_device(sizes, c, block[0], block[1], n_factors, choice, *src, out=out, image_flags=flags)
        assert e.value.code == code, last_error(gpu)
        torch.cuda.synchronize()
        assert out_still_poisoned(out) and bool((flags == POISON32).all()), "an error case wrote its outputs"

    gather_refused(INVALID_ARG, n_factors=0)
    gather_refused(INVALID_ARG, n_factors=33)
    gather_refused(INVALID_ARG, c=5)
    gather_refused(INVALID_ARG, sizes=[(50, 34, 200, 0), (9, 5, 36, 0, 1), (35, 20, 140, 0)])  # reserved
    assert "image 1" in last_error(gpu)
    gather_refused(INVALID_ARG, sizes=[(50, 34, 200, 0), (0, 5, 36, 0), (35, 20, 140, 0)])  # empty image
    assert "image 1" in last_error(gpu)
    gather_refused(INVALID_ARG, block=(0, 16))


# ---- 7. the handle is left alone ------------------------------------------------------------------------------------------------

def test_the_handle_is_left_alone(gpu, product):
    import torch
    frames = gpu.synth_frames_device(2, 200, 328, 4, dist=product.DIST_ALPHA)
    images, factors = host_images(32, 4, 0)[:4], HOST_FACTORS[0]
    table = directed_tables()[2]

    def single():
        vals, ow, oh, slots = host(gpu.shrink_frames_device(frames, 32, 32, 0, 4, 1.0))
        return vals.reshape(-1), ow.reshape(-1), oh.reshape(-1), slots.reshape(-1, slots.shape[-1])

    def three_calls():
        """the device select, a ladder with its gather, and the host form -> what they returned"""
        got = list(device_select(gpu, table))
        buf, geoms = upload(images, 4)
        out = gpu.shrink_varied_ladder_frames_device(buf, 32, 32, 0, 4, factors, descs=geoms, channels=4)[1:]
        choice = torch.tensor([1, 7, 0, 4], dtype=torch.int32, device="cuda")
        got += [x for x in host(gpu.gather_varied_rungs_device([(g[0], g[1]) for g in geoms], 4, 32, 32, len(factors), choice, *out))]
        files, ch, fl = gpu.encode_varied_images_fit(images, 32, 32, 0, DOWN, UP, factors, FIT_SSE, [0, U64, 10 ** 5, 10 ** 6])
        return got + [np.frombuffer(b"".join(files), np.uint8), ch, fl]

    single()  # (the first launch on a handle has no statistics of a launch before it)
    before, state = single(), gpu.state()
    first = three_calls()
    torch.cuda.synchronize()
    assert gpu.state() == state, "a fit call changed what pxz_handle_state reports"
    assert_same_tiles(single(), before, 4, "the single-geometry call after the fit calls")
    gpu.trim()
    again = three_calls()
    assert len(first) == len(again) == 9
    assert_same_tiles(tuple(again[2:6]), tuple(first[2:6]), 4, "the gather after a trim")
    for k in (0, 1, 6, 7, 8):
        assert first[k].tobytes() == again[k].tobytes(), f"result {k} differs after a trim"
