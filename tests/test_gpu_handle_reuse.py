"""One handle over a stream of calls, and caller buffers at every address class, against the oracle.

The parity suite checks each kernel on a fresh situation.  These tests pin what the results may NOT depend on: the counts
the last finished launch left in pinned memory (which pick alpha_kernel / alpha_first and size the worklist grid), the two
worklist counters, the "copied" flag that shares sums[2 t + 1] with the directional sums, and where in a 64-bit address
space the caller's buffers lie.  Bit-exact everywhere: values as u32 bits, sizes, valid slot bytes, file bytes, pixels."""
import numpy as np
import pytest

from test_gpu_parity import assert_same_tiles

pytestmark = pytest.mark.gpu

SEED = 20261016
NEAREST, CATMULLROM, LANCZOS3 = 0, 2, 4
POISON_DIM = -1  # 0xFFFFFFFF as the int32 the binding uses for sizes


def poisoned_tiles(n, T, slot_bytes, pattern, device="cuda"):
    import torch
    vals = torch.empty((n, T), dtype=torch.float32, device=device)
    vals.view(torch.int32).fill_(-1)  # 0xFFFFFFFF, not the -NaN 0xFFC00000 the oracle may store
    ow = torch.full((n, T), POISON_DIM, dtype=torch.int32, device=device)
    oh = torch.full((n, T), POISON_DIM, dtype=torch.int32, device=device)
    slots = torch.full((n, T, slot_bytes), pattern, dtype=torch.uint8, device=device) if slot_bytes else None
    return vals, ow, oh, slots


def fetch_tiles(out, n):
    vals, ow, oh, slots = out
    return (vals[n].cpu().numpy(), ow[n].cpu().numpy().astype(np.uint32), oh[n].cpu().numpy().astype(np.uint32),
            None if slots is None else slots[n].cpu().numpy())


def craft_transparency(opaque, alpha_src, n_transparent, bs, rng):
    """Frames [N, H, W, 4] (CUDA) whose full bs x bs tiles carry transparency in exactly n_transparent of them: those tiles take
    the alpha of alpha_src (and alpha 0 at their first pixel, so that every one of them has some), the rest stay opaque."""
    import torch
    N, H, W, _ = opaque.shape
    cols, rows = W // bs, H // bs
    total = N * cols * rows
    pick = np.zeros(total, bool)
    pick[rng.choice(total, size=n_transparent, replace=False)] = True
    mask = torch.from_numpy(pick.reshape(N, rows, cols)).cuda()
    pix = mask.repeat_interleave(bs, 1).repeat_interleave(bs, 2)  # [N, rows*bs, cols*bs]
    out = opaque.clone()
    a = out[:, : rows * bs, : cols * bs, 3]
    a.copy_(torch.where(pix, alpha_src[:, : rows * bs, : cols * bs, 3], a))
    first = out[:, 0: rows * bs: bs, 0: cols * bs: bs, 3]
    first.copy_(torch.where(mask, torch.zeros_like(first), first))
    return out


# ------------------------------------------------------------------------------------------------------------------------
# 1. unsynchronised call sequences on one handle
# ------------------------------------------------------------------------------------------------------------------------

class Seq:
    """A fixed sequence of calls on one handle.  Every step queues its work (no synchronisation) into outputs that were
    poisoned before the sequence; check() compares them with the oracle once everything has run."""

    def __init__(self, gpu, oracle):
        self.gpu, self.oracle = gpu, oracle
        self.steps = []
        self._exp = {}

    def expected_shrink(self, key, img, bw, bh, mode, filt, factor, want_pixels=True):
        k = (key, bw, bh, mode, filt, factor, want_pixels)
        if k not in self._exp:
            self._exp[k] = self.oracle.shrink_image(img, bw, bh, mode, filt, factor, want_pixels=want_pixels, nthreads=8)
        return self._exp[k]

    def add(self, kind, **kw):
        self.steps.append(dict(kind=kind, **kw))


def build_sequence(gpu, oracle, rng):
    import torch
    seq = Seq(gpu, oracle)
    frames = {}  # name -> (device tensor [N,H,W,C] (maybe a strided view), host copies per frame)

    def put(name, dev):
        torch.cuda.synchronize()
        frames[name] = (dev, [np.ascontiguousarray(dev[n].cpu().numpy()) for n in range(dev.shape[0])])

    # S1: 2 x 1664x1280 RGBA, 32x32 tiles -> 4160 full tiles; 2048 <= 2060 < 4160 / 2: alpha_kernel without alpha_first
    N1, H1, W1 = 2, 1280, 1664
    opaque = gpu.synth_frames_device(N1, H1, W1, 4, first_frame=40, dist=0)
    alpha = gpu.synth_frames_device(N1, H1, W1, 4, first_frame=40, dist=1)
    n1 = N1 * (H1 // 32) * (W1 // 32)
    put("opaque", opaque)
    put("full", craft_transparency(opaque, alpha, n1, 32, rng))
    put("part", craft_transparency(opaque, alpha, 2060, 32, rng))
    put("part_b", craft_transparency(gpu.synth_frames_device(N1, H1, W1, 4, first_frame=47, dist=0), alpha, 2070, 32, rng))
    # ragged, unaligned, strided: pitch 4040 bytes (not a multiple of 16), frame stride with 3 padding rows
    big = torch.zeros((2, 703, 1010, 4), dtype=torch.uint8, device="cuda")
    big[:, :700, 2:1002] = gpu.synth_frames_device(2, 700, 1000, 4, first_frame=51, dist=1)
    put("ragged_unaligned", big[:, :700, 2:1002])
    put("ragged_aligned", gpu.synth_frames_device(2, 700, 1000, 4, first_frame=52, dist=1))
    put("rgb", gpu.synth_frames_device(2, 720, 1000, 3, first_frame=53, dist=0))
    put("rgb64", gpu.synth_frames_device(1, 1088, 1920, 3, first_frame=54, dist=0))
    put("rgba64", gpu.synth_frames_device(1, 1088, 1984, 4, first_frame=55, dist=0))
    put("alpha64", gpu.synth_frames_device(1, 1024, 2048, 4, first_frame=56, dist=1))
    put("opaque64", gpu.synth_frames_device(1, 1024, 2048, 4, first_frame=57, dist=0))
    put("small", gpu.synth_frames_device(2, 200, 328, 4, first_frame=58, dist=1))
    put("small_rgb", gpu.synth_frames_device(2, 200, 328, 3, first_frame=59, dist=0))
    put("edge1", gpu.synth_frames_device(1, 64, 97, 4, first_frame=60, dist=0))  # 97 = 3 x 32 + 1: a 1-px edge tile

    S1 = dict(bw=32, bh=32, mode=1, filt=LANCZOS3, factor=16.0)
    S0 = dict(bw=32, bh=32, mode=0, filt=LANCZOS3, factor=1.0)
    sh = lambda name, **cfg: seq.add("shrink", frames=name, **cfg)
    # the swing on one signature: counts that over- and under-select, listed counts below and above the real ones
    for name in ("opaque", "full", "part", "opaque", "full", "opaque", "part", "full"):
        sh(name, **S1)
    # counts that belong to someone else: other tile sizes, modes, channels, entry points
    sh("ragged_unaligned", bw=16, bh=16, mode=0, filt=LANCZOS3, factor=0.5)
    seq.add("lod", frames="opaque", bw=32, bh=32, mode=1, factor=4.0)
    sh("full", bw=32, bh=32, mode=1, filt=NEAREST, factor=4.0)  # the lod launch above has this signature (want_pixels aside)
    sh("opaque", **S1)
    sh("full", **S1)
    sh("part", **S1)
    seq.add("encode", src=len(seq.steps) - 1)
    seq.add("decode", src=len(seq.steps) - 1)
    seq.add("expand", src=len(seq.steps) - 1, filt=LANCZOS3)
    sh("opaque", **S1)
    seq.add("process", frames="small", bs=32, down=4, up=0)
    sh("full", **S1)
    seq.add("tree", frames="small_rgb", bw=32, bh=32, thr=0.05)
    seq.add("fail_filter", frames="opaque")        # invalid filter: refused before any launch
    sh("part", **S1)
    seq.add("fail_tile", frames="edge1")           # directional on a 1-px edge tile: refused
    sh("opaque", **S1)
    seq.add("trim")
    sh("full", **S1)
    sh("ragged_aligned", bw=48, bh=48, mode=0, filt=CATMULLROM, factor=0.3)   # the run-time geometry detector
    sh("ragged_unaligned", bw=40, bh=24, mode=1, filt=LANCZOS3, factor=8.0)   # generic kernel throughout
    sh("rgb", bw=32, bh=32, mode=0, filt=LANCZOS3, factor=1.0)                # RGB on the square fast paths (clone_ahead)
    sh("rgb", bw=16, bh=16, mode=1, filt=LANCZOS3, factor=16.0)
    sh("rgb64", bw=64, bh=64, mode=0, filt=LANCZOS3, factor=1.0)
    sh("part_b", **S0)
    sh("opaque", **S0)
    sh("full", **S0)
    sh("part_b", **S0)
    sh("alpha64", bw=64, bh=64, mode=0, filt=LANCZOS3, factor=1.0)
    sh("opaque64", bw=64, bh=64, mode=0, filt=LANCZOS3, factor=1.0)
    sh("rgba64", bw=64, bh=64, mode=1, filt=LANCZOS3, factor=16.0)
    seq.add("encode", src=len(seq.steps) - 1)
    seq.add("decode", src=len(seq.steps) - 1)
    seq.add("expand", src=len(seq.steps) - 1, filt=NEAREST)
    sh("part", **S1)
    return seq, frames


def run_sequence(seq, frames, sync, product):
    """Queues every step (sync=False: no synchronisation at all; True: after each step, with Handle.state() recorded).
    Returns the outputs per step and the states."""
    import torch
    gpu = seq.gpu
    outs, states = [], []
    # outputs first, all poisoned (a per-call slot pattern), before anything runs
    for k, st in enumerate(seq.steps):
        pattern = (0x3B + 0x47 * k + (0x80 if sync else 0)) & 0xFF
        if st["kind"] == "shrink":
            dev = frames[st["frames"]][0]
            N, H, W, C = dev.shape
            cols, rows = product.grid(W, H, st["bw"], st["bh"])
            outs.append(poisoned_tiles(N, cols * rows, st["bw"] * st["bh"] * C, pattern))
        elif st["kind"] == "encode":
            src = seq.steps[st["src"]]
            N, H, W, C = frames[src["frames"]][0].shape
            cols, rows = product.grid(W, H, src["bw"], src["bh"])
            cap = N * (26 + rows * 4) + N * cols * rows * (13 + 10 + src["bw"] * src["bh"] * (C + 1) + 8)
            outs.append((torch.full((N + 1,), -1, dtype=torch.int64, device="cuda"),
                         torch.full((cap,), pattern, dtype=torch.uint8, device="cuda")))
        elif st["kind"] == "decode":
            src = seq.steps[seq.steps[st["src"]]["src"]]
            N, H, W, C = frames[src["frames"]][0].shape
            cols, rows = product.grid(W, H, src["bw"], src["bh"])
            outs.append(poisoned_tiles(N, cols * rows, src["bw"] * src["bh"] * C, pattern))
        elif st["kind"] == "expand":
            src = seq.steps[seq.steps[seq.steps[st["src"]]["src"]]["src"]]
            outs.append(torch.full(tuple(frames[src["frames"]][0].shape), pattern, dtype=torch.uint8, device="cuda"))
        else:
            outs.append(None)
    torch.cuda.synchronize()
    for k, st in enumerate(seq.steps):
        kind = st["kind"]
        if kind == "shrink":
            gpu.shrink_frames_device(frames[st["frames"]][0], st["bw"], st["bh"], st["mode"], st["filt"], st["factor"], out=outs[k])
        elif kind == "lod":
            outs[k] = gpu.lod_frames_device(frames[st["frames"]][0], st["bw"], st["bh"], st["mode"], st["factor"])
        elif kind == "encode":
            src = seq.steps[st["src"]]
            gpu.encode_frames_device(tuple(frames[src["frames"]][0].shape), src["bw"], src["bh"], *outs[st["src"]], out=outs[k])
        elif kind == "decode":
            src = seq.steps[seq.steps[st["src"]]["src"]]
            offs, buf = outs[st["src"]]
            gpu.decode_frames_device(buf, offs, tuple(frames[src["frames"]][0].shape), src["bw"], src["bh"], out=outs[k])
        elif kind == "expand":
            src = seq.steps[seq.steps[seq.steps[st["src"]]["src"]]["src"]]
            _, ow, oh, slots = outs[st["src"]]
            gpu.expand_frames_device(tuple(frames[src["frames"]][0].shape), src["bw"], src["bh"], st["filt"], ow, oh, slots, out=outs[k])
        elif kind == "process":
            outs[k] = gpu.process_frames_device(frames[st["frames"]][0], st["bs"], st["bs"], st["down"], st["up"])
        elif kind == "tree":
            outs[k] = gpu.tree_process_frames_device(frames[st["frames"]][0], st["bw"], st["bh"], st["thr"])
        elif kind == "fail_filter":
            with pytest.raises(product.PxzError) as e:
                gpu.shrink_frames_device(frames[st["frames"]][0], 32, 32, 1, 9, 16.0)
            assert e.value.code == -1
        elif kind == "fail_tile":
            with pytest.raises(product.PxzError) as e:
                gpu.shrink_frames_device(frames[st["frames"]][0], 32, 32, 1, LANCZOS3, 16.0)
            assert e.value.code == -4
        elif kind == "trim":
            gpu.trim()
        if sync:
            torch.cuda.synchronize()
            states.append(gpu.state())
    torch.cuda.synchronize()
    return outs, states


def check_sequence(seq, frames, outs, what):
    oracle = seq.oracle
    for k, st in enumerate(seq.steps):
        kind = st["kind"]
        tag = f"{what}, seed {SEED}, step {k} ({kind} {st.get('frames', '')} {st.get('bw', '')}x{st.get('bh', '')} mode {st.get('mode', '')})"
        if kind == "shrink":
            dev, host = frames[st["frames"]]
            for n, img in enumerate(host):
                exp = seq.expected_shrink((st["frames"], n), img, st["bw"], st["bh"], st["mode"], st["filt"], st["factor"])
                assert_same_tiles(fetch_tiles(outs[k], n), exp, dev.shape[3], f"{tag} frame {n}")
        elif kind == "lod":
            l0, l1 = outs[k][0].cpu().numpy(), outs[k][1].cpu().numpy()
            dev, host = frames[st["frames"]]
            N, H, W, C = dev.shape
            cols, rows = oracle.grid(W, H, st["bw"], st["bh"])
            for n, img in enumerate(host):
                exp = np.zeros((2, cols * rows), np.float32)
                for t in range(cols * rows):
                    x, y, w, h = oracle.tile_rect(W, H, st["bw"], st["bh"], t)
                    exp[0, t], exp[1, t] = oracle.lod_directional(img[y:y + h, x:x + w])[:2]
                assert (l0[n].view(np.uint32) == exp[0].view(np.uint32)).all(), f"{tag} frame {n}: lod0"
                assert (l1[n].view(np.uint32) == exp[1].view(np.uint32)).all(), f"{tag} frame {n}: lod1"
        elif kind == "encode":
            src = seq.steps[st["src"]]
            dev, host = frames[src["frames"]]
            N, H, W, C = dev.shape
            offs, buf = outs[k]
            offs = offs.cpu().numpy()
            data = buf[: int(offs[-1])].cpu().numpy().tobytes()
            for n, img in enumerate(host):
                v, w, h, s = seq.expected_shrink((src["frames"], n), img, src["bw"], src["bh"], src["mode"], src["filt"], src["factor"])
                ref = oracle.encode_container(W, H, src["bw"], src["bh"], C, 0, v, None, w, h, s)
                assert data[offs[n]:offs[n + 1]] == ref, f"{tag} file {n}"
        elif kind == "decode":
            src = seq.steps[seq.steps[st["src"]]["src"]]
            dev, host = frames[src["frames"]]
            for n, img in enumerate(host):
                exp = seq.expected_shrink((src["frames"], n), img, src["bw"], src["bh"], src["mode"], src["filt"], src["factor"])
                assert_same_tiles(fetch_tiles(outs[k], n), exp, dev.shape[3], f"{tag} file {n}")
        elif kind == "expand":
            src = seq.steps[seq.steps[seq.steps[st["src"]]["src"]]["src"]]
            dev, host = frames[src["frames"]]
            N, H, W, C = dev.shape
            got = outs[k].cpu().numpy()
            for n, img in enumerate(host):
                _, w, h, s = seq.expected_shrink((src["frames"], n), img, src["bw"], src["bh"], src["mode"], src["filt"], src["factor"])
                ref = oracle.expand_image(W, H, src["bw"], src["bh"], C, st["filt"], w, h, s)
                bad = (got[n] != ref).any(axis=2)
                assert not bad.any(), f"{tag} frame {n}: {int(bad.sum())} pixels differ"
        elif kind == "process":
            got = outs[k].cpu().numpy()
            for n, img in enumerate(frames[st["frames"]][1]):
                bad = (got[n] != oracle.process_image(img, st["bs"], st["bs"], st["down"], st["up"])).any(axis=2)
                assert not bad.any(), f"{tag} frame {n}: {int(bad.sum())} pixels differ"
        elif kind == "tree":
            got = outs[k].cpu().numpy()
            for n, img in enumerate(frames[st["frames"]][1]):
                bad = (got[n] != oracle.tree_process_image(img, st["bw"], st["bh"], st["thr"])).any(axis=2)
                assert not bad.any(), f"{tag} frame {n}: {int(bad.sum())} pixels differ"


def test_unsynchronised_call_sequence_on_one_handle(product, oracle):
    """~50 calls on one handle: a swing of one signature between opaque, fully and partly transparent frames (the counts of
    the last finished launch over- and under-select the kernels and under- and over-size the worklist grid), calls of other
    signatures and other entry points (lod, encode, decode, expand, process, tree) in between, two refused calls and a trim.
    Queued without any synchronisation, then once more with a synchronisation after each call; both equal the oracle, and
    the synchronised run shows that the sequence reached every selection it is meant to cover."""
    import torch
    rng = np.random.default_rng(SEED)
    gpu = product.Handle(0)
    try:
        seq, frames = build_sequence(gpu, oracle, rng)
        outs, _ = run_sequence(seq, frames, False, product)
        assert gpu.decode_status() == 0, f"seed {SEED}"
        check_sequence(seq, frames, outs, "unsynchronised")
        del outs
        outs, states = run_sequence(seq, frames, True, product)
        check_sequence(seq, frames, outs, "synchronised")
    finally:
        gpu.close()
    # what the synchronised run reached (state() after step k: the selection step k made, and the counts it left behind)
    sig = lambda st: tuple(st.get(x) for x in ("kind", "bw", "bh", "mode", "filt", "factor")) + (tuple(frames[st["frames"]][0].shape),)
    covered = set()
    prev_launch = None  # index of the last step that launched the shrink kernels
    for k, st in enumerate(seq.steps):
        if st["kind"] != "shrink":
            if st["kind"] in ("lod", "process", "tree"):
                prev_launch = None  # (they go through the same launch, with their own signature)
            continue
        s = states[k]
        if s["alpha_kernel"] and not s["alpha_first"]:
            covered.add("alpha_kernel only")
        if s["alpha_first"]:
            assert s["alpha_kernel"]
            covered.add("alpha_first")
        if not s["alpha_kernel"]:
            covered.add("neither")
        if (st["bw"], st["mode"]) == (32, 1) and s["alpha_kernel"] and st["frames"] == "opaque":
            covered.add("alpha kernel on opaque frames")
        if (st["bw"], st["mode"]) == (32, 1) and not s["alpha_kernel"] and st["frames"] == "full":
            covered.add("no alpha kernel on transparent frames")
        if prev_launch is not None and sig(seq.steps[prev_launch]) == sig(st):
            expect, real = states[prev_launch]["tiles_listed_by_last_finished_launch"], s["tiles_listed_by_last_finished_launch"]
            if expect is not None and real is not None:
                covered.add("listed below" if expect < real else ("listed above" if expect > real else "listed equal"))
        prev_launch = k
    want = {"alpha_kernel only", "alpha_first", "neither", "listed below", "listed above",
            "alpha kernel on opaque frames", "no alpha kernel on transparent frames"}
    assert want <= covered, f"seed {SEED}: the sequence no longer reaches {sorted(want - covered)} (reached {sorted(covered)})"


# ------------------------------------------------------------------------------------------------------------------------
# 2. the "copied" flag in sums[2 t + 1]
# ------------------------------------------------------------------------------------------------------------------------

def trap_frame():
    """1024x1024 RGBA, flat grey, with the bottom-right pixel of every 32x32 tile one step redder: the only 3x3 window of a tile
    that sees it is the last one, where it is the +1 corner of both Sobel kernels -- the directional detector leaves
    (sum_hz, sum_vr) = (1, 1) in sums[] for every tile, i.e. a 1 in sums[2 t + 1], the dword that means "copied" to shrink_by."""
    img = np.full((1024, 1024, 4), 128, np.uint8)
    img[..., 3] = 255
    img[31::32, 31::32, 0] += 1
    return img


def busy_edges(img, bs, rng):
    """Noise over the ragged right column and bottom row, so that those tiles are stored at full size (level 0)."""
    H, W, C = img.shape
    out = img.copy()
    ex, ey = (W // bs) * bs, (H // bs) * bs
    out[:, ex:, :3] = rng.integers(0, 256, out[:, ex:, :3].shape, dtype=np.uint8)
    out[ey:, :, :3] = rng.integers(0, 256, out[ey:, :, :3].shape, dtype=np.uint8)
    return out


def test_copied_flag_is_never_taken_from_another_launch(product, oracle):
    """One handle, geometries of 1024 tiles each (sums[] and the work buffer are reused without reallocation).  Before every
    shrink_by the directional detector sets the trap: a 1 in sums[2 t + 1] of every tile (shown through lod_frames_device).
    Then shrink_by with slots on a ragged frame (the right column is not the detector's: its flag stays 1), shrink_by without
    slots (no copies) then with, RGB at 16 px (never copies) then RGBA at 32 px, RGBA at 16 px, and the 64-px pair
    (clone_split64_kernel and its list), ragged and transparent.  Slots are poisoned before every call: a tile skipped
    without having been copied in that launch shows as a difference in its valid bytes."""
    import torch
    rng = np.random.default_rng(SEED + 2)
    gpu = product.Handle(0)
    trap = trap_frame()
    trap_dev = torch.from_numpy(trap)[None].cuda()
    fac = 30 * 30 * 4096
    one = np.float32(1.0 / fac)  # what a sum of 1 comes out as (operations.rs:256-257)
    k_call = [0]

    def set_trap():
        vals, ow, oh, slots = gpu.shrink_frames_device(trap_dev, 32, 32, 1, LANCZOS3, 16.0)
        l0, l1 = gpu.lod_frames_device(trap_dev, 32, 32, 1, 16.0)
        torch.cuda.synchronize()
        exp = oracle.shrink_image(trap, 32, 32, 1, LANCZOS3, 16.0)
        assert_same_tiles(fetch_tiles((vals, ow, oh, slots), 0), exp, 4, f"seed {SEED}: trap")
        assert (l1.cpu().numpy()[0] == one).all() and (l0.cpu().numpy()[0] == one).all(), \
            f"seed {SEED}: the trap frame no longer leaves a sum of 1 in sums[2 t + 1]"

    def shrink(img, bs, want_pixels=True, hint=False, expect_whole_edges=False):
        k_call[0] += 1
        H, W, C = img.shape
        cols, rows = product.grid(W, H, bs, bs)
        assert cols * rows == 1024
        out = poisoned_tiles(1, 1024, bs * bs * C if want_pixels else 0, (0x29 * k_call[0] + 7) & 0xFF)
        dev = torch.from_numpy(img)[None].cuda()
        gpu.shrink_frames_device(dev, bs, bs, 0, LANCZOS3, 1.0, want_pixels=want_pixels, out=out, transparency_hint=hint)
        torch.cuda.synchronize()
        exp = oracle.shrink_image(img, bs, bs, 0, LANCZOS3, 1.0, want_pixels=want_pixels, nthreads=8)
        what = f"seed {SEED}: call {k_call[0]}, {W}x{H} c{C} at {bs} px, slots {want_pixels}, hint {hint}"
        assert_same_tiles(fetch_tiles(out, 0), exp, C, what)
        if expect_whole_edges:  # the trap can bite: ragged tiles that are stored whole, with a stale 1 in their flag
            ex, ey = W // bs, H // bs
            edge = np.array([(t % cols) >= ex or (t // cols) >= ey for t in range(1024)])
            whole = (exp[1] == np.minimum(bs, W - (np.arange(1024) % cols) * bs)) & \
                    (exp[2] == np.minimum(bs, H - (np.arange(1024) // cols) * bs))
            assert (edge & whole).sum() >= 16, what

    try:
        opaque = lambda w, h, c, f: oracle.synth_frame(w, h, c, f, 0)
        set_trap()
        shrink(busy_edges(opaque(1000, 1000, 4, 70), 32, rng), 32, expect_whole_edges=True)  # ragged, edge 8
        set_trap()
        shrink(opaque(1024, 1024, 4, 71), 32, want_pixels=False)
        shrink(opaque(1024, 1024, 4, 72), 32)
        set_trap()
        shrink(opaque(512, 512, 3, 73), 16)
        shrink(opaque(1024, 1024, 4, 74), 32)
        set_trap()
        shrink(opaque(512, 512, 4, 75), 16)
        shrink(busy_edges(opaque(500, 500, 4, 76), 16, rng), 16, expect_whole_edges=True)  # 32 x 32 tiles, edge 4
        set_trap()
        shrink(opaque(2048, 2048, 4, 77), 64)
        set_trap()
        shrink(busy_edges(opaque(2000, 2000, 4, 78), 64, rng), 64, expect_whole_edges=True)  # edge 16
        set_trap()
        shrink(oracle.synth_frame(2048, 2048, 4, 79, 1), 64, hint=True)
        shrink(oracle.synth_frame(2048, 2048, 4, 80, 1), 64)  # (transparency as seen by the launch before)
        set_trap()
        shrink(opaque(2048, 2048, 3, 81), 64)
        shrink(opaque(1024, 1024, 3, 82), 32)
    finally:
        gpu.close()


# ------------------------------------------------------------------------------------------------------------------------
# 3. caller buffers at every address class
# ------------------------------------------------------------------------------------------------------------------------

GIB4 = 1 << 32
ARENA = GIB4 + (1 << 29)  # one allocation of 4.5 GiB: every residue mod 2^32, and a boundary with 256 MiB on either side


class Arena:
    def __init__(self):
        import torch
        self.t = torch.empty(ARENA, dtype=torch.uint8, device="cuda")
        self.base = self.t.data_ptr()
        # a multiple of 2^32 with 256 MiB of the arena on either side (the interval has length 2^32: there is one)
        lo, hi = self.base + (1 << 28), self.base + ARENA - (1 << 28)
        self.k = ((lo + GIB4 - 1) // GIB4) * GIB4
        assert lo <= self.k <= hi
        # 256 MiB whose addresses all have bit 31 of the low half set, away from the boundary region
        self.hi_half = self.k - (1 << 31) if self.k - (1 << 31) >= self.base else self.k + (1 << 31)
        assert self.base <= self.hi_half and self.hi_half + (1 << 28) <= self.base + ARENA
        assert self.hi_half + (1 << 28) <= self.k - (1 << 28) or self.hi_half >= self.k + (1 << 28)
        self.bump = self.hi_half

    def view(self, addr, nbytes, dtype, shape):
        import torch
        off = addr - self.base
        assert 0 <= off and off + nbytes <= ARENA, "a view outside the arena"
        v = self.t[off: off + nbytes].view(dtype).view(shape)
        assert v.data_ptr() == addr
        return v

    def carve(self, cls, nbytes, dtype, shape, misalign=0):
        """cls 'a': bit 31 of the low half set (bump allocation in that region); 'b': spans the boundary strictly inside;
        'c': starts in the last 4 KiB before the boundary."""
        if cls == "a":
            addr = self.bump + misalign
            self.bump = (addr + nbytes + 4095) & ~4095
            assert self.bump <= self.hi_half + (1 << 28)
            assert all(((a & 0xFFFFFFFF) >> 31) == 1 for a in (addr, addr + nbytes - 1)), hex(addr)
        elif cls == "b":
            half = (nbytes // 2) & ~255 if nbytes >= 512 else 16
            addr = self.k - half + misalign
            assert addr < self.k < addr + nbytes - 1, (hex(addr), nbytes)
        else:
            addr = self.k - 4096 + 48 + misalign
            assert (addr & 0xFFFFFFFF) >= GIB4 - 4096 and addr < self.k
        return self.view(addr, nbytes, dtype, shape)


def test_caller_buffers_at_every_address_class(product, oracle):
    """Every caller-owned buffer of a round trip carved out of one 4.5 GiB allocation: (a) all of them where bit 31 of the
    address's low half is set; (b) each in turn spanning a multiple of 2^32; (c) each in turn starting in the last 4 KiB
    below one.  shrink_by and shrink_directionally at 16 / 32 / 64 / 48 px (RGBA 16-byte aligned, and RGB 4-byte aligned
    at 32 px), then writer -> reader -> expand; everything equal to the oracle."""
    import torch
    gpu = product.Handle(0)
    arena = Arena()
    N, H, W = 2, 760, 1000
    host4 = [oracle.synth_frame(W, H, 4, 90 + n, 1) for n in range(N)]
    host3 = [oracle.synth_frame(W, H, 3, 92 + n, 0) for n in range(N)]
    configs = [(16, 0, 4), (16, 1, 4), (32, 0, 4), (32, 1, 4), (64, 0, 4), (64, 1, 4), (48, 0, 4), (48, 1, 4), (32, 0, 3)]
    factor = {0: 1.0, 1: 16.0}
    exp = {(bs, m, c): [oracle.shrink_image((host4 if c == 4 else host3)[n], bs, bs, m, LANCZOS3, factor[m], nthreads=8)
                        for n in range(N)] for bs, m, c in configs}

    def place(roles, cls, role, nbytes, dtype, shape, misalign=0):
        if cls == "a" or role in roles:
            return arena.carve(cls, nbytes, dtype, shape, misalign)
        return torch.empty(shape, dtype=dtype, device="cuda")

    def check_shrink(out, key, what):
        for n in range(N):
            assert_same_tiles(fetch_tiles(out, n), exp[key][n], key[2], f"{what} frame {n}")

    def round_trip(cls, roles):
        what0 = f"class {cls}, {roles or 'all'}"
        for bs, m, c in configs:
            what = f"{what0}: {bs} px mode {m} c{c}"
            if cls == "a":
                arena.bump = arena.hi_half  # (the views of the last configuration are dead: synchronised and checked)
            cols, rows = product.grid(W, H, bs, bs)
            T = cols * rows
            mis = 4 if c == 3 else 0  # RGB: rows and frames 4-byte aligned, not 16
            frames = place(roles, cls, "frames", N * H * W * c, torch.uint8, (N, H, W, c), mis)
            frames.copy_(torch.from_numpy(np.stack(host4 if c == 4 else host3)))
            vals = place(roles, cls, "values", N * T * 4, torch.float32, (N, T))
            ow = place(roles, cls, "dims", N * T * 4, torch.int32, (N, T))
            oh = place(roles, cls, "dims" if cls == "a" else "", N * T * 4, torch.int32, (N, T))  # (b, c: one buffer per boundary)
            slots = place(roles, cls, "slots", N * T * bs * bs * c, torch.uint8, (N, T, bs * bs * c))
            vals.view(torch.int32).fill_(-1)
            ow.fill_(-1)
            oh.fill_(-1)
            slots.fill_(0x5C)
            gpu.shrink_frames_device(frames, bs, bs, m, LANCZOS3, factor[m], out=(vals, ow, oh, slots))
            torch.cuda.synchronize()
            check_shrink((vals, ow, oh, slots), (bs, m, c), what)
            if (bs, m, c) not in ((32, 1, 4), (64, 0, 4), (16, 0, 4)):
                continue
            # writer -> reader -> expand on these tiles
            cap = N * (26 + rows * 4) + N * T * (13 + 10 + bs * bs * (c + 1) + 8)
            offs = place(roles, cls, "file offsets", (N + 1) * 8, torch.int64, (N + 1,))
            buf = place(roles, cls, "files", cap, torch.uint8, (cap,))
            offs.fill_(-1)
            buf.fill_(0xA5)
            gpu.encode_frames_device((N, H, W, c), bs, bs, vals, ow, oh, slots, out=(offs, buf))
            dv = place(roles, cls, "decoded values", N * T * 4, torch.float32, (N, T))
            dw = place(roles, cls, "decoded dims", N * T * 4, torch.int32, (N, T))
            dh = place(roles, cls, "decoded dims" if cls == "a" else "", N * T * 4, torch.int32, (N, T))
            ds = place(roles, cls, "decoded slots", N * T * bs * bs * c, torch.uint8, (N, T, bs * bs * c))
            dv.view(torch.int32).fill_(-1)
            dw.fill_(-1)
            dh.fill_(-1)
            ds.fill_(0x6D)
            gpu.decode_frames_device(buf, offs, (N, H, W, c), bs, bs, out=(dv, dw, dh, ds))
            img = place(roles, cls, "expanded", N * H * W * c, torch.uint8, (N, H, W, c))
            img.fill_(0x7E)
            gpu.expand_frames_device((N, H, W, c), bs, bs, LANCZOS3, dw, dh, ds, out=img)
            torch.cuda.synchronize()
            assert gpu.decode_status() == 0, what
            o = offs.cpu().numpy()
            data = buf[: int(o[-1])].cpu().numpy().tobytes()
            got = img.cpu().numpy()
            for n in range(N):
                v, w, h, s = exp[(bs, m, c)][n]
                ref = oracle.encode_container(W, H, bs, bs, c, 0, v, None, w, h, s)
                assert data[o[n]:o[n + 1]] == ref, f"{what}: file {n}"
                ref = oracle.expand_image(W, H, bs, bs, c, LANCZOS3, w, h, s)
                bad = (got[n] != ref).any(axis=2)
                assert not bad.any(), f"{what}: expand, frame {n}: {int(bad.sum())} pixels differ"
            check_shrink((dv, dw, dh, ds), (bs, m, c), f"{what}: decoded")
            del offs, buf, dv, dw, dh, ds, img
        # (views of the arena go with the loop's names)

    try:
        round_trip("a", ())
        for role in ("frames", "values", "dims", "slots", "file offsets", "files", "decoded values", "decoded dims",
                     "decoded slots", "expanded"):
            for cls in ("b", "c"):
                round_trip(cls, (role,))
    finally:
        gpu.close()
        del arena
        torch.cuda.empty_cache()
