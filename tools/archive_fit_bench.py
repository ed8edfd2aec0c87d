"""Fit a .pixlzr archive to a budget on one MI355X, without the images: the folder of tools/varied_bench.py (256 RGBA images, sides
64 .. 4096 log-uniform) shrunk once to files at 64x64 and 32x32 blocks in both modes (factor 1.0, or 16 for shrink_directionally),
then re-shrunk at the reference's 20 factors (whole-folder.rs:83-88: k = i / 20; times 16 for shrink_directionally); Lanczos3
down, CatmullRom for both expands.  Both parts check bit for bit before they time, alternate the flows, and report every sample.

(a) the device call alone, on tiles in HBM: pxz_reshrink_distortion_varied_device against what defines it on the same build --
    pxz_expand_varied_frames_device of the archive into a packed image and pxz_distortion_varied_frames_device over the K * n
    descriptors -- timed by events around the calls, allocations warm.  The bytes the image costs are reported beside the times.
(b) the host form: pxz_transcode_varied_files_fit against pxz_decode_varied_files + pxz_encode_varied_images_fit, wall time.
    The targets are each file's median length over the rungs, so the choices spread.

    python tools/archive_fit_bench.py [--images 256] [--reps 3] [--device-only] [--json profiles/archive_fit_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import __graft_entry__ as G  # noqa: E402
from varied_bench import folder, frame_of  # noqa: E402

P = G.load_product()
SWEEP = [i / 20.0 for i in range(20, 0, -1)]  # 1.0, 0.95, ... 0.05
DOWN, XF, UP = 4, 2, 2


def alternate(flows, reps, clock):
    """reps samples of every flow, the order reversed every other round -> {flow: [ms]}"""
    times = {f: [] for f in flows}
    for i in range(reps):
        for f in (flows if i % 2 == 0 else flows[::-1]):
            times[f].append(clock(f))
    return times


def spread(ts):
    return dict(median=round(statistics.median(ts), 3), min=round(min(ts), 3), max=round(max(ts), 3), samples=[round(t, 3) for t in ts])


def device_call(h, buf, geoms, block, mode, reps):
    import torch
    n = len(geoms)
    sizes = [(g[0], g[1]) for g in geoms]
    scale = 16.0 if mode == 1 else 1.0
    factors = [k * scale for k in SWEEP]
    K, slot = len(factors), block * block * 4
    offs, _, aw, ah, aslots = h.shrink_varied_frames_device(buf, block, block, mode, DOWN, scale, descs=geoms, channels=4)
    T = int(offs[-1])
    _, _, ow, oh, slots = h.reshrink_varied_ladder_frames_device(sizes, 4, block, block, mode, DOWN, factors, XF, aw, ah, aslots)
    # the image the old way needs: tightly packed, 256-byte aligned starts
    packed, at = [], 0
    for (w, hh) in sizes:
        packed.append((w, hh, w * 4, at))
        at += (w * hh * 4 + 255) // 256 * 256
    image = torch.zeros(at, dtype=torch.uint8, device="cuda")
    new = torch.empty((K, n, 4), dtype=torch.int64, device="cuda")
    old = torch.empty((K * n, 4), dtype=torch.int64, device="cuda")
    flat = (ow.reshape(-1), oh.reshape(-1), slots.reshape(K * T, slot))

    def run_new():
        h.reshrink_distortion_varied_device(sizes, 4, block, block, XF, UP, aw, ah, aslots, ow, oh, slots, out=(None, new))

    def run_old():
        h.expand_varied_frames_device(packed, 4, block, block, XF, aw, ah, aslots, image)
        h.distortion_varied_frames_device(image, block, block, UP, *flat, descs=packed * K, channels=4, out=(None, old))

    run_new(), run_old()  # (warm: tables, scratch)
    torch.cuda.synchronize()
    if not torch.equal(new.reshape(K * n, 4), old) or not bool(new.any()):
        print(f"MISMATCH device call {block}x{block} mode {mode}", flush=True)
        sys.exit(1)
    stream = torch.cuda.current_stream()

    def clock(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    times = alternate([run_new, run_old], reps, clock)
    tn, to = statistics.median(times[run_new]), statistics.median(times[run_old])
    row = dict(part="a: device call", block=f"{block}x{block}", mode=mode, images=n, K=K, tiles=T, image_bytes=at,
               archive_slot_bytes=T * slot, new_ms=spread(times[run_new]), old_ms=spread(times[run_old]), old_over_new=round(to / tn, 3),
               exact=True, note="call time by events: the launches with their host-side planning and table uploads, not the kernels alone")
    print(json.dumps(row), flush=True)
    del image, slots, flat, aslots
    torch.cuda.empty_cache()
    return row


def host_form(h, imgs, block, mode, reps):
    scale = 16.0 if mode == 1 else 1.0
    factors = [k * scale for k in SWEEP]
    n = len(imgs)
    files = h.encode_varied_images(imgs, block, block, mode, DOWN, scale)
    file_bytes, _ = h.rate_distortion_varied_files(files, block, block, mode, DOWN, XF, UP, factors)
    targets = [int(np.sort(file_bytes[:, i])[len(factors) // 2]) for i in range(n)]

    def run_new():
        return h.transcode_varied_files_fit(files, block, block, mode, DOWN, XF, UP, factors, P.FIT_BYTES, targets)

    def run_old():
        images, _ = h.decode_varied_files(files, 4, block, block, XF)
        return h.encode_varied_images_fit(images, block, block, mode, DOWN, UP, factors, P.FIT_BYTES, targets)

    got, exp = run_new(), run_old()
    if got[0] != exp[0] or not (got[1] == exp[1]).all() or not (got[2] == exp[2]).all():
        print(f"MISMATCH host form {block}x{block} mode {mode}", flush=True)
        sys.exit(1)

    def clock(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3

    times = alternate([run_new, run_old], reps, clock)
    tn, to = statistics.median(times[run_new]), statistics.median(times[run_old])
    row = dict(part="b: host form", block=f"{block}x{block}", mode=mode, images=n, K=len(factors), archive_bytes=sum(len(f) for f in files),
               out_bytes=sum(len(f) for f in got[0]), distinct_choices=len(set(got[1].tolist())), flagged=int(got[2].sum()),
               new_ms=spread(times[run_new]), old_ms=spread(times[run_old]), old_over_new=round(to / tn, 3), byte_exact=True)
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "archive_fit_bench.json"))
    ap.add_argument("--device-only", action="store_true", help="only part (a)")
    args = ap.parse_args()
    h = P.Handle(0)
    buf, geoms = folder(args.images, 2026)
    print(f"folder: {len(geoms)} RGBA images, {sum(g[0] * g[1] for g in geoms) / 1e6:.1f} Mpx", flush=True)
    rows = [device_call(h, buf, geoms, block, mode, max(args.reps, 5)) for block in (64, 32) for mode in (0, 1)]
    imgs = [] if args.device_only else [frame_of(buf, g)[0].cpu().numpy() for g in geoms]
    del buf
    if imgs:
        rows += [host_form(h, imgs, block, mode, args.reps) for block in (64, 32) for mode in (0, 1)]
    h.close()
    with open(args.json, "w") as f:
        json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
