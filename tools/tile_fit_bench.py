"""Fit to a budget per tile on one MI355X, on the folder of tools/varied_bench.py (256 RGBA images, sides 64 .. 4096
log-uniform) at the reference's 20 factors (whole-folder.rs:83-88; times 16 for shrink_directionally), 64x64 and 32x32 blocks,
both modes, Lanczos3 down and CatmullRom up.

What the feature buys (deterministic integers, from the device calls on the folder's tiles in HBM): at each image's median file
length as its target, the total squared error and the PSNR of a rung per tile (pxz_fit_varied_tiles_device, every image its own
group) against a factor per image (pxz_fit_varied_ladder_device) on the same tables; and the folder as ONE group whose target is
the sum of those budgets.  The device's result is checked against pxz_fit_tiles_select, and the gather against per-tile slices
of the rungs, before anything is timed.

Time: the select and the gather calls alone by events on the handle's stream (the call with its host-side planning and uploads,
not the kernels alone), the gather's algorithmic traffic over its time; then the host form pxz_encode_varied_images_fit_tiles
against pxz_encode_varied_images_fit on the same inputs, alternating, wall time, every sample reported.

    python tools/tile_fit_bench.py [--images 256] [--reps 3] [--device-only] [--json out.json]
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
DOWN, UP = 4, 2


def psnr_of(sse, samples):
    return round(P.psnr(int(sse), samples), 3) if sse else float("inf")


def device_steps(h, buf, geoms, reps):
    import torch
    n, rows = len(geoms), []
    sizes = [(g[0], g[1]) for g in geoms]
    samples = sum(w * hh for (w, hh) in sizes) * 4
    stream = torch.cuda.current_stream()
    for block in (64, 32):
        for mode in (0, 1):
            factors = [k * (16.0 if mode == 1 else 1.0) for k in SWEEP]
            K, slot = len(factors), block * block * 4
            offs, vals, ow, oh, slots = h.shrink_varied_ladder_frames_device(buf, block, block, mode, DOWN, factors, descs=geoms, channels=4)
            T = int(offs[-1])
            flat = (vals.reshape(-1), ow.reshape(-1), oh.reshape(-1), slots.reshape(K * T, slot))
            rec, foffs = h.record_bytes_varied_device(sizes * K, 4, block, block, *flat)
            tile_sse, image_sse = h.distortion_varied_frames_device(buf, block, block, UP, flat[1], flat[2], flat[3], descs=list(geoms) * K, channels=4)
            rec, tile_sse, image_sse = rec.reshape(K, T), tile_sse.reshape(K, T, 4), image_sse.reshape(K, n, 4)
            file_bytes = (foffs[1:] - foffs[:-1]).reshape(K, n)
            targets = torch.sort(file_bytes, dim=0)[0][K // 2].cpu().tolist()
            # a factor per image, the yardstick
            i_choice, i_flags = h.fit_varied_ladder_device(foffs, image_sse, P.FIT_BYTES, targets)
            pick = i_choice.long().view(1, n)
            image_fit_bytes = int(file_bytes.gather(0, pick).sum())
            image_fit_sse = int(image_sse.sum(dim=2).gather(0, pick).sum())
            # a rung per tile: every image its own group, and the folder as one group with the summed budget
            per_image = h.fit_varied_tiles_device(sizes, 4, block, block, rec, tile_sse, P.FIT_BYTES, targets)
            folder_fit = h.fit_varied_tiles_device(sizes, 4, block, block, rec, tile_sse, P.FIT_BYTES, [sum(targets)], group_first=[0, n])
            out = h.gather_varied_tile_rungs_device(sizes, 4, block, block, K, per_image[0], vals, ow, oh, slots)
            torch.cuda.synchronize()
            # checks: the host's select on the downloaded tables; the gather against per-tile slices
            rows_of = [-(-g[1] // block) for g in geoms]
            h_rec, h_sse = rec.cpu().numpy().astype(np.uint32), tile_sse.cpu().numpy().view(np.uint64)
            ok = True
            for got, tile_offs, fixed, tg in ((per_image, offs, [26 + 4 * r for r in rows_of], targets),
                                              (folder_fit, [0, T], [sum(26 + 4 * r for r in rows_of)], [sum(targets)])):
                exp = P.fit_tiles_select(tile_offs, fixed, h_rec, h_sse, P.FIT_BYTES, tg)
                ok = ok and all((g.cpu().numpy().astype(e.dtype) == e).all() for g, e in zip(got, exp))
            src = per_image[0].long() * T + torch.arange(T, device="cuda")
            ok = ok and torch.equal(out[0].view(torch.int32), flat[0].view(torch.int32)[src]) and torch.equal(out[1], flat[1][src])
            ok = ok and torch.equal(out[2], flat[2][src])
            valid_bytes = 0
            for a in range(0, T, 1 << 15):  # (the mask of a whole batch would not fit beside it)
                w = (out[1][a:a + (1 << 15)] * out[2][a:a + (1 << 15)] * 4).view(-1, 1)
                valid = torch.arange(slot, device="cuda").view(1, -1) < w
                ok = ok and torch.equal(out[3][a:a + (1 << 15)][valid], flat[3][src[a:a + (1 << 15)]][valid])
                valid_bytes += int(w.sum())
            if not ok:
                print(f"MISMATCH device steps {block}x{block} mode {mode}", flush=True)
                sys.exit(1)

            def timed(fn):
                ts = []
                for i in range(reps + 1):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    fn()
                    e1.record(stream)
                    torch.cuda.synchronize()
                    if i:
                        ts.append(e0.elapsed_time(e1))
                return ts

            t_rec = timed(lambda: h.record_bytes_varied_device(sizes * K, 4, block, block, *flat, out=(rec.reshape(-1), foffs)))
            t_sel = timed(lambda: h.fit_varied_tiles_device(sizes, 4, block, block, rec, tile_sse, P.FIT_BYTES, targets, out=per_image))
            t_one = timed(lambda: h.fit_varied_tiles_device(sizes, 4, block, block, rec, tile_sse, P.FIT_BYTES, [sum(targets)], group_first=[0, n],
                                                            out=folder_fit))
            t_img = timed(lambda: h.fit_varied_ladder_device(foffs, image_sse, P.FIT_BYTES, targets, out=(i_choice, i_flags)))
            t_gather = timed(lambda: h.gather_varied_tile_rungs_device(sizes, 4, block, block, K, per_image[0], vals, ow, oh, slots, out=out))
            moved = 2 * (valid_bytes + 12 * T) + 4 * T
            tg = statistics.median(t_gather)
            tb, ts = int(per_image[2].sum()), int(per_image[3].sum())
            fl = per_image[4].cpu().numpy()
            row = dict(device_steps=True, block=f"{block}x{block}", mode=mode, images=n, K=K, tiles=T, budget_bytes=sum(targets),
                       image_fit_bytes=image_fit_bytes, image_fit_sse=image_fit_sse, image_fit_psnr=psnr_of(image_fit_sse, samples),
                       image_fit_missed=int(i_flags.sum()),
                       tile_fit_bytes=tb, tile_fit_sse=ts, tile_fit_psnr=psnr_of(ts, samples), tile_fit_missed=int((fl & 1).sum()),
                       tile_fit_uniform_groups=int(((fl & 4) != 0).sum()),
                       folder_fit_bytes=int(folder_fit[2][0]), folder_fit_sse=int(folder_fit[3][0]), folder_fit_psnr=psnr_of(int(folder_fit[3][0]), samples),
                       folder_fit_lambda=int(folder_fit[1][0]), folder_fit_flags=int(folder_fit[4][0]),
                       sse_tile_over_image=round(ts / image_fit_sse, 4) if image_fit_sse else None,
                       sse_folder_over_image=round(int(folder_fit[3][0]) / image_fit_sse, 4) if image_fit_sse else None,
                       record_bytes_ms=round(statistics.median(t_rec), 4), select_ms=round(statistics.median(t_sel), 4),
                       select_one_group_ms=round(statistics.median(t_one), 4), image_select_ms=round(statistics.median(t_img), 4),
                       gather_ms=round(tg, 4), gathered_valid_bytes=valid_bytes, gather_gbps=round(moved / tg / 1e6, 1), exact=True,
                       note="call times by events: the launches with their host-side planning and table uploads, not the kernels alone",
                       record_bytes_samples=[round(t, 4) for t in t_rec], select_samples=[round(t, 4) for t in t_sel],
                       select_one_group_samples=[round(t, 4) for t in t_one], image_select_samples=[round(t, 4) for t in t_img],
                       gather_samples=[round(t, 4) for t in t_gather])
            rows.append(row)
            print(json.dumps(row), flush=True)
            del vals, ow, oh, slots, flat, out, tile_sse, rec
            torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--json", default=None)
    ap.add_argument("--device-only", action="store_true", help="only the device calls on device-resident tiles")
    args = ap.parse_args()
    h = P.Handle(0)
    buf, geoms = folder(args.images, 2026)
    rows = device_steps(h, buf, geoms, max(args.reps, 5))
    imgs = [] if args.device_only else [frame_of(buf, g)[0].cpu().numpy() for g in geoms]
    del buf
    n = len(imgs)
    print(f"folder: {len(geoms)} RGBA images, {sum(g[0] * g[1] for g in geoms) / 1e6:.1f} Mpx", flush=True)
    for block in ((64, 32) if n else ()):
        for mode in (0, 1):
            factors = [k * (16.0 if mode == 1 else 1.0) for k in SWEEP]
            file_bytes, sse = h.rate_distortion_varied_images(imgs, block, block, mode, DOWN, UP, factors)
            targets = [int(np.sort(file_bytes[:, i])[len(factors) // 2]) for i in range(n)]

            def run_tiles():
                return h.encode_varied_images_fit_tiles(imgs, block, block, mode, DOWN, UP, factors, P.FIT_BYTES, targets)

            def run_images():
                return h.encode_varied_images_fit(imgs, block, block, mode, DOWN, UP, factors, P.FIT_BYTES, targets)

            got, exp = run_tiles(), run_images()
            t_bytes, t_sse = int(got[3].sum()), int(got[4].sum())
            i_bytes = sum(len(f) for f in exp[0])
            i_sse = int(sum(sse[exp[1][i], i].sum() for i in range(n)))
            if t_bytes != sum(len(f) for f in got[0]) or any(len(f) > t for f, t, fl in zip(got[0], targets, got[5]) if not fl & 1):
                print(f"MISMATCH {block}x{block} mode {mode}: the files are not what the groups' totals say", flush=True)
                sys.exit(1)
            flows = [run_tiles, run_images]
            times = {f: [] for f in flows}
            for i in range(args.reps):
                for f in (flows if i % 2 == 0 else flows[::-1]):
                    t0 = time.perf_counter()
                    f()
                    times[f].append((time.perf_counter() - t0) * 1e3)
            tt, ti = statistics.median(times[run_tiles]), statistics.median(times[run_images])
            row = dict(block=f"{block}x{block}", mode=mode, criterion="bytes", images=n, K=len(factors), tile_fit_files_bytes=t_bytes,
                       tile_fit_sse=t_sse, image_fit_files_bytes=i_bytes, image_fit_sse=i_sse, tile_fit_ms=round(tt, 1), image_fit_ms=round(ti, 1),
                       tile_over_image=round(tt / ti, 3), tile_fit_samples=[round(t, 1) for t in times[run_tiles]],
                       image_fit_samples=[round(t, 1) for t in times[run_images]])
            rows.append(row)
            print(json.dumps(row), flush=True)
    h.close()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
