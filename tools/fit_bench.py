"""Fit to a budget on one MI355X: one pxz_encode_varied_images_fit call against what a caller does today on the same build --
pxz_rate_distortion_varied_images, pxz_fit_select on the host, and one pxz_encode_varied_images per distinct chosen factor over
the images that chose it -- on the folder of tools/varied_bench.py (256 RGBA images, sides 64 .. 4096 log-uniform) at the
reference's 20 factors (whole-folder.rs:83-88: k = i / 20; times 16 for shrink_directionally); 64x64 and 32x32 blocks, both
modes, both criteria, Lanczos3 down and CatmullRom up.  The targets are each image's median file length (FIT_BYTES) or median
error (FIT_SSE), so the choices spread over the rungs.  Both ways are checked byte for byte against each other before anything
is timed.  Host forms are synchronous: wall time around the calls, the two flows alternating, every sample of a row reported.
The fit runs the writer a second time, over the chosen rungs (about 1/K of its first run); this is where that cost shows.
Before the host forms, the two new device calls alone on the folder's tiles in HBM (device_steps below; --device-only stops there).

    python tools/fit_bench.py [--images 256] [--reps 3] [--device-only] [--json out.json]
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


def device_steps(h, buf, geoms, reps):
    """the two new kernels alone, on tiles already in HBM: ladder, writer offsets and distortion once, then pxz_fit_varied_ladder_device
    and pxz_gather_varied_rungs_device timed by events on the handle's stream (one warm-up, then reps samples each).  The gather is
    checked against slices of the rungs first; its traffic is what the algorithm needs -- every valid byte read once and written
    once, 12 bytes of value and sizes per tile each way -- over the kernel's time, against 8 TB/s."""
    import torch
    n, rows = len(geoms), []
    stream = torch.cuda.current_stream()
    for block in (64, 32):
        for mode in (0, 1):
            factors = [k * (16.0 if mode == 1 else 1.0) for k in SWEEP]
            K, slot = len(factors), block * block * 4
            offs, vals, ow, oh, slots = h.shrink_varied_ladder_frames_device(buf, block, block, mode, DOWN, factors, descs=geoms, channels=4)
            T = int(offs[-1])
            flat = (vals.reshape(-1), ow.reshape(-1), oh.reshape(-1), slots.reshape(K * T, slot))
            foffs = torch.empty(K * n + 1, dtype=torch.int64, device="cuda")
            h.encode_varied_frames_device([(g[0], g[1]) for g in geoms] * K, 4, block, block, *flat,
                                          out=(foffs, torch.empty(256, dtype=torch.uint8, device="cuda")))  # (no room: its offsets are wanted)
            _, sse = h.distortion_varied_frames_device(buf, block, block, UP, flat[1], flat[2], flat[3], descs=list(geoms) * K, channels=4,
                                                       want_tiles=False)
            sse = sse.reshape(K, n, 4)
            file_bytes = (foffs[1:] - foffs[:-1]).reshape(K, n)
            targets = torch.sort(file_bytes, dim=0)[0][K // 2].cpu().tolist()
            choice, flags = h.fit_varied_ladder_device(foffs, sse, P.FIT_BYTES, targets)
            out = h.gather_varied_rungs_device([(g[0], g[1]) for g in geoms], 4, block, block, K, choice, vals, ow, oh, slots)
            torch.cuda.synchronize()
            h_choice, h_flags = P.fit_select(file_bytes.cpu().numpy().astype(np.uint64), sse.cpu().numpy().astype(np.uint64), P.FIT_BYTES, targets)
            owner = torch.repeat_interleave(torch.arange(n, device="cuda"), torch.from_numpy(np.diff(offs.astype(np.int64))).cuda())
            src = choice.long()[owner] * T + torch.arange(T, device="cuda")
            ok = (choice.cpu().numpy().astype(np.uint32) == h_choice).all() and (flags.cpu().numpy().astype(np.uint32) == h_flags).all()
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

            t_fit = timed(lambda: h.fit_varied_ladder_device(foffs, sse, P.FIT_BYTES, targets, out=(choice, flags)))
            t_gather = timed(lambda: h.gather_varied_rungs_device([(g[0], g[1]) for g in geoms], 4, block, block, K, choice, vals, ow, oh,
                                                                  slots, out=out))
            moved = 2 * (valid_bytes + 12 * T)
            tg = statistics.median(t_gather)
            row = dict(device_steps=True, block=f"{block}x{block}", mode=mode, images=n, K=K, tiles=T, gathered_valid_bytes=valid_bytes,
                       fit_ms=round(statistics.median(t_fit), 4), gather_ms=round(tg, 4), gather_gbps=round(moved / tg / 1e6, 1),
                       gather_frac_of_8000_gbps=round(moved / tg / 1e6 / 8000.0, 3), exact=True,
                       note="call time by events: the launch with its host-side planning and the table's upload, not the kernel alone",
                       fit_samples=[round(t, 4) for t in t_fit], gather_samples=[round(t, 4) for t in t_gather])
            rows.append(row)
            print(json.dumps(row), flush=True)
            del vals, ow, oh, slots, flat, out
            torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--json", default=None)
    ap.add_argument("--device-only", action="store_true", help="only the two kernels on device-resident tiles")
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
            for criterion in (P.FIT_BYTES, P.FIT_SSE):
                q = file_bytes if criterion == P.FIT_BYTES else sse.sum(axis=2)
                targets = [int(np.sort(q[:, i])[len(factors) // 2]) for i in range(n)]

                def run_fit():
                    return h.encode_varied_images_fit(imgs, block, block, mode, DOWN, UP, factors, criterion, targets)

                def run_today():
                    fb, ss = h.rate_distortion_varied_images(imgs, block, block, mode, DOWN, UP, factors)
                    choice, flags = P.fit_select(fb, ss, criterion, targets)
                    files = [None] * n
                    for r in sorted(set(choice.tolist())):
                        who = [i for i in range(n) if choice[i] == r]
                        for i, f in zip(who, h.encode_varied_images([imgs[i] for i in who], block, block, mode, DOWN, factors[r])):
                            files[i] = f
                    return files, choice, flags

                got, exp = run_fit(), run_today()
                if got[0] != exp[0] or not (got[1] == exp[1]).all() or not (got[2] == exp[2]).all():
                    print(f"MISMATCH {block}x{block} mode {mode} criterion {criterion}", flush=True)
                    sys.exit(1)
                flows = [run_fit, run_today]
                times = {f: [] for f in flows}
                for i in range(args.reps):
                    for f in (flows if i % 2 == 0 else flows[::-1]):
                        t0 = time.perf_counter()
                        f()
                        times[f].append((time.perf_counter() - t0) * 1e3)
                tf, tt = statistics.median(times[run_fit]), statistics.median(times[run_today])
                row = dict(block=f"{block}x{block}", mode=mode, criterion="bytes" if criterion == P.FIT_BYTES else "sse", images=n, K=len(factors),
                           distinct_choices=len(set(got[1].tolist())), flagged=int(got[2].sum()), files_bytes=sum(len(f) for f in got[0]),
                           fit_ms=round(tf, 1), today_ms=round(tt, 1), speedup=round(tt / tf, 3), byte_exact=True,
                           fit_samples=[round(t, 1) for t in times[run_fit]], today_samples=[round(t, 1) for t in times[run_today]])
                rows.append(row)
                print(json.dumps(row), flush=True)
    h.close()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
