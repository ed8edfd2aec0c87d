"""Decode at reduced scale on one MI355X: pxz_expand_varied_scaled_frames_device at scales 0 to 3 against
pxz_expand_varied_frames_device, the only way to the pixels before it (a caller who wants 1/2^k of them still has to write them
all, and to down-size them by its own means afterwards: that second step is NOT in the baseline's time).  The seeded folder of
tools/varied_bench.py (256 RGBA images), shrunk mildly (shrink_by 1.0) and strongly (shrink_by 0.125) with Lanczos3, in 64x64
and in 32x32 tiles, written by the device writer, read by the unchanged reader, expanded with Lanczos3.  Device time from HIP
events, median (and every sample) of --reps runs; at scale 0 the two calls' outputs are compared byte for byte before anything
is timed.  The host forms (files in, pixels out, synchronous) are timed against their twins with the wall clock: the whole
folder through pxz_decode_varied_files_scaled / pxz_decode_varied_files, and one 224 x 224 window per file (aligned to 8)
through pxz_decode_windows_files_scaled / pxz_decode_windows_files.

    python tools/scaled_decode_bench.py [--reps 5] [--images 256] [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

SCALES = (0, 1, 2, 3)


def timed(torch, fn, reps):
    fn()  # warm-up (tables, scratch)
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return dict(ms=round(statistics.median(ts), 3), samples=[round(t, 3) for t in ts])


def walled(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return dict(ms=round(statistics.median(ts), 3), samples=[round(t, 3) for t in ts])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    import varied_bench as VB
    P = VB.P
    h = P.Handle(0)
    rows = []
    c, filt = 4, 4
    buf, geoms = VB.folder(args.images, 2026)
    sizes = [(g[0], g[1]) for g in geoms]
    mpx = sum(w * hh for (w, hh) in sizes) / 1e6

    def layout(k):
        out, at = [], 0
        for (w, hh) in sizes:
            sw, sh = -(-w // (1 << k)), -(-hh // (1 << k))
            out.append((w, hh, sw * c, at))
            at += (sw * sh * c + 255) & ~255
        return out, at

    for b in (64, 32):
        for what, factor in (("mild", 1.0), ("strong", 0.125)):
            _, vals, ow, oh, slots = h.shrink_varied_frames_device(buf, b, b, 0, 4, factor, descs=geoms, channels=c)
            fo, fbuf = h.encode_varied_frames_device(sizes, c, b, b, vals, ow, oh, slots)
            torch.cuda.synchronize()
            stored_mpx = float((ow.to(torch.int64) * oh.to(torch.int64)).sum().item()) / 1e6
            del vals, ow, oh, slots
            torch.cuda.empty_cache()
            _, dv, dw, dh, ds = h.decode_varied_frames_device(fbuf, fo, sizes, c, b, b)
            torch.cuda.synchronize()
            assert h.decode_status() == 0
            full, full_bytes = layout(0)
            whole = torch.empty(full_bytes, dtype=torch.uint8, device="cuda")
            base = timed(torch, lambda: h.expand_varied_frames_device(full, c, b, b, filt, dw, dh, ds, whole), args.reps)
            ref = whole.clone()
            for k in SCALES:
                descs, total = layout(k)
                out = torch.zeros(total, dtype=torch.uint8, device="cuda")
                call = lambda: h.expand_varied_scaled_frames_device(descs, c, b, b, filt, [k] * len(sizes), dw, dh, ds, out)  # noqa: E731
                call()
                torch.cuda.synchronize()
                assert h.decode_status() == 0
                row = dict(case=f"folder of {len(sizes)} files ({mpx:.1f} Mpx, {stored_mpx:.1f} Mpx stored), {what} shrink", tile=f"{b}x{b}", scale_log2=k,
                           out_mbytes=round(total / 1e6, 1), full_mbytes=round(full_bytes / 1e6, 1))
                if k == 0:
                    row["bit_exact"] = bool(torch.equal(out, ref))
                    if not row["bit_exact"]:
                        print(f"MISMATCH {what} {b}x{b}", flush=True)
                        sys.exit(1)
                row["expand_varied_frames_device"] = base
                row["expand_varied_scaled_frames_device"] = timed(torch, call, args.reps)
                rows.append(row)
                print(json.dumps(row), flush=True)
                del out
            # the host forms on the same files
            torch.cuda.synchronize()
            offs = fo.cpu().numpy()
            host = fbuf.cpu().numpy()
            files = [host[int(offs[i]):int(offs[i + 1])].tobytes() for i in range(len(sizes))]
            rng = np.random.default_rng(224)
            rects = []
            for i, (w, hh) in enumerate(sizes):
                ww, wh = min(224, w // 8 * 8), min(224, hh // 8 * 8)
                if ww == 0 or wh == 0:
                    ww, wh, x, y = w, hh, 0, 0
                else:
                    x, y = int(rng.integers(0, (w - ww) // 8 + 1)) * 8, int(rng.integers(0, (hh - wh) // 8 + 1)) * 8
                rects.append((i, x, y, ww, wh))
            twin = walled(lambda: h.decode_varied_files(files, c, b, b, filt, sizes=sizes), args.reps)
            twin_w = walled(lambda: h.decode_windows_files(files, rects, c, b, b, filt, sizes=sizes), args.reps)
            for k in SCALES:
                row = dict(case=f"host forms, {what} shrink", tile=f"{b}x{b}", scale_log2=k, decode_varied_files=twin, decode_windows_files=twin_w)
                row["decode_varied_files_scaled"] = walled(lambda: h.decode_varied_files_scaled(files, c, b, b, filt, [k] * len(files), sizes=sizes), args.reps)
                row["decode_windows_files_scaled"] = walled(
                    lambda: h.decode_windows_files_scaled(files, rects, c, b, b, filt, [k] * len(rects), sizes=sizes), args.reps)
                rows.append(row)
                print(json.dumps(row), flush=True)
            del fbuf, whole, ref, dv, dw, dh, ds
            torch.cuda.empty_cache()
    h.close()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
