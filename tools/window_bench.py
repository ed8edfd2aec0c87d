"""Pixel windows of files on one MI355X: pxz_decode_windows_device + pxz_expand_windows_device against what a caller had
before them -- pxz_decode_varied_frames_device + pxz_expand_varied_frames_device of the same files, whole, followed by a
device-side crop (a torch slice copy per window).  Device time from HIP events, median (and every sample) of --reps runs; the
crops of both sides are compared byte for byte before anything is timed.

  first case   one 16384 x 16384 RGBA frame (synthetic, opaque), shrink_by 0.5 with Lanczos3, written by the device writer, in
               32x32 and in 64x64 tiles; windows of 256^2, 1024^2, 4096^2 px at a tile-aligned and at an odd origin, and the
               whole image; expanded with Lanczos3.
  second case  the seeded folder of tools/varied_bench.py (the 256 files of tools/varied_decode_bench.py, shrink_by 1.0), one
               224 x 224 window per file (smaller where the image is) at a seeded origin.

    python tools/window_bench.py [--reps 5] [--images 256] [--side 16384] [--json out.json]
    PXZ_LIB=<build of the parent commit> python tools/window_bench.py ...
                                  the baseline rows alone, from a library without the window calls
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--side", type=int, default=16384)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    import varied_bench as VB
    P = VB.P
    lib = os.path.basename(os.environ.get("PXZ_LIB", "default"))
    have_windows = hasattr(P.load_library(), "pxz_window_layout")
    h = P.Handle(0)
    rows = []
    print(f"{lib}: window calls {'present' if have_windows else 'absent: baseline rows only'}", flush=True)

    def run_case(label, fbuf, fo, sizes, b, rects, filt):
        """rects: (image, x, y, w, h) per window -> one row: the whole-file calls + slice copies against the window calls"""
        c = 4
        geoms, at = [], 0
        for (w, hh) in sizes:
            geoms.append((w, hh, w * c, at))
            at += (w * hh * c + 255) & ~255
        whole = torch.empty(at, dtype=torch.uint8, device="cuda")
        T = int(P.varied_layout(geoms, b, b)[-1])
        dv = (torch.zeros(T, dtype=torch.float32, device="cuda"), torch.zeros(T, dtype=torch.int32, device="cuda"),
              torch.zeros(T, dtype=torch.int32, device="cuda"), torch.zeros((T, b * b * c), dtype=torch.uint8, device="cuda"))
        windows, wat = [], 0
        for (i, x, y, w, hh) in rects:
            windows.append((i, x, y, w, hh, w * c, wat))
            wat += (w * hh * c + 255) & ~255
        crops_a = torch.zeros(wat, dtype=torch.uint8, device="cuda")
        views = [(torch.as_strided(whole, (win[4], win[3], c), (geoms[win[0]][2], c, 1), geoms[win[0]][3] + win[2] * geoms[win[0]][2] + win[1] * c),
                  torch.as_strided(crops_a, (win[4], win[3], c), (win[5], c, 1), win[6])) for win in windows]

        def baseline():
            h.decode_varied_frames_device(fbuf, fo, sizes, c, b, b, out=dv)
            h.expand_varied_frames_device(geoms, c, b, b, filt, dv[1], dv[2], dv[3], whole)
            for src, dst in views:
                dst.copy_(src)

        baseline()
        torch.cuda.synchronize()
        assert h.decode_status() == 0
        row = dict(lib=lib, case=label, tile=f"{b}x{b}", windows=len(windows), window_px=sum(r[3] * r[4] for r in rects), file_tiles=T)
        if have_windows:
            Tw = int(P.window_layout(sizes, windows, b, b)[-1])
            dw = (torch.zeros(Tw, dtype=torch.float32, device="cuda"), torch.zeros(Tw, dtype=torch.int32, device="cuda"),
                  torch.zeros(Tw, dtype=torch.int32, device="cuda"), torch.zeros((Tw, b * b * c), dtype=torch.uint8, device="cuda"))
            crops_b = torch.zeros(wat, dtype=torch.uint8, device="cuda")

            def window_calls():
                h.decode_windows_device(fbuf, fo, sizes, windows, c, b, b, out=dw)
                h.expand_windows_device(sizes, windows, c, b, b, filt, dw[1], dw[2], dw[3], crops_b)

            window_calls()
            torch.cuda.synchronize()
            row["covered_tiles"] = Tw
            row["bit_exact"] = h.decode_status() == 0 and torch.equal(crops_a, crops_b)
            if not row["bit_exact"]:
                print(f"MISMATCH {label} {b}x{b}", flush=True)
                sys.exit(1)
        row["whole_files_then_crop"] = timed(torch, baseline, args.reps)
        if have_windows:
            row["window_calls"] = timed(torch, window_calls, args.reps)
            row["decode_windows_alone"] = timed(torch, lambda: h.decode_windows_device(fbuf, fo, sizes, windows, c, b, b, out=dw), args.reps)
        rows.append(row)
        print(json.dumps(row), flush=True)

    # ---- one large frame
    S = args.side
    frame = h.synth_frames_device(1, S, S, 4, dist=P.DIST_OPAQUE)
    for b in (32, 64):
        vals, ow, oh, slots = h.shrink_frames_device(frame, b, b, 0, 4, 0.5)
        fo, fbuf = h.encode_frames_device((1, S, S, 4), b, b, vals, ow, oh, slots)
        torch.cuda.synchronize()
        fbuf = fbuf[: int(fo[1])].clone()
        del vals, ow, oh, slots
        torch.cuda.empty_cache()
        for side in (256, 1024, 4096):
            if side >= S:
                continue
            for what, (x, y) in (("aligned", (S // 4, S // 4)), ("odd", (S // 4 + 3, S // 4 + 5))):
                run_case(f"{S}x{S} frame, {side}x{side} window at ({x}, {y}) [{what}]", fbuf, fo, [(S, S)], b, [(0, x, y, side, side)], 4)
        run_case(f"{S}x{S} frame, the whole image as one window", fbuf, fo, [(S, S)], b, [(0, 0, 0, S, S)], 4)
        del fbuf
        torch.cuda.empty_cache()
    del frame
    torch.cuda.empty_cache()

    # ---- a folder of differently sized files, one crop each
    buf, geoms = VB.folder(args.images, 2026)
    sizes = [(g[0], g[1]) for g in geoms]
    rng = np.random.default_rng(224)
    rects = []
    for i, (w, hh) in enumerate(sizes):
        ww, wh = min(224, w), min(224, hh)
        rects.append((i, int(rng.integers(0, w - ww + 1)), int(rng.integers(0, hh - wh + 1)), ww, wh))
    for b in (64, 32):
        _, vals, ow, oh, slots = h.shrink_varied_frames_device(buf, b, b, 0, 4, 1.0, descs=geoms, channels=4)
        fo, fbuf = h.encode_varied_frames_device(sizes, 4, b, b, vals, ow, oh, slots)
        torch.cuda.synchronize()
        del vals, ow, oh, slots
        torch.cuda.empty_cache()
        run_case(f"folder of {len(sizes)} files ({sum(w * hh for (w, hh) in sizes) / 1e6:.1f} Mpx), one 224x224 window each", fbuf, fo, sizes, b, rects, 4)
        del fbuf
        torch.cuda.empty_cache()
    h.close()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
