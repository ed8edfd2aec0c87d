"""The decode side of varied batches on one MI355X: one pxz_decode_varied_frames_device / pxz_expand_varied_frames_device call
against a loop of pxz_decode_frames_device + pxz_expand_frames_device calls (one pair per file, one stream) over the seeded
folder of tools/varied_bench.py, whose files the varied encoder writes; the host form against per-file pxz_decode_file +
pxz_expand_image; an equal-geometry 8 x 8K batch against the single-geometry fast paths.  Every comparison is checked bit for
bit before it is timed.  Device time from HIP events, median (and every sample) of --reps runs.

    python tools/varied_decode_bench.py [--images 256] [--reps 5] [--host-images 32] [--json out.json]
    PXZ_LIB=<build of the parent commit> python tools/varied_decode_bench.py --loop-only --json parent.json
                                          the loop alone, from a library without the varied decode side (the baseline)
    python tools/varied_decode_bench.py --baseline parent.json ...
                                          also requires: reader and reader + expand rows faster than that loop by more than the
                                          spread of the repeats (exit status 1 otherwise)
    python tools/varied_decode_bench.py --trace-run N      one writer + reader + expand pass over N images and nothing else
                                          (under rocprofv3 --kernel-trace --stats: the launches do not grow with N)
    python tools/varied_decode_bench.py --compare-traces DIR_A DIR_B
                                          the project's kernels and their call counts in two such traces must agree
"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

ROWS = [  # (block, mode, factor, label)
    (64, 0, 1.0, "shrink_by 1.0"), (64, 1, 16.0, "directional 16.0"), (64, 0, 0.06, "shrink_by 0.06"),
    (32, 0, 1.0, "shrink_by 1.0"), (32, 1, 16.0, "directional 16.0"), (32, 0, 0.06, "shrink_by 0.06"),
]


def compare_traces(dir_a, dir_b):
    def counts(d):
        found = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        assert found, f"no kernel_stats.csv under {d}"
        out = {}
        for row in csv.DictReader(open(found[0])):
            name = row.get("Name") or row.get("KernelName") or ""
            if "pxz::" in name or name.startswith("pxz") or "_ZN3pxz" in name:
                out[name] = int(row.get("Calls") or row.get("Count") or 0)
        return out
    a, b = counts(dir_a), counts(dir_b)
    for name in sorted(set(a) | set(b)):
        print(f"{a.get(name, 0):4d} {b.get(name, 0):4d}  {name[:110]}")
    if a != b or not a:
        print("the traces list different project kernels or counts")
        return 1
    print(f"{len(a)} project kernels, the same number of launches in both traces")
    return 0


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
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-images", type=int, default=32)
    ap.add_argument("--json", default=None)
    ap.add_argument("--loop-only", action="store_true")
    ap.add_argument("--baseline", default=None)
    ap.add_argument("--trace-run", type=int, default=0)
    ap.add_argument("--compare-traces", nargs=2, default=None)
    args = ap.parse_args()
    if args.compare_traces:
        sys.exit(compare_traces(*args.compare_traces))

    import torch
    import varied_bench as VB
    P = VB.P
    lib = os.path.basename(os.environ.get("PXZ_LIB", "default"))
    h = P.Handle(0)

    if args.trace_run:
        buf, geoms = VB.folder(args.trace_run, 2026)
        sizes = [(g[0], g[1]) for g in geoms]
        _, vals, ow, oh, slots = h.shrink_varied_frames_device(buf, 64, 64, 1, 4, 16.0, descs=geoms, channels=4)
        fo, fbuf = h.encode_varied_frames_device(sizes, 4, 64, 64, vals, ow, oh, slots)
        _, v2, w2, h2, s2 = h.decode_varied_frames_device(fbuf, fo, sizes, 4, 64, 64)
        h.expand_varied_frames_device(geoms, 4, 64, 64, 4, w2, h2, s2, torch.empty_like(buf))
        torch.cuda.synchronize()
        assert h.decode_status() == 0 and torch.equal(w2, ow) and torch.equal(h2, oh)
        h.close()
        return

    buf, geoms = VB.folder(args.images, 2026)
    n = len(geoms)
    sizes = [(g[0], g[1]) for g in geoms]
    px = sum(w * hh for (w, hh) in sizes)
    print(f"{lib}: folder of {n} RGBA images, {px / 1e6:.1f} Mpx", flush=True)
    baseline = {}
    if args.baseline:
        for r in json.load(open(args.baseline)):
            if "loop_reader" in r:
                baseline[(r["tile"], r["files"])] = r
    rows, failed = [], False
    img_out = torch.empty_like(buf)
    img_loop = torch.empty_like(buf)
    for (b, mode, factor, label) in ROWS:
        offs = P.varied_layout(geoms, b, b)
        T = int(offs[-1])
        _, vals, ow, oh, slots = h.shrink_varied_frames_device(buf, b, b, mode, 4, factor, descs=geoms, channels=4)
        fo, fbuf = h.encode_varied_frames_device(sizes, 4, b, b, vals, ow, oh, slots)
        torch.cuda.synchronize()
        full_w = torch.tensor([g[0] for g in geoms], device="cuda")
        share_full = None
        distinct = len(set(zip(ow.cpu().numpy().tolist(), oh.cpu().numpy().tolist())))
        # the share of tiles stored at the full size of their place (edge tiles included): the oracle of "mostly copies"
        place_w = torch.empty(T, dtype=torch.int32, device="cuda")
        place_h = torch.empty(T, dtype=torch.int32, device="cuda")
        for i, (w, hh) in enumerate(sizes):
            a, e = int(offs[i]), int(offs[i + 1])
            cols, rws = P.grid(w, hh, b, b)
            pw = torch.full((rws, cols), b, dtype=torch.int32, device="cuda")
            ph = torch.full((rws, cols), b, dtype=torch.int32, device="cuda")
            pw[:, -1] = w - (cols - 1) * b
            ph[-1, :] = hh - (rws - 1) * b
            place_w[a:e], place_h[a:e] = pw.reshape(-1), ph.reshape(-1)
        share_full = float(((ow == place_w) & (oh == place_h)).float().mean())
        del full_w, place_w, place_h
        # outputs: the varied call's, and one set per file for the loop (views of one allocation each: no allocation is timed)
        dv = (torch.zeros(T, dtype=torch.float32, device="cuda"), torch.zeros(T, dtype=torch.int32, device="cuda"),
              torch.zeros(T, dtype=torch.int32, device="cuda"), torch.zeros((T, b * b * 4), dtype=torch.uint8, device="cuda"))
        dl = tuple(torch.zeros_like(x) for x in dv)
        singles, foffs, shapes, frames = [], [], [], []
        for i, (w, hh) in enumerate(sizes):
            a, e = int(offs[i]), int(offs[i + 1])
            singles.append(tuple(x[a:e][None] for x in dl))
            foffs.append(fo[i:i + 2])
            shapes.append((1, hh, w, 4))
            frames.append(VB.frame_of(img_loop, geoms[i]))
        have_varied = not args.loop_only

        def loop_reader():
            for i in range(n):
                h.decode_frames_device(fbuf, foffs[i], shapes[i], b, b, out=singles[i])

        def varied_reader():
            h.decode_varied_frames_device(fbuf, fo, sizes, 4, b, b, out=dv)

        def loop_expand(filt):
            for i in range(n):
                h.expand_frames_device(shapes[i], b, b, filt, singles[i][1], singles[i][2], singles[i][3], out=frames[i])

        def varied_expand(filt):
            h.expand_varied_frames_device(geoms, 4, b, b, filt, dv[1], dv[2], dv[3], img_out)

        loop_reader()
        torch.cuda.synchronize()
        ok = h.decode_status() == 0 and torch.equal(dl[1], ow) and torch.equal(dl[2], oh) and torch.equal(dl[0].view(torch.int32), vals.view(torch.int32))
        if have_varied:
            varied_reader()
            ok = ok and h.decode_status() == 0
            valid = torch.arange(b * b * 4, device="cuda").view(1, -1) < (ow * oh * 4).view(-1, 1)
            ok = ok and torch.equal(dv[1], dl[1]) and torch.equal(dv[2], dl[2]) and torch.equal(dv[0].view(torch.int32), dl[0].view(torch.int32))
            ok = ok and torch.equal(dv[3][valid], dl[3][valid]) and torch.equal(dv[3][valid], slots[valid])
            del valid
            for filt in (0, 4):
                img_out.zero_()
                img_loop.zero_()
                loop_expand(filt)
                varied_expand(filt)
                torch.cuda.synchronize()
                ok = ok and h.decode_status() == 0 and torch.equal(img_out, img_loop)
        if not ok:
            print(f"MISMATCH {b}x{b} {label}", flush=True)
            sys.exit(1)
        row = dict(lib=lib, tile=f"{b}x{b}", files=label, tiles=T, share_full=round(share_full, 4), distinct_sizes=distinct, bit_exact=ok)
        row["loop_reader"] = timed(torch, loop_reader, args.reps)
        row["loop_expand_nearest"] = timed(torch, lambda: loop_expand(0), args.reps)
        row["loop_expand_lanczos3"] = timed(torch, lambda: loop_expand(4), args.reps)
        row["loop_both_lanczos3"] = timed(torch, lambda: (loop_reader(), loop_expand(4)), args.reps)
        if have_varied:
            row["varied_reader"] = timed(torch, varied_reader, args.reps)
            row["varied_expand_nearest"] = timed(torch, lambda: varied_expand(0), args.reps)
            row["varied_expand_lanczos3"] = timed(torch, lambda: varied_expand(4), args.reps)
            row["varied_both_lanczos3"] = timed(torch, lambda: (varied_reader(), varied_expand(4)), args.reps)
            base = baseline.get((row["tile"], row["files"]))
            if base:
                for what in ("reader", "both_lanczos3"):
                    lo, va = base["loop_" + what], row["varied_" + what]
                    spread = max(max(lo["samples"]) - min(lo["samples"]), max(va["samples"]) - min(va["samples"]))
                    won = lo["ms"] - va["ms"] > spread
                    row["parent_loop_" + what] = lo
                    row[what + "_faster_than_parent_loop_by_more_than_spread"] = won
                    failed = failed or not won
        rows.append(row)
        print(json.dumps(row), flush=True)
        del dv, dl, singles, frames, fbuf, slots
        torch.cuda.empty_cache()

    if not args.loop_only:
        # host form: the first host-images files of the folder (64x64 blocks, shrink_by 1.0), wall clock
        k = min(args.host_images, n)
        imgs = [VB.frame_of(buf, g)[0].cpu().numpy() for g in geoms[:k]]
        files = h.encode_varied_images(imgs, 64, 64, 0, 4, 1.0)
        h.decode_varied_files(files, 4, 64, 64, 4)  # (warm-up)
        t0 = time.perf_counter()
        got, _ = h.decode_varied_files(files, 4, 64, 64, 4)
        t_varied = (time.perf_counter() - t0) * 1e3
        L = P.binding.load_library()
        import ctypes as C
        import numpy as np

        def per_file():
            out = []
            for f in files:
                w, hh, bw, bh, c, _ = P.file_header(f)
                cols, rws = P.grid(w, hh, bw, bh)
                raw = np.frombuffer(f, np.uint8)
                hdr = [C.c_uint32() for _ in range(6)]
                vals = np.zeros(cols * rws, np.float32)
                tw, th = np.zeros(cols * rws, np.uint32), np.zeros(cols * rws, np.uint32)
                sl = np.zeros((cols * rws, bw * bh * c), np.uint8)
                rc = L.pxz_decode_file(h._h, raw.ctypes.data, raw.size, *[C.byref(x) for x in hdr], vals.ctypes.data, tw.ctypes.data,
                                       th.ctypes.data, sl.ctypes.data)
                assert rc == 0
                out.append(h.expand_image(w, hh, c, bw, bh, 4, tw, th, sl))
            return out
        per_file()  # (warm-up)
        t0 = time.perf_counter()
        ref = per_file()
        t_loop = (time.perf_counter() - t0) * 1e3
        row = dict(host_form_files=k, decode_varied_files_ms=round(t_varied, 1), per_file_decode_file_and_expand_image_ms=round(t_loop, 1),
                   bit_exact=all((a == r).all() for a, r in zip(got, ref)))
        rows.append(row)
        print(json.dumps(row), flush=True)
        if not row["bit_exact"]:
            sys.exit(1)
    del buf, img_out, img_loop
    torch.cuda.empty_cache()

    if not args.loop_only:
        # equal geometry, for the record: 8 x 8K through the varied reader / expand against the single-geometry fast paths
        frames8 = h.synth_frames_device(8, 4320, 7680, 4, dist=P.DIST_OPAQUE)
        shape = tuple(frames8.shape)
        geo8 = [(7680, 4320, 7680 * 4, k * 7680 * 4320 * 4) for k in range(8)]
        size8 = [(7680, 4320)] * 8
        for b in (64, 32):
            vals, ow, oh, slots = h.shrink_frames_device(frames8, b, b, 1, 4, 16.0)
            fo, fbuf = h.encode_frames_device(shape, b, b, vals, ow, oh, slots)
            one = h.decode_frames_device(fbuf, fo, shape, b, b)
            res = h.decode_varied_frames_device(fbuf, fo, size8, 4, b, b)
            torch.cuda.synchronize()
            ok = torch.equal(res[2], one[1].reshape(-1)) and torch.equal(res[3], one[2].reshape(-1)) and torch.equal(res[2], ow.reshape(-1))
            back_f = torch.empty_like(frames8)
            back_v = torch.empty_like(frames8)
            row = dict(equal_geometry="8x7680x4320", tile=f"{b}x{b}", files="directional 16.0")
            row["frames_reader"] = timed(torch, lambda: h.decode_frames_device(fbuf, fo, shape, b, b, out=one), args.reps)
            row["varied_reader"] = timed(torch, lambda: h.decode_varied_frames_device(fbuf, fo, size8, 4, b, b, out=res[1:]), args.reps)
            for filt, name in ((0, "nearest"), (4, "lanczos3")):
                h.expand_frames_device(shape, b, b, filt, one[1], one[2], one[3], out=back_f)
                h.expand_varied_frames_device(geo8, 4, b, b, filt, res[2], res[3], res[4], back_v.reshape(-1))
                torch.cuda.synchronize()
                ok = ok and torch.equal(back_f, back_v)
                row["frames_expand_" + name] = timed(torch, lambda: h.expand_frames_device(shape, b, b, filt, one[1], one[2], one[3], out=back_f), args.reps)
                row["varied_expand_" + name] = timed(torch, lambda: h.expand_varied_frames_device(geo8, 4, b, b, filt, res[2], res[3], res[4], back_v.reshape(-1)), args.reps)
            row["bit_exact"] = ok
            rows.append(row)
            print(json.dumps(row), flush=True)
            if not ok:
                sys.exit(1)
            del vals, ow, oh, slots, fbuf, one, res, back_f, back_v
            torch.cuda.empty_cache()
    h.close()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)
    if failed:
        print("a required row is not faster than the parent's loop by more than the spread")
        sys.exit(1)


if __name__ == "__main__":
    main()
