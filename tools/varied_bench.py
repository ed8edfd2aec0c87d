"""Varied batches on one MI355X: one pxz_shrink_varied_frames_device call against a loop of pxz_shrink_frames_device calls
(one per image, one stream), with and without the writer; the host form against per-image pxz_shrink_image +
pxz_encode_container; and an equal-geometry 8 x 8K batch against pxz_shrink_frames_device.  Every comparison is checked bit
for bit before it is timed.  Device time from HIP events, median of --reps runs.

    python tools/varied_bench.py [--images 256] [--reps 5] [--host-images 32] [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as G  # noqa: E402

P = G.load_product()


def folder(n, seed):
    """a seeded 'folder': RGBA images with sides 64 .. 4096 (log-uniform, mixed aspect ratios), gradients + noise, on the
    device, back to back in one buffer at 256-byte aligned offsets"""
    rng = np.random.default_rng(seed)
    sizes = [(int(round(2 ** rng.uniform(6, 12))), int(round(2 ** rng.uniform(6, 12)))) for _ in range(n)]
    # (shrink_directionally refuses 1-px edge tiles, as the reference panics on them: no side of 32 k + 1)
    sizes = [(w + (w % 32 == 1), h + (h % 32 == 1)) for (w, h) in sizes]
    g = torch.Generator(device="cuda").manual_seed(seed)
    offs, total = [], 0
    for (w, h) in sizes:
        offs.append(total)
        total += (w * h * 4 + 255) // 256 * 256
    buf = torch.empty(total, dtype=torch.uint8, device="cuda")
    for (w, h), o in zip(sizes, offs):
        yy = torch.arange(h, device="cuda").view(h, 1, 1)
        xx = torch.arange(w, device="cuda").view(1, w, 1)
        base = (xx * 3 + yy * 2 + torch.arange(4, device="cuda").view(1, 1, 4) * 40) % 256
        noise = torch.randint(0, 48, (h, w, 4), device="cuda", generator=g)
        img = ((base + noise) % 256).to(torch.uint8)
        img[..., 3] = 255
        buf[o:o + w * h * 4] = img.reshape(-1)
    return buf, [(w, h, w * 4, o) for (w, h), o in zip(sizes, offs)]


def frame_of(buf, geom):
    w, h, pitch, off = geom
    return torch.as_strided(buf, (1, h, w, 4), (pitch * h, pitch, 4, 1), off)


def timed(fn, reps):
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
    return statistics.median(ts)


def same(res, singles, offs, c):
    _, vals, ow, oh, slots = res
    for i, (sv, sw, sh, ss) in enumerate(singles):
        a, b = int(offs[i]), int(offs[i + 1])
        if not (torch.equal(vals[a:b].view(torch.int32), sv[0].view(torch.int32)) and torch.equal(ow[a:b], sw[0]) and torch.equal(oh[a:b], sh[0])):
            return False
        valid = torch.arange(ss.shape[2], device="cuda").view(1, -1) < (sw[0] * sh[0] * c).view(-1, 1)
        if not torch.equal(slots[a:b][valid], ss[0][valid]):
            return False
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-images", type=int, default=32)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    h = P.Handle(0)
    buf, geoms = folder(args.images, 2026)
    px = sum(g[0] * g[1] for g in geoms)
    rows = []
    print(f"folder: {len(geoms)} RGBA images, {px / 1e6:.1f} Mpx", flush=True)
    for (bw, bh) in ((64, 64), (32, 32)):
        offs = P.varied_layout(geoms, bw, bh)
        T = int(offs[-1])
        out = (torch.empty(T, dtype=torch.float32, device="cuda"), torch.empty(T, dtype=torch.int32, device="cuda"),
               torch.empty(T, dtype=torch.int32, device="cuda"), torch.empty((T, bw * bh * 4), dtype=torch.uint8, device="cuda"))
        singles = []
        for g in geoms:
            c_, r_ = P.grid(g[0], g[1], bw, bh)
            n = c_ * r_
            singles.append((torch.empty((1, n), dtype=torch.float32, device="cuda"), torch.empty((1, n), dtype=torch.int32, device="cuda"),
                            torch.empty((1, n), dtype=torch.int32, device="cuda"), torch.empty((1, n, bw * bh * 4), dtype=torch.uint8, device="cuda")))
        sizes = [(g[0], g[1]) for g in geoms]
        fcap = sum(26 + 4 * P.grid(w, hh, bw, bh)[1] for (w, hh) in sizes) + T * (41 + bw * bh * 5)
        fo = torch.empty(len(geoms) + 1, dtype=torch.int64, device="cuda")
        fbuf = torch.empty(fcap, dtype=torch.uint8, device="cuda")
        for filt, fname in ((4, "Lanczos3"), (2, "CatmullRom")):
            for mode, factor in ((0, 1.0), (1, 16.0)):
                def run_varied():
                    return h.shrink_varied_frames_device(buf, bw, bh, mode, filt, factor, descs=geoms, channels=4, out=out)

                def run_loop():
                    for g, o in zip(geoms, singles):
                        h.shrink_frames_device(frame_of(buf, g), bw, bh, mode, filt, factor, out=o)

                def run_varied_enc():
                    res = run_varied()
                    h.encode_varied_frames_device(sizes, 4, bw, bh, res[1], res[2], res[3], res[4], out=(fo, fbuf))

                def run_loop_enc():
                    run_loop()
                    for g, o in zip(geoms, singles):
                        h.encode_frames_device((1, g[1], g[0], 4), bw, bh, o[0], o[1], o[2], o[3])

                res = run_varied()
                run_loop()
                torch.cuda.synchronize()
                ok = same(res, singles, offs, 4)
                if not ok:
                    print(f"MISMATCH {bw}x{bh} {fname} mode {mode}", flush=True)
                    sys.exit(1)
                tv, tl = timed(run_varied, args.reps), timed(run_loop, args.reps)
                tve, tle = timed(run_varied_enc, args.reps), timed(run_loop_enc, args.reps)
                row = dict(tile=f"{bw}x{bh}", filter=fname, mode=mode, tiles=T, varied_ms=round(tv, 3), loop_ms=round(tl, 3),
                           varied_enc_ms=round(tve, 3), loop_enc_ms=round(tle, 3), bit_exact=ok)
                rows.append(row)
                print(json.dumps(row), flush=True)
        del out, singles, fbuf
        torch.cuda.empty_cache()
    # host form: the first host-images images of the folder
    k = min(args.host_images, len(geoms))
    imgs = [frame_of(buf, g)[0].cpu().numpy() for g in geoms[:k]]
    files = h.encode_varied_images(imgs, 64, 64, 0, 4, 1.0)  # (warm-up)
    t0 = time.perf_counter()
    files = h.encode_varied_images(imgs, 64, 64, 0, 4, 1.0)
    t_host_varied = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    ref = []
    for img in imgs:
        vals, ow, oh, slots = h.shrink_image(img, 64, 64, 0, 4, 1.0)
        ref.append(P.encode_container(img.shape[1], img.shape[0], 64, 64, 4, 0, vals, None, ow, oh, slots))
    t_host_loop = (time.perf_counter() - t0) * 1e3
    row = dict(host_form_images=k, varied_images_ms=round(t_host_varied, 1), per_image_shrink_image_and_container_ms=round(t_host_loop, 1),
               bit_exact=all(r == f for r, f in zip(ref, files)))
    rows.append(row)
    print(json.dumps(row), flush=True)
    del buf
    torch.cuda.empty_cache()
    # equal geometry: 8 x 8K
    frames = h.synth_frames_device(8, 4320, 7680, 4, dist=P.DIST_OPAQUE)
    fb = frames.reshape(-1)
    geo8 = [(7680, 4320, 7680 * 4, k * 7680 * 4320 * 4) for k in range(8)]
    for (bw, bh) in ((64, 64), (32, 32)):
        offs = P.varied_layout(geo8, bw, bh)
        T = int(offs[-1])
        out = (torch.empty(T, dtype=torch.float32, device="cuda"), torch.empty(T, dtype=torch.int32, device="cuda"),
               torch.empty(T, dtype=torch.int32, device="cuda"), torch.empty((T, bw * bh * 4), dtype=torch.uint8, device="cuda"))
        n = T // 8
        one = (torch.empty((8, n), dtype=torch.float32, device="cuda"), torch.empty((8, n), dtype=torch.int32, device="cuda"),
               torch.empty((8, n), dtype=torch.int32, device="cuda"), torch.empty((8, n, bw * bh * 4), dtype=torch.uint8, device="cuda"))
        for mode, factor in ((0, 1.0), (1, 16.0)):
            res = h.shrink_varied_frames_device(fb, bw, bh, mode, 4, factor, descs=geo8, channels=4, out=out)
            h.shrink_frames_device(frames, bw, bh, mode, 4, factor, out=one)
            torch.cuda.synchronize()
            ok = same(res, [tuple(x[f:f + 1] for x in one) for f in range(8)], offs, 4)
            if not ok:
                print(f"MISMATCH 8x8K {bw}x{bh} mode {mode}", flush=True)
                sys.exit(1)
            tv = timed(lambda: h.shrink_varied_frames_device(fb, bw, bh, mode, 4, factor, descs=geo8, channels=4, out=out), args.reps)
            tf = timed(lambda: h.shrink_frames_device(frames, bw, bh, mode, 4, factor, out=one), args.reps)
            row = dict(equal_geometry="8x7680x4320", tile=f"{bw}x{bh}", filter="Lanczos3", mode=mode, varied_ms=round(tv, 3),
                       frames_call_ms=round(tf, 3), bit_exact=ok)
            rows.append(row)
            print(json.dumps(row), flush=True)
        del out, one
        torch.cuda.empty_cache()
    h.close()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
