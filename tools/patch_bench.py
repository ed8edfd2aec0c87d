"""Patching pixel windows into .pixlzr files on one MI355X: the device chain pxz_decode_windows_device -> pxz_patch_windows_device
(in place) -> pxz_splice_windows_device, and the host form pxz_patch_windows_files, against what a caller had before them, built
only from calls of the commit before:

  today, device   pxz_decode_varied_frames_device of the WHOLE files, a gather of the covered tiles, pxz_expand_windows_device of
                  the hulls, the overlay, pxz_shrink_varied_frames_device of the hulls, the new tiles copied back into the batch,
                  pxz_encode_varied_frames_device of the WHOLE files.  The same operation: its files are compared with the
                  chain's byte for byte before anything is timed.
  today, host     pxz_decode_varied_files, the overlay in numpy, pxz_encode_varied_images.  NOT the same operation: it shrinks
                  every tile of every file a second time and changes tiles nobody edited; the row says so.

Device time from HIP events, host forms by the wall clock; median (and every sample) of --reps runs.

  first case   one --side x --side RGBA frame (synthetic, opaque), shrink_by 0.5 with Lanczos3, written by the device writer, in
               32x32 and in 64x64 tiles; windows of 64^2, 512^2, 4096^2 px at an odd origin, patched in both modes.
  second case  the seeded folder of tools/varied_bench.py, one 224 x 224 window per file (smaller where the image is).

    python tools/patch_bench.py [--reps 5] [--images 256] [--side 16384] [--host-frame] [--json out.json]
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

MODES = ((0, 0.5, "shrink_by 0.5"), (1, 8.0, "shrink_directionally 8.0"))


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
    return dict(ms=round(statistics.median(ts), 1), samples=[round(t, 1) for t in ts])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--side", type=int, default=16384)
    ap.add_argument("--host-frame", action="store_true", help="time the host forms on the large frame too (gigabytes over the bus)")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    import varied_bench as VB
    P = VB.P
    h = P.Handle(0)
    rows = []
    c = 4

    def run_case(label, fbuf, fo, sizes, b, rects, patches, host):
        """rects: (image, x, y, w, h) per window; patches: their new pixels, CUDA tensors [h, w, 4] -> one row per mode"""
        n = len(sizes)
        geoms, at = [], 0
        for (w, hh) in sizes:
            geoms.append((w, hh, w * c, at))
            at += (w * hh * c + 255) & ~255
        vo = P.varied_layout(geoms, b, b)
        T = int(vo[-1])
        plain = [(i, x, y, w, hh, 0, 0) for (i, x, y, w, hh) in rects]
        wo = P.patch_check(sizes, plain, b, b)
        Tw = int(wo[-1])
        # the patches in one buffer; the hulls as windows of a packed image and as a varied batch; the covered tiles' numbers
        pwin, pat = [], 0
        hulls, hdescs, hat, idx = [], [], 0, []
        for (i, x, y, w, hh) in rects:
            pwin.append((i, x, y, w, hh, w * c, pat))
            pat += (w * hh * c + 255) & ~255
            c0, r0 = x // b, y // b
            cc, cr = (x + w - 1) // b - c0 + 1, (y + hh - 1) // b - r0 + 1
            hx, hy = c0 * b, r0 * b
            hw, hhh = min((c0 + cc) * b, sizes[i][0]) - hx, min((r0 + cr) * b, sizes[i][1]) - hy
            hulls.append((i, hx, hy, hw, hhh, hw * c, hat))
            hdescs.append((hw, hhh, hw * c, hat))
            hat += (hw * hhh * c + 255) & ~255
            cols = -(-sizes[i][0] // b)
            idx += [int(vo[i]) + (r0 + j) * cols + c0 + k for j in range(cr) for k in range(cc)]
        patch = torch.zeros(max(pat, 1), dtype=torch.uint8, device="cuda")
        pviews = []
        for (i, x, y, w, hh, pitch, off), px in zip(pwin, patches):
            torch.as_strided(patch, (hh, w, c), (pitch, c, 1), off).copy_(px)
        himg = torch.zeros(hat, dtype=torch.uint8, device="cuda")
        for (i, x, y, w, hh), (_, hx, hy, hw, hhh, hp, hoff), (_, _, _, _, _, pp, poff) in zip(rects, hulls, pwin):
            pviews.append((torch.as_strided(patch, (hh, w, c), (pp, c, 1), poff),
                           torch.as_strided(himg, (hh, w, c), (hp, c, 1), hoff + (y - hy) * hp + (x - hx) * c)))
        idx = torch.tensor(idx, dtype=torch.int64, device="cuda")

        def tiles(count):
            return (torch.zeros(count, dtype=torch.float32, device="cuda"), torch.zeros(count, dtype=torch.int32, device="cuda"),
                    torch.zeros(count, dtype=torch.int32, device="cuda"), torch.zeros((count, b * b * c), dtype=torch.uint8, device="cuda"))
        dv, cov, hout, dw = tiles(T), tiles(Tw), tiles(Tw), tiles(Tw)
        rf = torch.zeros(len(rects), dtype=torch.int32, device="cuda")
        pf = torch.zeros(len(rects), dtype=torch.int32, device="cuda")
        room = fbuf.numel() + Tw * (13 + 14 + b * b * (c + 1) + 8)
        new = (torch.zeros(n + 1, dtype=torch.int64, device="cuda"), torch.empty(room, dtype=torch.uint8, device="cuda"))
        old = (torch.zeros(n + 1, dtype=torch.int64, device="cuda"), torch.empty(room, dtype=torch.uint8, device="cuda"))
        for mode, factor, mode_name in MODES:
            def chain():
                h.decode_windows_device(fbuf, fo, sizes, plain, c, b, b, out=dw, window_flags=rf)
                h.patch_windows_device(sizes, pwin, c, b, b, mode, 4, factor, 4, patch, dw[1], dw[2], dw[3], out=dw, window_flags=pf)
                h.splice_windows_device(fbuf, fo, sizes, plain, c, b, b, *dw, reader_flags=rf, patch_flags=pf, out=new)

            def today():
                h.decode_varied_frames_device(fbuf, fo, sizes, c, b, b, out=dv)
                for q in (1, 2, 3):
                    torch.index_select(dv[q], 0, idx, out=cov[q])
                h.expand_windows_device(sizes, hulls, c, b, b, 4, cov[1], cov[2], cov[3], himg)
                for src, dst in pviews:
                    dst.copy_(src)
                h.shrink_varied_frames_device(himg, b, b, mode, 4, factor, descs=hdescs, channels=c, out=hout)
                for q in range(4):
                    dv[q].index_copy_(0, idx, hout[q])
                h.encode_varied_frames_device(sizes, c, b, b, *dv, out=old)

            chain()
            today()
            torch.cuda.synchronize()
            total = int(new[0][-1])
            same = bool(int(rf.sum()) == 0 and int(pf.sum()) == 0 and torch.equal(new[0], old[0]) and torch.equal(new[1][:total], old[1][:total]))
            row = dict(case=label, tile=f"{b}x{b}", mode=mode_name, windows=len(rects), window_px=sum(r[3] * r[4] for r in rects), file_tiles=T,
                       covered_tiles=Tw, old_bytes=int(fo[-1]), new_bytes=total, same_files=same)
            if not same:
                print(f"MISMATCH {label} {b}x{b} {mode_name}", flush=True)
                sys.exit(1)
            row["device_chain"] = timed(torch, chain, args.reps)
            row["device_today"] = timed(torch, today, args.reps)
            row["device_ratio_today_over_chain"] = round(row["device_today"]["ms"] / row["device_chain"]["ms"], 2)
            if host:
                fo_h = fo.cpu().numpy()
                raw = fbuf.cpu().numpy()
                files = [raw[int(fo_h[i]):int(fo_h[i + 1])].tobytes() for i in range(n)]
                hp = [px.cpu().numpy() for px in patches]

                room_h = np.empty(room, np.uint8)  # (given room the form runs once; without it the binding asks for the size first)

                def host_form():
                    return h.patch_windows_files(files, rects, hp, b, b, mode, 4, factor, 4, out=room_h)

                def host_today():
                    imgs, _ = h.decode_varied_files(files, c, b, b, 4)
                    for (i, x, y, w, hh), px in zip(rects, hp):
                        imgs[i][y:y + hh, x:x + w] = px
                    return h.encode_varied_images(imgs, b, b, mode, 4, factor)

                got = host_form()
                row["host_form_same_files"] = b"".join(got) == new[1][:total].cpu().numpy().tobytes()
                row["host_form"] = walled(host_form, args.reps)
                row["host_today_reshrinks_every_tile"] = walled(host_today, args.reps)
                row["host_today_note"] = "not the same operation: every tile of every file is shrunk a second time"
            rows.append(row)
            print(json.dumps(row), flush=True)

    # ---- one large frame
    S = args.side
    frame = h.synth_frames_device(1, max(S, 64), max(S, 64), 4, dist=P.DIST_OPAQUE)
    for b in (32, 64) if S > 0 else ():  # (--side 0: the folder alone)
        vals, ow, oh, slots = h.shrink_frames_device(frame, b, b, 0, 4, 0.5)
        fo, fbuf = h.encode_frames_device((1, S, S, 4), b, b, vals, ow, oh, slots)
        torch.cuda.synchronize()
        fbuf = fbuf[: int(fo[1])].clone()
        del vals, ow, oh, slots
        torch.cuda.empty_cache()
        for side in (64, 512, 4096):
            if side + S // 4 + 1003 >= S:
                continue
            x, y = S // 4 + 3, S // 4 + 5
            px = frame[0, y + 700:y + 700 + side, x + 1000:x + 1000 + side].contiguous()  # other pixels of the same frame
            run_case(f"{S}x{S} frame, {side}x{side} window at ({x}, {y})", fbuf, fo, [(S, S)], b, [(0, x, y, side, side)], [px], args.host_frame)
        del fbuf
        torch.cuda.empty_cache()
    del frame
    torch.cuda.empty_cache()

    # ---- a folder of differently sized files, one window each
    buf, geoms = VB.folder(args.images, 2026)
    sizes = [(g[0], g[1]) for g in geoms]
    rng = np.random.default_rng(224)
    rects, patches = [], []
    for i, (w, hh) in enumerate(sizes):
        ww, wh = min(224, w), min(224, hh)
        x, y = int(rng.integers(0, w - ww + 1)), int(rng.integers(0, hh - wh + 1))
        rects.append((i, x, y, ww, wh))
        img = torch.as_strided(buf, (hh, w, c), (geoms[i][2], c, 1), geoms[i][3])
        patches.append(torch.flip(img[hh - wh:, w - ww:], (0, 1)).contiguous())  # the image's own last pixels, mirrored
    for b in (64, 32):
        _, vals, ow, oh, slots = h.shrink_varied_frames_device(buf, b, b, 0, 4, 1.0, descs=geoms, channels=4)
        fo, fbuf = h.encode_varied_frames_device(sizes, 4, b, b, vals, ow, oh, slots)
        torch.cuda.synchronize()
        fbuf = fbuf[: int(fo[-1])].clone()
        del vals, ow, oh, slots
        torch.cuda.empty_cache()
        run_case(f"folder of {len(sizes)} files ({sum(w * hh for (w, hh) in sizes) / 1e6:.1f} Mpx), one 224x224 window each", fbuf, fo, sizes, b, rects,
                 patches, True)
        del fbuf
        torch.cuda.empty_cache()
    h.close()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
