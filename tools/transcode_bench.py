"""Re-shrinking .pixlzr tiles on one MI355X (the reference CLI's pix_to_pix for a folder): pxz_reshrink_varied_frames_device
against the calls that were there before it, pxz_expand_varied_frames_device + pxz_shrink_varied_frames_device, from the same
decoded tiles; and files -> files -- reader, re-shrink in place, writer -- against the four chained device calls reader, expand,
shrink, writer.  The folder is tools/varied_bench.py's (256 RGBA images of 64-4096 px); it is first shrunk at factor f, then
re-shrunk at f / 2 (shrink_by 2.0 -> 1.0, shrink_directionally 32 -> 16), 64x64 and 32x32 tiles, Lanczos3 on both sides.

Both sides of a comparison run in this one process, alternating, after bench.py's warm-up (>= 60 ms of untimed load, then W
steps); device time from HIP events, median and every sample of --reps runs.  Every comparison is checked bit for bit before it
is timed.  The bytes of the image batch that the chained calls need and the re-shrink does not are printed beside the times: a
fact of the calls' signatures, not a measurement.  Each timed step runs under a limit of its own (--step-limit seconds): a step
that exceeds it ends the process with status 124, and nothing else is started.

    python tools/transcode_bench.py [--images 256] [--reps 9] [--warmup 5] [--host-images 32] [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

CONFIGS = [  # (block, mode, factor of the files, factor of the re-shrink, label)
    (64, 0, 2.0, 1.0, "shrink_by 2.0 -> 1.0"), (64, 1, 32.0, 16.0, "directional 32 -> 16"),
    (32, 0, 2.0, 1.0, "shrink_by 2.0 -> 1.0"), (32, 1, 32.0, 16.0, "directional 32 -> 16"),
    # the folder's images keep nearly every tile full at the factors above (the clone-in case); strongly shrunk files, whose
    # tiles are expanded before they are measured, for the record
    (64, 0, 0.12, 0.06, "shrink_by 0.12 -> 0.06"), (64, 1, 2.0, 1.0, "directional 2 -> 1"),
    (32, 0, 0.12, 0.06, "shrink_by 0.12 -> 0.06"), (32, 1, 2.0, 1.0, "directional 2 -> 1"),
]
FILTER = 4  # Lanczos3


class StepLimit:
    """a step that has not finished after `seconds` ends the process (status 124): a hung device call cannot be interrupted"""

    def __init__(self, seconds, what):
        self.timer = threading.Timer(seconds, self.expired)
        self.timer.daemon = True
        self.what = what

    def expired(self):
        print(f"step limit exceeded: {self.what}", flush=True)
        os._exit(124)

    def __enter__(self):
        self.timer.start()

    def __exit__(self, *exc):
        self.timer.cancel()


def compare(torch, a, b, warmup, reps, limit, what):
    """a and b alternating: >= 60 ms of untimed load and `warmup` steps of each, then `reps` timed steps of each"""
    def one(fn):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e)
    with StepLimit(limit, what + " (warm-up)"):
        t0 = time.perf_counter()
        while (time.perf_counter() - t0) * 1e3 < 60.0:
            a()
            b()
            torch.cuda.synchronize()
        for _ in range(warmup):
            a()
            b()
        torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(reps):
        with StepLimit(limit, what):
            ta.append(one(a))
            tb.append(one(b))
    return (dict(ms=round(statistics.median(ta), 3), samples=[round(t, 3) for t in ta]),
            dict(ms=round(statistics.median(tb), 3), samples=[round(t, 3) for t in tb]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-images", type=int, default=32)
    ap.add_argument("--step-limit", type=float, default=120.0)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()

    import torch
    import varied_bench as VB
    P = VB.P
    assert torch.cuda.is_available(), "this tool measures on the MI355X; there is nothing to report without one"
    h = P.Handle(0)
    buf, geoms = VB.folder(args.images, 2026)
    n = len(geoms)
    sizes = [(g[0], g[1]) for g in geoms]
    px = sum(w * hh for (w, hh) in sizes)
    image_batch_bytes = int(buf.numel())
    print(f"folder of {n} RGBA images, {px / 1e6:.1f} Mpx; image batch of the chained calls: {image_batch_bytes} bytes", flush=True)
    img = torch.empty_like(buf)  # what expand-varied writes and shrink-varied reads back: the re-shrink allocates none of it
    rows = []
    for (b, mode, f1, f2, label) in CONFIGS:
        T = int(P.varied_layout(geoms, b, b)[-1])
        _, vals, tw, th, slots = h.shrink_varied_frames_device(buf, b, b, mode, FILTER, f1, descs=geoms, channels=4)
        fo, fbuf = h.encode_varied_frames_device(sizes, 4, b, b, vals, tw, th, slots)
        torch.cuda.synchronize()
        file_bytes = int(fo[-1])

        def outputs():
            return (torch.empty(T, dtype=torch.float32, device="cuda"), torch.empty(T, dtype=torch.int32, device="cuda"),
                    torch.empty(T, dtype=torch.int32, device="cuda"), torch.empty((T, b * b * 4), dtype=torch.uint8, device="cuda"))
        out_a, out_b, dec_a, dec_b = outputs(), outputs(), outputs(), outputs()
        wr_a = (torch.empty_like(fo), torch.empty_like(fbuf))
        wr_b = (torch.empty_like(fo), torch.empty_like(fbuf))

        def reshrink():
            h.reshrink_varied_frames_device(sizes, 4, b, b, mode, FILTER, f2, FILTER, tw, th, slots, out=out_a)

        def expand_shrink():
            h.expand_varied_frames_device(geoms, 4, b, b, FILTER, tw, th, slots, img)
            h.shrink_varied_frames_device(img, b, b, mode, FILTER, f2, descs=geoms, channels=4, out=out_b)

        def files_reshrink():
            h.decode_varied_frames_device(fbuf, fo, sizes, 4, b, b, out=dec_a)
            h.reshrink_varied_frames_device(sizes, 4, b, b, mode, FILTER, f2, FILTER, dec_a[1], dec_a[2], dec_a[3], out=dec_a)
            h.encode_varied_frames_device(sizes, 4, b, b, dec_a[0], dec_a[1], dec_a[2], dec_a[3], out=wr_a)

        def files_chained():
            h.decode_varied_frames_device(fbuf, fo, sizes, 4, b, b, out=dec_b)
            h.expand_varied_frames_device(geoms, 4, b, b, FILTER, dec_b[1], dec_b[2], dec_b[3], img)
            h.shrink_varied_frames_device(img, b, b, mode, FILTER, f2, descs=geoms, channels=4, out=out_b)
            h.encode_varied_frames_device(sizes, 4, b, b, out_b[0], out_b[1], out_b[2], out_b[3], out=wr_b)

        # bit for bit before anything is timed
        with StepLimit(args.step_limit, f"{b}x{b} {label}: check"):
            reshrink()
            expand_shrink()
            torch.cuda.synchronize()
            ok = h.decode_status() == 0
            ok = ok and torch.equal(out_a[0].view(torch.int32), out_b[0].view(torch.int32)) and torch.equal(out_a[1], out_b[1]) and torch.equal(out_a[2], out_b[2])
            valid = torch.arange(b * b * 4, device="cuda").view(1, -1) < (out_b[1] * out_b[2] * 4).view(-1, 1)
            ok = ok and torch.equal(out_a[3][valid], out_b[3][valid])
            del valid
            files_reshrink()
            files_chained()
            torch.cuda.synchronize()
            ok = ok and torch.equal(wr_a[0], wr_b[0]) and int(wr_a[0][-1]) <= wr_a[1].numel()
            end = int(wr_b[0][-1])
            ok = ok and torch.equal(wr_a[1][:end], wr_b[1][:end])
        if not ok:
            print(f"MISMATCH {b}x{b} {label}", flush=True)
            sys.exit(1)
        place = torch.tensor([min(b, w - x) * min(b, hh - y) for (w, hh) in sizes for y in range(0, hh, b) for x in range(0, w, b)], device="cuda")
        row = dict(tile=f"{b}x{b}", files=label, tiles=T, file_bytes=file_bytes, image_batch_bytes=image_batch_bytes, bit_exact=ok,
                   share_stored_full=round(float((tw * th == place).float().mean()), 4),
                   share_full_after=round(float((out_a[1] * out_a[2] == place).float().mean()), 4))
        del place
        row["reshrink"], row["expand_plus_shrink"] = compare(torch, reshrink, expand_shrink, args.warmup, args.reps, args.step_limit,
                                                             f"{b}x{b} {label}: tiles -> tiles")
        row["files_reader_reshrink_writer"], row["files_reader_expand_shrink_writer"] = compare(
            torch, files_reshrink, files_chained, args.warmup, args.reps, args.step_limit, f"{b}x{b} {label}: files -> files")
        row["reshrink_not_slower"] = row["reshrink"]["ms"] <= row["expand_plus_shrink"]["ms"]
        row["files_not_slower"] = row["files_reader_reshrink_writer"]["ms"] <= row["files_reader_expand_shrink_writer"]["ms"]
        rows.append(row)
        print(json.dumps(row), flush=True)
        del out_a, out_b, dec_a, dec_b, wr_a, wr_b, vals, tw, th, slots, fbuf
        torch.cuda.empty_cache()

    # host form, wall clock: the first host-images files of the folder (64x64, shrink_by) through pxz_transcode_varied_files,
    # against the same files through upload + the four chained device calls + download
    k = min(args.host_images, n)
    sub, subsizes = geoms[:k], sizes[:k]
    _, vals, tw, th, slots = h.shrink_varied_frames_device(buf, 64, 64, 0, FILTER, 2.0, descs=sub, channels=4)
    fo, fbuf = h.encode_varied_frames_device(subsizes, 4, 64, 64, vals, tw, th, slots)
    torch.cuda.synchronize()
    offs = fo.cpu().numpy()
    raw = fbuf[: int(offs[-1])].cpu().numpy()
    files = [raw[int(offs[i]):int(offs[i + 1])].tobytes() for i in range(k)]
    del vals, tw, th, slots, fbuf

    def host_chain():
        blob = torch.frombuffer(bytearray(b"".join(files)), dtype=torch.uint8).cuda()
        o = torch.tensor(offs.astype("int64")).cuda()
        _, v, w_, h_, s = h.decode_varied_frames_device(blob, o, subsizes, 4, 64, 64)
        h.expand_varied_frames_device(sub, 4, 64, 64, FILTER, w_, h_, s, img)
        _, v2, w2, h2, s2 = h.shrink_varied_frames_device(img, 64, 64, 0, FILTER, 1.0, descs=sub, channels=4)
        fo2, fb2 = h.encode_varied_frames_device(subsizes, 4, 64, 64, v2, w2, h2, s2)
        o2 = fo2.cpu().numpy()
        r2 = fb2[: int(o2[-1])].cpu().numpy()
        return [r2[int(o2[i]):int(o2[i + 1])].tobytes() for i in range(k)]

    def host_call():
        return h.transcode_varied_files(files, 64, 64, 0, FILTER, 1.0, FILTER)

    with StepLimit(args.step_limit, "host form"):
        ref, got = host_chain(), host_call()  # (warm-up, and the check)
        ok = ref == got
        ta, tb = [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            host_call()
            ta.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            host_chain()
            tb.append((time.perf_counter() - t0) * 1e3)
    row = dict(host_form_files=k, transcode_varied_files_ms=round(statistics.median(ta), 1),
               upload_four_device_calls_download_ms=round(statistics.median(tb), 1), bit_exact=ok)
    rows.append(row)
    print(json.dumps(row), flush=True)
    h.close()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)
    if not ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
