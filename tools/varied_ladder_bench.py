"""The varied ladder on one MI355X: one pxz_shrink_varied_ladder_frames_device call against K calls of
pxz_shrink_varied_frames_device (the baseline: one per factor, same handle, same process) on the folder of tools/varied_bench.py
(256 RGBA images, sides 64 .. 4096 log-uniform); 32x32 and 64x64 tiles, both modes, Lanczos3, K = 1, 2, 5, 20.  The factors are
the first K of the reference's sweep, from the top (whole-folder.rs:83-88: k = i / 20; times 16 for shrink_directionally, whose
values are that much smaller).  Every rung is checked bit for bit against the baseline before anything is timed.  The two flows
alternate; device time from events on the handle's stream, median of --reps.  Then the host form: one
pxz_rate_distortion_varied_images call against a loop of pxz_rate_distortion_image over the first --host-images images.

    python tools/varied_ladder_bench.py [--images 256] [--reps 5] [--host-images 16] [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import __graft_entry__ as G  # noqa: E402
from varied_bench import folder, frame_of  # noqa: E402

P = G.load_product()
SWEEP = [i / 20.0 for i in range(20, 0, -1)]  # 1.0, 0.95, ... 0.05


def factors_of(mode, K):
    step = {1: [0], 2: [0, 10], 5: [0, 4, 8, 12, 16]}.get(K) or list(range(K))
    return [SWEEP[j] * (16.0 if mode == 1 else 1.0) for j in step]


def same_rung(got, exp, c):
    """one rung of the ladder (views) against one varied call's outputs: value bits, sizes, the valid bytes of every slot"""
    gv, gw, gh, gs = got
    ev, ew, eh, es = exp
    if not (torch.equal(gv.view(torch.int32), ev.view(torch.int32)) and torch.equal(gw, ew) and torch.equal(gh, eh)):
        return False
    step = 1 << 16  # (the mask of a whole rung of a large folder would not fit beside it)
    for a in range(0, gs.shape[0], step):
        valid = torch.arange(gs.shape[1], device="cuda").view(1, -1) < (ew[a:a + step] * eh[a:a + step] * c).view(-1, 1)
        if not torch.equal(gs[a:a + step][valid], es[a:a + step][valid]):
            return False
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-images", type=int, default=16)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    h = P.Handle(0)
    buf, geoms = folder(args.images, 2026)
    stream = torch.cuda.current_stream()
    rows = []
    print(f"folder: {len(geoms)} RGBA images, {sum(g[0] * g[1] for g in geoms) / 1e6:.1f} Mpx", flush=True)
    for (bw, bh) in ((32, 32), (64, 64)):
        T = int(P.varied_layout(geoms, bw, bh)[-1])
        one = (torch.empty(T, dtype=torch.float32, device="cuda"), torch.empty(T, dtype=torch.int32, device="cuda"),
               torch.empty(T, dtype=torch.int32, device="cuda"), torch.empty((T, bw * bh * 4), dtype=torch.uint8, device="cuda"))
        for K in (1, 2, 5, 20):
            out = (torch.empty((K, T), dtype=torch.float32, device="cuda"), torch.empty((K, T), dtype=torch.int32, device="cuda"),
                   torch.empty((K, T), dtype=torch.int32, device="cuda"), torch.empty((K, T, bw * bh * 4), dtype=torch.uint8, device="cuda"))
            for mode in (0, 1):
                factors = factors_of(mode, K)

                def run_ladder():
                    h.shrink_varied_ladder_frames_device(buf, bw, bh, mode, 4, factors, descs=geoms, channels=4, out=out)

                def run_baseline():
                    for k in factors:
                        h.shrink_varied_frames_device(buf, bw, bh, mode, 4, k, descs=geoms, channels=4, out=one)

                run_ladder()
                for r, k in enumerate(factors):
                    h.shrink_varied_frames_device(buf, bw, bh, mode, 4, k, descs=geoms, channels=4, out=one)
                    torch.cuda.synchronize()
                    if not same_rung(tuple(x[r] for x in out), one, 4):
                        print(f"MISMATCH {bw}x{bh} mode {mode} K {K} rung {r} (factor {k})", flush=True)
                        sys.exit(1)
                flows = [run_ladder, run_baseline]
                times = {f: [] for f in flows}
                for i in range(args.reps + 1):  # (the first round warms up)
                    ev = []
                    for f in (flows if i % 2 == 0 else flows[::-1]):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record(stream)
                        f()
                        e1.record(stream)
                        ev.append((f, e0, e1))
                    torch.cuda.synchronize()
                    if i:
                        for f, e0, e1 in ev:
                            times[f].append(e0.elapsed_time(e1))
                tl, tb = statistics.median(times[run_ladder]), statistics.median(times[run_baseline])
                row = dict(tile=f"{bw}x{bh}", mode=mode, K=K, tiles=T, ladder_ms=round(tl, 3), k_varied_calls_ms=round(tb, 3),
                           speedup=round(tb / tl, 3), bit_exact=True, ladder_samples=[round(t, 3) for t in times[run_ladder]],
                           k_varied_calls_samples=[round(t, 3) for t in times[run_baseline]])
                rows.append(row)
                print(json.dumps(row), flush=True)
            del out
            torch.cuda.empty_cache()
        del one
        torch.cuda.empty_cache()
    # host form: the first host-images images of the folder, 64x64 tiles, five factors, Lanczos3 down and CatmullRom up
    n = min(args.host_images, len(geoms))
    imgs = [frame_of(buf, g)[0].cpu().numpy() for g in geoms[:n]]
    for mode in (0, 1):
        factors = factors_of(mode, 5)
        h.rate_distortion_varied_images(imgs, 64, 64, mode, 4, 2, factors)  # (warm-up)
        t0 = time.perf_counter()
        fb, sse = h.rate_distortion_varied_images(imgs, 64, 64, mode, 4, 2, factors)
        t_varied = (time.perf_counter() - t0) * 1e3
        [h.rate_distortion_image(img, 64, 64, mode, 4, 2, factors) for img in imgs[:1]]  # (warm-up)
        t0 = time.perf_counter()
        ref = [h.rate_distortion_image(img, 64, 64, mode, 4, 2, factors) for img in imgs]
        t_loop = (time.perf_counter() - t0) * 1e3
        ok = all((fb[:, i] == ref[i][0]).all() and (sse[:, i] == ref[i][1]).all() for i in range(n))
        row = dict(host_form_images=n, mode=mode, K=5, rate_distortion_varied_images_ms=round(t_varied, 1),
                   per_image_rate_distortion_image_ms=round(t_loop, 1), exact=bool(ok))
        rows.append(row)
        print(json.dumps(row), flush=True)
        if not ok:
            sys.exit(1)
    h.close()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
