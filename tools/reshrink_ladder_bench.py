"""The re-shrink ladder on one MI355X: one pxz_reshrink_varied_ladder_frames_device call against K calls of
pxz_reshrink_varied_frames_device (the baseline: one per factor, same handle, same process, the same stored tiles).  The folder
is tools/varied_bench.py's (256 RGBA images of 64-4096 px), first shrunk at factor f as in tools/transcode_bench.py -- its four
rows of mostly full tiles (the clone-in case) and its four rows of strongly shrunk files (every tile expanded first) -- then
re-shrunk at K factors: f times the first K of the reference's sweep from the top (whole-folder.rs:83-88: k = i / 20), the
question being how far an archive written at f can be squeezed.  32x32 and 64x64 tiles, both modes, Lanczos3 on both sides,
K = 1, 2, 5, 20.

Both sides run in this one process, alternating, after >= 60 ms of untimed load and W steps of each; device time from events,
median and every sample of --reps runs.  Every rung is checked bit for bit against the baseline before anything is timed.  Each
step runs under a limit of its own (--step-limit seconds): a step that exceeds it ends the process with status 124.

    python tools/reshrink_ladder_bench.py [--images 256] [--reps 5] [--warmup 3] [--json out.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from transcode_bench import CONFIGS, FILTER, StepLimit, compare  # noqa: E402

SWEEP = [i / 20.0 for i in range(20, 0, -1)]  # 1.0, 0.95, ... 0.05
KS = (1, 2, 5, 20)


def factors_of(f, K):
    step = {1: [0], 2: [0, 10], 5: [0, 4, 8, 12, 16]}.get(K) or list(range(K))
    return [f * SWEEP[j] for j in step]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--step-limit", type=float, default=120.0)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    assert args.reps >= 5, "a median of fewer than 5 is not reported"

    import torch
    import varied_bench as VB
    from varied_ladder_bench import same_rung
    P = VB.P
    assert torch.cuda.is_available(), "this tool measures on the MI355X; there is nothing to report without one"
    h = P.Handle(0)
    buf, geoms = VB.folder(args.images, 2026)
    sizes = [(g[0], g[1]) for g in geoms]
    print(f"folder of {len(geoms)} RGBA images, {sum(w * hh for (w, hh) in sizes) / 1e6:.1f} Mpx", flush=True)
    rows = []
    for (b, mode, f1, _, label) in CONFIGS:
        T = int(P.varied_layout(geoms, b, b)[-1])
        _, _, tw, th, slots = h.shrink_varied_frames_device(buf, b, b, mode, FILTER, f1, descs=geoms, channels=4)
        torch.cuda.synchronize()
        place = torch.tensor([min(b, w - x) * min(b, hh - y) for (w, hh) in sizes for y in range(0, hh, b) for x in range(0, w, b)], device="cuda")
        stored_full = round(float((tw * th == place).float().mean()), 4)
        del place
        single = (torch.empty(T, dtype=torch.float32, device="cuda"), torch.empty(T, dtype=torch.int32, device="cuda"),
                  torch.empty(T, dtype=torch.int32, device="cuda"), torch.empty((T, b * b * 4), dtype=torch.uint8, device="cuda"))
        for K in KS:
            factors = factors_of(f1, K)
            out = (torch.empty((K, T), dtype=torch.float32, device="cuda"), torch.empty((K, T), dtype=torch.int32, device="cuda"),
                   torch.empty((K, T), dtype=torch.int32, device="cuda"), torch.empty((K, T, b * b * 4), dtype=torch.uint8, device="cuda"))

            def run_ladder():
                h.reshrink_varied_ladder_frames_device(sizes, 4, b, b, mode, FILTER, factors, FILTER, tw, th, slots, out=out)

            def run_baseline():
                for f in factors:
                    h.reshrink_varied_frames_device(sizes, 4, b, b, mode, FILTER, f, FILTER, tw, th, slots, out=single)

            what = f"{b}x{b} files at {f1} ({'shrink_by' if mode == 0 else 'directional'}), K = {K}"
            with StepLimit(args.step_limit, what + ": check"):
                run_ladder()
                torch.cuda.synchronize()
                ok = h.decode_status() == 0
                resamples = 0
                for r, f in enumerate(factors):
                    h.reshrink_varied_frames_device(sizes, 4, b, b, mode, FILTER, f, FILTER, tw, th, slots, out=single)
                    torch.cuda.synchronize()
                    ok = ok and same_rung(tuple(x[r] for x in out), single, 4)
                # distinct reduced sizes per tile among its rungs: the resamples the ladder runs, against K in the baseline
                key = (out[1].to(torch.int64) << 32) | out[2].to(torch.int64)
                srt = torch.sort(key, dim=0).values
                distinct = 1 + (srt[1:] != srt[:-1]).sum(dim=0) if K > 1 else torch.ones(T, dtype=torch.int64, device="cuda")
                resamples = round(float(distinct.float().mean()), 3)
                del key, srt, distinct
            if not ok:
                print(f"MISMATCH {what}", flush=True)
                sys.exit(1)
            row = dict(tile=f"{b}x{b}", mode=mode, files=label.split(" ->")[0], file_factor=f1, K=K, factors=[round(f, 5) for f in factors], tiles=T,
                       share_stored_full=stored_full, distinct_sizes_per_tile=resamples, bit_exact=ok)
            row["ladder"], row["k_calls"] = compare(torch, run_ladder, run_baseline, args.warmup, args.reps, args.step_limit, what)
            row["speedup"] = round(row["k_calls"]["ms"] / row["ladder"]["ms"], 2)
            rows.append(row)
            print(json.dumps(row), flush=True)
            if args.json:  # (kept current row by row: a step limit ends the process)
                with open(args.json, "w") as f:
                    json.dump(rows, f, indent=1)
            del out
            torch.cuda.empty_cache()
        del single, tw, th, slots
        torch.cuda.empty_cache()
    h.close()


if __name__ == "__main__":
    main()
