"""Wall-clock cost of one pxz_shrink_frames_device call where the host's share is largest: a few thousand calls on one handle,
one synchronize at the end, microseconds per call (the binding's own share included, the same for every build).

  python tools/shrink_call_cost.py [--calls 4000] [--reps 5]      (PXZ_LIB names another build's library)

Rows: 1 x 256x256 RGBA, 32x32 shrink_directionally, device-resident; 1 x 1920x1080 RGB at an odd address, 32x32 shrink_by (the
widen route).  Prints one JSON line: per row the median and the spread of the repetitions."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch
    from __graft_entry__ import load_product
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=4000)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    product = load_product()
    h = product.Handle(0)
    torch.manual_seed(3)
    small = torch.randint(0, 256, (1, 256, 256, 4), dtype=torch.uint8, device="cuda")
    small[..., 3] = 255
    flat = torch.randint(0, 256, (1 + 1080 * 1920 * 3,), dtype=torch.uint8, device="cuda")
    rgb = torch.as_strided(flat, (1, 1080, 1920, 3), (1080 * 1920 * 3, 1920 * 3, 3, 1), 1)
    rows = [("256x256 RGBA 32x32 directional", small, product.MODE_SHRINK_DIRECTIONALLY, 16.0),
            ("1920x1080 RGB odd address 32x32 shrink_by", rgb, product.MODE_SHRINK_BY, 1.0)]
    result = {}
    for name, frames, mode, factor in rows:
        out = h.shrink_frames_device(frames, 32, 32, mode, product.FILTER_LANCZOS3, factor)
        for _ in range(200):
            h.shrink_frames_device(frames, 32, 32, mode, product.FILTER_LANCZOS3, factor, out=out)
        torch.cuda.synchronize()
        us = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            for _ in range(args.calls):
                h.shrink_frames_device(frames, 32, 32, mode, product.FILTER_LANCZOS3, factor, out=out)
            torch.cuda.synchronize()
            us.append((time.perf_counter() - t0) * 1e6 / args.calls)
        us.sort()
        result[name] = {"median_us": round(us[len(us) // 2], 2), "min_us": round(us[0], 2), "max_us": round(us[-1], 2)}
    h.close()
    print(json.dumps({"lib": product.binding.library_path(), "calls": args.calls, "reps": args.reps, "us_per_call": result}))


if __name__ == "__main__":
    main()
