"""The distortion call against the composition it replaces, in one process:

  python3 tools/rd_bench.py [n=10]

8 x 7680x4320 RGBA frames (env DIST, NF, W, H as in tools/exp.py), shrunk by the factor ladder (shrink_by, Lanczos3) at the five
factors 1.0 0.5 0.25 2.0 0.125; 32x32 and 64x64 tiles; up-scaling filters Nearest and Lanczos3; n_sets 1 (the first rung) and 5.
Timed with device events on the handle's stream, alternating which goes first, medians printed as one JSON line per case:
  distortion_ms   pxz_distortion_frames_device over the sets (tile sums and frame totals)
  varied_ms       pxz_distortion_varied_frames_device on the same frames as a batch of NF images (one set only)
  composed_ms     what the library offered before: pxz_expand_frames_device per set into one reused image, then torch per frame --
                  (a - b)^2 summed per tile into int64 (int16 differences, int32 squares: the cheapest spelling of it)
clone_share is the share of the sets' tiles stored at full size, which the distortion call neither reads nor resizes.  Before
timing, the call's tile sums are checked against the composition's, exactly.
"""
import json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from __graft_entry__ import load_product
P = load_product()
n = int(sys.argv[1]) if len(sys.argv) > 1 else 10
dist, nf = int(os.environ.get("DIST", "0")), int(os.environ.get("NF", "8"))
W, H, ch = int(os.environ.get("W", "7680")), int(os.environ.get("H", "4320")), 4
factors = [1.0, 0.5, 0.25, 2.0, 0.125]

h = P.Handle(0)
frames = h.synth_frames_device(nf, H, W, ch, 0, dist)
image = torch.empty_like(frames)
stream = torch.cuda.current_stream()


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    fn()
    e1.record(stream)
    return e0, e1


def tile_sums(a, b, bs):
    """per tile and channel sum of (a - b)^2 of one frame [H,W,C] -> int64 [tiles, C]"""
    d = a.to(torch.int16) - b.to(torch.int16)
    d = (d.to(torch.int32) * d.to(torch.int32))
    rows, cols = -(-H // bs), -(-W // bs)
    d = torch.nn.functional.pad(d, (0, 0, 0, cols * bs - W, 0, rows * bs - H))
    return d.reshape(rows, bs, cols, bs, ch).sum(dim=(1, 3), dtype=torch.int64).reshape(rows * cols, ch)


for bs in (32, 64):
    vals, ow, oh, slots = h.shrink_ladder_frames_device(frames, bs, bs, 0, 4, factors)
    cols, rows = P.grid(W, H, bs, bs)
    T = cols * rows
    fw = torch.full((rows, cols), bs, dtype=torch.int32, device="cuda")
    fh = fw.clone()
    fw[:, -1] = W - (cols - 1) * bs
    fh[-1, :] = H - (rows - 1) * bs
    full = (ow == fw.reshape(-1)) & (oh == fh.reshape(-1))
    descs = [(W, H, W * ch, f * W * H * ch) for f in range(nf)]
    for flt in (0, 4):
        for K in (1, 5):
            sw, sh, ss = ow[:K].contiguous(), oh[:K].contiguous(), slots[:K].contiguous()
            out = h.distortion_frames_device(frames, bs, bs, flt, sw, sh, ss)
            composed = torch.empty_like(out[0])

            def run_call():
                h.distortion_frames_device(frames, bs, bs, flt, sw, sh, ss, out=out)

            def run_varied():
                h.distortion_varied_frames_device(frames, bs, bs, flt, sw[0].reshape(-1), sh[0].reshape(-1), ss[0].reshape(nf * T, -1),
                                                  descs=descs, channels=ch, out=vout)

            def run_composed():
                for r in range(K):
                    h.expand_frames_device(tuple(frames.shape), bs, bs, flt, sw[r], sh[r], ss[r], out=image)
                    for f in range(nf):
                        composed[r, f] = tile_sums(frames[f], image[f], bs)

            run_call()
            run_composed()
            torch.cuda.synchronize()
            assert (out[0] == composed).all() and (out[1] == composed.sum(dim=2)).all(), "the call and the composition differ"
            flows = [run_call, run_composed]
            if K == 1:
                vout = (torch.empty((nf * T, ch), dtype=torch.int64, device="cuda"), torch.empty((nf, ch), dtype=torch.int64, device="cuda"))
                run_varied()
                torch.cuda.synchronize()
                assert (vout[0].reshape(nf, T, ch) == out[0][0]).all() and (vout[1] == out[1][0]).all(), "the varied call differs"
                flows.append(run_varied)
            times = {f: [] for f in flows}
            for i in range(n):
                order = flows[i % len(flows):] + flows[:i % len(flows)]
                ev = [(f, timed(f)) for f in order]
                torch.cuda.synchronize()
                for f, (e0, e1) in ev:
                    times[f].append(e0.elapsed_time(e1))
            med = {f: statistics.median(t) for f, t in times.items()}
            line = {"flow": "distortion", "frames": f"{nf}x{W}x{H}x{ch}", "block": bs, "filter_up": flt, "dist": dist, "n_sets": K,
                    "clone_share": round(float(full[:K].float().mean()), 4), "distortion_ms": round(med[run_call], 4),
                    "composed_ms": round(med[run_composed], 4), "speedup": round(med[run_composed] / med[run_call], 3)}
            if K == 1:
                line["varied_ms"] = round(med[run_varied], 4)
            line.update({"rounds": n, "exact": True})
            print(json.dumps(line), flush=True)
            del out, composed, sw, sh, ss
    del vals, ow, oh, slots
    torch.cuda.empty_cache()
h.close()
