"""Factor ladder against the single calls it replaces, in one process:

  python3 tools/ladder_bench.py [block=32] [K=5] [n=20]

8 x 7680x4320 frames (env CH, DIST, NF, W, H, FILTER as in tools/exp.py), shrink_by at the first K factors of
1.0 0.5 0.25 2.0 0.125 0.0625 4.0 8.0 ... .  Each round times one ladder call and the K single calls with device events on
the handle's stream, alternating which goes first; the medians are printed as one JSON line.  Before timing, every rung is
checked bit for bit against its single call at this size (values, sizes, valid slot bytes).
"""
import json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from __graft_entry__ import load_product
P = load_product()
argv = sys.argv[1:]
bs = int(argv[0]) if len(argv) > 0 else 32
K = int(argv[1]) if len(argv) > 1 else 5
n = int(argv[2]) if len(argv) > 2 else 20
ch, dist, nf = int(os.environ.get("CH", "4")), int(os.environ.get("DIST", "0")), int(os.environ.get("NF", "8"))
W, H, flt = int(os.environ.get("W", "7680")), int(os.environ.get("H", "4320")), int(os.environ.get("FILTER", "4"))
ALL = [1.0, 0.5, 0.25, 2.0, 0.125, 0.0625, 4.0, 8.0, 0.03125, 16.0, 0.015625, 32.0, 0.0078125, 64.0, 0.00390625, 128.0]
factors = ALL[:K]

h = P.Handle(0)
frames = h.synth_frames_device(nf, H, W, ch, 0, dist)
lad = h.shrink_ladder_frames_device(frames, bs, bs, 0, flt, factors)
one = None
for r, k in enumerate(factors):
    one = h.shrink_frames_device(frames, bs, bs, 0, flt, k, out=one)
    torch.cuda.synchronize()
    sv, sw, sh, ss = one
    assert (lad[0][r].view(torch.int32) == sv.view(torch.int32)).all(), f"rung {r}: values"
    assert (lad[1][r] == sw).all() and (lad[2][r] == sh).all(), f"rung {r}: sizes"
    valid = (sw.long() * sh.long() * ch).reshape(-1)
    a, b = lad[3][r].reshape(valid.numel(), -1), ss.reshape(valid.numel(), -1)
    lane = torch.arange(a.shape[1], device=a.device)[None, :]
    chunk = max(1, (256 << 20) // a.shape[1])
    for t0 in range(0, a.shape[0], chunk):
        t1 = min(a.shape[0], t0 + chunk)
        assert not ((a[t0:t1] != b[t0:t1]) & (lane < valid[t0:t1, None])).any(), f"rung {r}: payload bytes"
# algorithmic bytes of the ladder's second stage: one read of the frames + the valid bytes of every rung's slots
alg = nf * W * H * ch + int((lad[1].long() * lad[2].long()).sum()) * ch
singles = [h.shrink_frames_device(frames, bs, bs, 0, flt, k) for k in factors]  # one output set per rung, as the ladder has
stream = torch.cuda.current_stream()


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    fn()
    e1.record(stream)
    return e0, e1


def run_ladder():
    h.shrink_ladder_frames_device(frames, bs, bs, 0, flt, factors, out=lad)


def run_singles():
    for k, o in zip(factors, singles):
        h.shrink_frames_device(frames, bs, bs, 0, flt, k, out=o)


for _ in range(3):
    run_ladder()
    run_singles()
torch.cuda.synchronize()
tl, ts = [], []
for i in range(n):
    order = (run_ladder, run_singles) if i % 2 == 0 else (run_singles, run_ladder)
    ev = [(f, timed(f)) for f in order]
    torch.cuda.synchronize()
    for f, (e0, e1) in ev:
        (tl if f is run_ladder else ts).append(e0.elapsed_time(e1))
ml, ms = statistics.median(tl), statistics.median(ts)
print(json.dumps({"flow": "ladder", "frames": f"{nf}x{W}x{H}x{ch}", "block": bs, "filter": flt, "dist": dist, "K": K,
                  "factors": factors, "ladder_ms": round(ml, 4), "singles_ms": round(ms, 4), "speedup": round(ms / ml, 3),
                  "stage2_algorithmic_bytes": alg, "rounds": n, "bit_exact": True}))
h.close()
