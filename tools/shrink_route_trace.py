"""Which kernels a single-geometry shrink call launches, case by case: the check that a change of the host path (the route of
pxz_shrink_plan.h) launches what the build before it launched.

  rocprofv3 --kernel-trace --output-format csv -d OUT -- python tools/shrink_route_trace.py run
  python tools/shrink_route_trace.py summarize OUT > routes.txt

`run` walks the cases of tests/test_shrink_plan_host.py that can be called (no knobs: they are per process; no 613 MB pitch), one
synth launch between two cases as a separator; the transparency cases run twice on one handle, so that the second call reads the
first one's statistics.  `summarize` turns the trace into one line per launch -- case, kernel, grid, workgroup, LDS bytes -- which
is diffed between two builds (PXZ_LIB names the other build's library)."""
import csv
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BY, DIRECTIONAL, LANCZOS3, NEAREST = 0, 1, 4, 0

# (name, call, arguments): w, h, c, n, bw, bh, mode; low address bits, pitch, stride; opaque alpha; px, filt, hint; repeat
D = dict(w=64, h=64, c=4, n=1, bw=32, bh=32, mode=DIRECTIONAL, low=0, pitch=None, stride=None, opaque=True, px=True, filt=LANCZOS3, hint=False,
         factor=16.0, repeat=1)
CASES = [
    ("aligned", "shrink", {}), ("low 4", "shrink", dict(low=4)), ("low 1", "shrink", dict(low=1)), ("pitch 260", "shrink", dict(pitch=260)),
    ("stride, one frame", "shrink", dict(stride=16388)), ("stride, two frames", "shrink", dict(n=2, stride=16388)),
    ("32: 40x40", "shrink", dict(mode=BY, w=40, h=40)), ("32: 64x40", "shrink", dict(mode=BY, h=40)), ("32: 64x36", "shrink", dict(mode=BY, h=36)),
    ("32: 33x64", "shrink", dict(mode=BY, w=33)), ("16: 20x20", "shrink", dict(mode=BY, bw=16, bh=16, w=20, h=20)),
    ("16: 32x24", "shrink", dict(mode=BY, bw=16, bh=16, w=32, h=24)), ("16: 32x32", "shrink", dict(mode=BY, bw=16, bh=16, w=32, h=32)),
    ("64: 128x72", "shrink", dict(mode=BY, bw=64, bh=64, w=128, h=72)), ("64: 128x68", "shrink", dict(mode=BY, bw=64, bh=64, w=128, h=68)),
    ("8x8", "shrink", dict(mode=BY, bw=8, bh=8, w=16, h=16)), ("4x12", "shrink", dict(mode=BY, bw=4, bh=12, w=8, h=24, low=4)),
    ("128x128", "shrink", dict(mode=BY, bw=128, bh=128, w=128, h=128)), ("128x132", "shrink", dict(mode=BY, bw=128, bh=132, w=128, h=132)),
    ("6x16", "shrink", dict(mode=BY, bw=6, bh=16, w=12, h=32)), ("narrow frame", "shrink", dict(mode=BY, w=20)),
    ("rgb 32", "shrink", dict(mode=BY, c=3)), ("rgb 16", "shrink", dict(mode=BY, c=3, bw=16, bh=16, w=32, h=32)),
    ("rgb 64", "shrink", dict(mode=BY, c=3, bw=64, bh=64, w=128, h=128)), ("rgb odd address", "shrink", dict(mode=BY, c=3, low=1)),
    ("rgb 24x8", "shrink", dict(mode=BY, c=3, bw=24, bh=8, w=48, h=16)), ("rgb directional odd", "shrink", dict(c=3, low=1)),
    ("116", "shrink", dict(bw=116, bh=116, w=116, h=116)), ("117", "shrink", dict(bw=117, bh=117, w=351, h=468)),
    ("ladder 89", "ladder", dict(mode=BY, bw=89, bh=89, w=89, h=89)), ("ladder 90", "ladder", dict(mode=BY, bw=90, bh=90, w=90, h=90)),
    ("ladder 32", "ladder", dict(mode=BY, w=40, h=40)), ("ladder directional", "ladder", {}),
    ("2048 tiles, transparent", "shrink", dict(w=2048, h=1024, opaque=False, repeat=2)),
    ("8192 tiles, transparent", "shrink", dict(w=4096, h=2048, opaque=False, repeat=2)),
    ("8192 tiles, opaque", "shrink", dict(w=4096, h=2048, repeat=2)), ("hint", "shrink", dict(hint=True, opaque=False)),
    ("no pixels", "shrink", dict(mode=BY, px=False)), ("lod directional", "lod", {}), ("lod shrink_by", "lod", dict(mode=BY, w=40, h=40)),
    ("nearest rgb odd", "shrink", dict(mode=BY, c=3, low=1, filt=NEAREST)), ("process", "process", dict(w=40, h=40)), ("process rgb", "process", dict(c=3, low=1)),
    ("bench: 256x256 RGBA 32x32 directional", "shrink", dict(w=256, h=256)),
    ("bench: 1920x1080 RGB odd address 32x32 shrink_by", "shrink", dict(mode=BY, c=3, w=1920, h=1080, low=1, factor=1.0)),
]


def frames_of(a):
    """-> a uint8 CUDA tensor [n, h, w, c] at the asked address bits, pitch and stride, filled with seeded noise"""
    import torch
    pitch = a["pitch"] or a["w"] * a["c"]
    stride = a["stride"] or pitch * a["h"]
    flat = torch.empty(a["low"] + a["n"] * stride + 64, dtype=torch.uint8, device="cuda")
    flat.random_(0, 256)
    frames = torch.as_strided(flat, (a["n"], a["h"], a["w"], a["c"]), (stride, pitch, a["c"], 1), a["low"])
    if a["c"] == 4 and a["opaque"]:
        frames[..., 3] = 255
    assert frames.data_ptr() % 16 == a["low"] % 16
    return frames


def run():
    import torch
    from __graft_entry__ import load_product
    product = load_product()
    torch.manual_seed(7)
    for i, (name, call, change) in enumerate(CASES):
        a = {**D, **change}
        frames = frames_of(a)
        h = product.Handle(0)
        h.synth_frames_device(1, 1, 1, 4)  # the separator
        for _ in range(a["repeat"]):
            if call == "shrink":
                h.shrink_frames_device(frames, a["bw"], a["bh"], a["mode"], a["filt"], a["factor"], want_pixels=a["px"], transparency_hint=a["hint"])
            elif call == "lod":
                h.lod_frames_device(frames, a["bw"], a["bh"], a["mode"], a["factor"])
            elif call == "ladder":
                h.shrink_ladder_frames_device(frames, a["bw"], a["bh"], a["mode"], a["filt"], [1.0, 0.25])
            else:
                h.process_frames_device(frames, a["bw"], a["bh"])
            torch.cuda.synchronize()
        h.close()
        print(i, name, flush=True)
    print("cases", len(CASES))


def summarize(folder):
    files = glob.glob(os.path.join(folder, "**", "*kernel_trace.csv"), recursive=True)
    assert len(files) == 1, files
    rows = list(csv.DictReader(open(files[0])))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    case = -1
    for r in rows:
        name = r["Kernel_Name"]
        if "synth" in name:
            case += 1
            continue
        if case < 0 or name.startswith("void at::") or "at::native" in name:
            continue
        geom = [r[k] for k in sorted(r) if k.startswith(("Grid_Size", "Workgroup_Size", "LDS_Block_Size"))]
        print(CASES[case][0] if case < len(CASES) else case, "|", name.split("(")[0], "|", " ".join(geom))
    print("cases", case + 1)


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run()
    else:
        summarize(sys.argv[2])
