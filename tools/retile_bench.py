"""Re-tiling .pixlzr tiles on one MI355X (the reference CLI's pix_to_pix with -b for a folder), by the protocol of
tools/transcode_bench.py.  Two comparisons per row:

  tiles -> tiles   pxz_retile_varied_frames_device against the calls that were there before it, pxz_expand_varied_frames_device at
                   the source block + pxz_shrink_varied_frames_device at the destination block, from the same decoded tiles
                   (device time from HIP events);
  files -> files   the host form pxz_transcode_varied_files of this tree against the same call of a library built from the parent
                   commit, which PXZ_LIB names (wall clock: the call is synchronous, uploads and downloads included).  Without
                   PXZ_LIB this comparison is left out.  The yardstick is the parent's composition, never the new code.

The folder is tools/varied_bench.py's (256 RGBA images of 64-4096 px), first shrunk at the source block at factor f, then re-tiled
at the destination block at f / 2: the reference's usual factors (shrink_by 2.0 -> 1.0, directional 32 -> 16) and the strongly
shrunk pair of tools/transcode_bench.py; Lanczos3 on both sides.  Pairs: 64x64 -> 32x32, 32x32 -> 64x64, 32x32 -> 48x20.  The
directional rows of 32x32 -> 48x20 take the images that leave no 1-px edge tile against 48x20 (the call refuses the others, as
the reference panics on them); their count is in the row.

Both sides of a comparison run in this one process, alternating, after bench.py's warm-up (>= 60 ms of untimed load, then W
steps of each); median and every sample of --reps runs.  Every row is checked bit for bit before it is timed.  The bytes of the
image batch that the chained calls need and the re-tile does not are printed beside the times: a fact of the calls'
signatures, not a measurement.  Each timed step runs under a limit of its own (--step-limit seconds): a step that exceeds it ends
the process with status 124, and nothing else is started.

    [PXZ_LIB=<parent build>] python tools/retile_bench.py [--images 256] [--host-images 256] [--reps 9] [--warmup 5]
                                                          [--variant-lib <another build of this tree>] [--json out.json]
"""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

PAIRS = [((64, 64), (32, 32)), ((32, 32), (64, 64)), ((32, 32), (48, 20))]
FACTORS = [  # (mode, factor of the files, factor of the re-tile, label)
    (0, 2.0, 1.0, "shrink_by 2.0 -> 1.0"), (1, 32.0, 16.0, "directional 32 -> 16"),
    # the folder's images keep nearly every tile full at the factors above (the clone-in case); strongly shrunk files, whose
    # tiles are expanded before they are assembled, for the record
    (0, 0.12, 0.06, "shrink_by 0.12 -> 0.06"), (1, 2.0, 1.0, "directional 2 -> 1"),
]
FILTER = 4  # Lanczos3


def other_binding(path, name):
    """the binding module once more, over another build of the library (binding.py reads PXZ_LIB when it is imported); None
    without a path.  PXZ_LIB is out of the environment again before the tree's own package is imported, which then loads the
    tree's library."""
    if not path:
        return None
    os.environ["PXZ_LIB"] = os.path.abspath(path)
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "pixlzr-rust_amd", "binding.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    del os.environ["PXZ_LIB"]
    assert mod.library_path() == os.path.abspath(path)
    return mod


def wall_compare(a, b, warmup, reps, limit, what, StepLimit):
    """two synchronous host calls alternating: >= 60 ms and `warmup` steps of each untimed, then `reps` timed steps of each"""
    def one(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3
    with StepLimit(limit, what + " (warm-up)"):
        t0, k = time.perf_counter(), 0
        while (time.perf_counter() - t0) * 1e3 < 60.0 or k < warmup:
            a()
            b()
            k += 1
    ta, tb = [], []
    for _ in range(reps):
        with StepLimit(limit, what):
            ta.append(one(a))
            tb.append(one(b))
    return (dict(ms=round(statistics.median(ta), 2), samples=[round(t, 2) for t in ta]),
            dict(ms=round(statistics.median(tb), 2), samples=[round(t, 2) for t in tb]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--host-images", type=int, default=256)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--step-limit", type=float, default=120.0)
    ap.add_argument("--variant-lib", default=None, help="another build of this tree (an experiment: make exp EXP=<n>); its re-tile is "
                    "timed against this tree's, tiles -> tiles, after a check that both give the same bits")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()

    PB = other_binding(os.environ.pop("PXZ_LIB", None), "pxz_parent_binding")
    VBIND = other_binding(args.variant_lib, "pxz_variant_binding")
    import torch
    import varied_bench as VB
    from transcode_bench import StepLimit, compare
    P = VB.P
    assert torch.cuda.is_available(), "this tool measures on the MI355X; there is nothing to report without one"
    assert os.path.samefile(P.library_path(), os.path.join(ROOT, "pixlzr-rust_amd", "csrc", "libpixlzr_hip.so")), P.library_path()
    h = P.Handle(0)
    hp = None
    if PB is not None:
        assert not hasattr(PB.load_library(), "pxz_retile_varied_frames_device"), "PXZ_LIB must name a build of the parent commit"
        hp = PB.Handle(0)
    hv = VBIND.Handle(0) if VBIND is not None else None
    buf, all_geoms = VB.folder(args.images, 2026)
    img = torch.empty_like(buf)  # what expand-varied writes and shrink-varied reads back: the re-tile allocates none of it
    print(f"folder of {len(all_geoms)} RGBA images, {sum(g[0] * g[1] for g in all_geoms) / 1e6:.1f} Mpx; "
          f"files -> files against {PB.library_path() if PB else 'nothing (no PXZ_LIB)'}", flush=True)
    rows = []
    for ((sw, sh), (dw, dh)) in PAIRS:
        for (mode, f1, f2, label) in FACTORS:
            geoms = [g for g in all_geoms if mode == 0 or (g[0] % dw != 1 and g[1] % dh != 1 and g[0] % sw != 1 and g[1] % sh != 1)]
            sizes = [(g[0], g[1]) for g in geoms]
            n = len(geoms)
            image_batch_bytes = sum(g[0] * g[1] * 4 for g in geoms)
            what = f"{sw}x{sh} -> {dw}x{dh} {label}"
            T = int(P.varied_layout(geoms, dw, dh)[-1])
            _, vals, tw, th, slots = h.shrink_varied_frames_device(buf, sw, sh, mode, FILTER, f1, descs=geoms, channels=4)
            torch.cuda.synchronize()

            def outputs():
                return (torch.empty(T, dtype=torch.float32, device="cuda"), torch.empty(T, dtype=torch.int32, device="cuda"),
                        torch.empty(T, dtype=torch.int32, device="cuda"), torch.empty((T, dw * dh * 4), dtype=torch.uint8, device="cuda"))
            out_a, out_b = outputs(), outputs()

            def retile():
                h.retile_varied_frames_device(sizes, 4, sw, sh, dw, dh, mode, FILTER, f2, FILTER, tw, th, slots, out=out_a)

            def expand_shrink():
                h.expand_varied_frames_device(geoms, 4, sw, sh, FILTER, tw, th, slots, img)
                h.shrink_varied_frames_device(img, dw, dh, mode, FILTER, f2, descs=geoms, channels=4, out=out_b)

            # bit for bit before anything is timed
            with StepLimit(args.step_limit, f"{what}: check"):
                retile()
                expand_shrink()
                torch.cuda.synchronize()
                ok = h.decode_status() == 0
                ok = ok and torch.equal(out_a[0].view(torch.int32), out_b[0].view(torch.int32)) and torch.equal(out_a[1], out_b[1]) and torch.equal(out_a[2], out_b[2])
                valid = torch.arange(dw * dh * 4, device="cuda").view(1, -1) < (out_b[1] * out_b[2] * 4).view(-1, 1)
                ok = ok and torch.equal(out_a[3][valid], out_b[3][valid])
                del valid
            if not ok:
                print(f"MISMATCH {what}: tiles -> tiles", flush=True)
                sys.exit(1)
            src_place = torch.tensor([min(sw, w - x) * min(sh, hh - y) for (w, hh) in sizes for y in range(0, hh, sh) for x in range(0, w, sw)], device="cuda")
            dst_place = torch.tensor([min(dw, w - x) * min(dh, hh - y) for (w, hh) in sizes for y in range(0, hh, dh) for x in range(0, w, dw)], device="cuda")
            row = dict(pair=f"{sw}x{sh} -> {dw}x{dh}", files=label, images=n, source_tiles=int(tw.numel()), tiles=T, image_batch_bytes=image_batch_bytes,
                       bit_exact=ok, share_stored_full=round(float((tw * th == src_place).float().mean()), 4),
                       share_full_after=round(float((out_a[1] * out_a[2] == dst_place).float().mean()), 4),
                       lds_bytes=P.retile_lds_bytes(sw, sh, dw, dh, mode, FILTER))
            del src_place, dst_place
            row["retile"], row["expand_plus_shrink"] = compare(torch, retile, expand_shrink, args.warmup, args.reps, args.step_limit,
                                                               f"{what}: tiles -> tiles")
            row["retile_not_slower"] = row["retile"]["ms"] <= row["expand_plus_shrink"]["ms"]
            if hv is not None:
                out_v = outputs()

                def retile_variant():
                    hv.retile_varied_frames_device(sizes, 4, sw, sh, dw, dh, mode, FILTER, f2, FILTER, tw, th, slots, out=out_v)

                with StepLimit(args.step_limit, f"{what}: variant check"):
                    retile_variant()
                    torch.cuda.synchronize()
                    valid = torch.arange(dw * dh * 4, device="cuda").view(1, -1) < (out_b[1] * out_b[2] * 4).view(-1, 1)
                    same = (torch.equal(out_v[0].view(torch.int32), out_b[0].view(torch.int32)) and torch.equal(out_v[1], out_b[1]) and
                            torch.equal(out_v[2], out_b[2]) and torch.equal(out_v[3][valid], out_b[3][valid]))
                    del valid
                if not same:
                    print(f"MISMATCH {what}: variant build", flush=True)
                    sys.exit(1)
                row["retile_again"], row["retile_variant_build"] = compare(torch, retile, retile_variant, args.warmup, args.reps, args.step_limit,
                                                                           f"{what}: this tree's re-tile against the variant build's")
                del out_v

            if hp is not None:
                # files -> files: the first host-images files, on the host, through both libraries' host forms
                k = min(args.host_images, n)
                fo, fbuf = h.encode_varied_frames_device(sizes[:k], 4, sw, sh, vals, tw, th, slots)
                torch.cuda.synchronize()
                offs = fo.cpu().numpy()
                raw = fbuf[: int(offs[-1])].cpu().numpy()
                files = [raw[int(offs[i]):int(offs[i + 1])].tobytes() for i in range(k)]
                del fo, fbuf, raw
                res = {}
                with StepLimit(args.step_limit, f"{what}: files size"):
                    total = sum(len(f) for f in h.transcode_varied_files(files, dw, dh, mode, FILTER, f2, FILTER))
                out_new, out_old = np.empty(total + 4096, np.uint8), np.empty(total + 4096, np.uint8)

                def files_new():
                    res["new"] = h.transcode_varied_files(files, dw, dh, mode, FILTER, f2, FILTER, out=out_new)

                def files_parent():
                    res["old"] = hp.transcode_varied_files(files, dw, dh, mode, FILTER, f2, FILTER, out=out_old)

                with StepLimit(args.step_limit, f"{what}: files check"):
                    files_new()
                    files_parent()
                if res["new"] != res["old"]:
                    print(f"MISMATCH {what}: files -> files", flush=True)
                    sys.exit(1)
                row["host_form_files"] = k
                row["host_form_in_bytes"] = sum(len(f) for f in files)
                row["host_form_out_bytes"] = sum(len(f) for f in res["new"])
                row["host_form_image_bytes_not_allocated"] = sum(w * hh * 4 for (w, hh) in sizes[:k])
                res.clear()
                row["files_host_form"], row["files_host_form_parent"] = wall_compare(files_new, files_parent, args.warmup, args.reps, args.step_limit,
                                                                                      f"{what}: files -> files", StepLimit)
                row["files_not_slower"] = row["files_host_form"]["ms"] <= row["files_host_form_parent"]["ms"]
                del files, out_new, out_old
                res.clear()
            rows.append(row)
            print(json.dumps(row), flush=True)
            del out_a, out_b, vals, tw, th, slots
            torch.cuda.empty_cache()
    h.close()
    if hp is not None:
        hp.close()
    if hv is not None:
        hv.close()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
