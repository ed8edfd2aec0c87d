"""The re-tile ladder on one MI355X (how far can an archive be squeezed at another block size), by the protocol of
tools/retile_bench.py and tools/reshrink_ladder_bench.py.  Per row:

  tiles -> tiles   one pxz_retile_varied_ladder_frames_device call against (a) K calls of pxz_retile_varied_frames_device, one per
                   factor, and (b) pxz_expand_varied_frames_device at the source block + pxz_shrink_varied_ladder_frames_device at
                   the destination block -- the calls the host form made before -- all from the same decoded tiles (device time
                   from HIP events);
  files -> files   the host form pxz_transcode_varied_ladder_files of this tree against the same call of a library built from the
                   parent commit, which PXZ_LIB names (wall clock: the call is synchronous, uploads and downloads included).
                   Without PXZ_LIB this comparison is left out.  The yardstick is the parent's composition, never the new code.

The folder is tools/varied_bench.py's (256 RGBA images of 64-4096 px), first shrunk at the source block at factor f -- the
reference's usual factors and the strongly shrunk files of tools/retile_bench.py -- then re-tiled at the destination block at K
factors: f times the first K of the reference's sweep as tools/reshrink_ladder_bench.py picks them; Lanczos3 on both sides.
Pairs: 64x64 -> 32x32, 32x32 -> 64x64, 32x32 -> 48x20; K = 1, 2, 5, 20.  The directional rows take the images that leave no 1-px
edge tile against either grid; their count is in the row.

Both sides of a comparison run in this one process, alternating, after >= 60 ms of untimed load and W steps of each; median and
every sample of --reps runs.  Every rung of every row is checked bit for bit before anything is timed.  The bytes of the image
batch that the chained calls need and the ladder does not are printed beside the times: a fact of the calls' signatures, not a
measurement.  Each timed step runs under a limit of its own (--step-limit seconds): a step that exceeds it ends the process with
status 124, and nothing else is started.

    [PXZ_LIB=<parent build>] python tools/retile_ladder_bench.py [--images 256] [--host-images 256] [--reps 9] [--warmup 5]
                                 [--ks 1,2,5,20] [--pairs 0,1,2] [--variant-lib <another build of this tree>] [--json out.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from reshrink_ladder_bench import factors_of  # noqa: E402
from retile_bench import FACTORS, FILTER, PAIRS, other_binding, wall_compare  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--host-images", type=int, default=256)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--step-limit", type=float, default=120.0)
    ap.add_argument("--ks", default="1,2,5,20")
    ap.add_argument("--pairs", default="0,1,2", help="indices into retile_bench.PAIRS")
    ap.add_argument("--host-ks", default="5", help="the K of the files -> files rows")
    ap.add_argument("--variant-lib", default=None, help="another build of this tree; its re-tile ladder is timed against this tree's, "
                    "tiles -> tiles, after a check that both give the same bits")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    assert args.reps >= 5, "a median of fewer than 5 is not reported"
    ks = [int(k) for k in args.ks.split(",")]
    host_ks = [int(k) for k in args.host_ks.split(",") if k]

    PB = other_binding(os.environ.pop("PXZ_LIB", None), "pxz_parent_binding")
    VBIND = other_binding(args.variant_lib, "pxz_variant_binding")
    import torch
    import varied_bench as VB
    from transcode_bench import StepLimit, compare
    from varied_ladder_bench import same_rung
    P = VB.P
    assert torch.cuda.is_available(), "this tool measures on the MI355X; there is nothing to report without one"
    assert os.path.samefile(P.library_path(), os.path.join(ROOT, "pixlzr-rust_amd", "csrc", "libpixlzr_hip.so")), P.library_path()
    h = P.Handle(0)
    hp = None
    if PB is not None:
        assert not hasattr(PB.load_library(), "pxz_retile_varied_ladder_frames_device"), "PXZ_LIB must name a build of the parent commit"
        hp = PB.Handle(0)
    hv = VBIND.Handle(0) if VBIND is not None else None
    buf, all_geoms = VB.folder(args.images, 2026)
    img = torch.empty_like(buf)  # what expand-varied writes and the varied ladder reads back: the re-tile ladder allocates none of it
    print(f"folder of {len(all_geoms)} RGBA images, {sum(g[0] * g[1] for g in all_geoms) / 1e6:.1f} Mpx; "
          f"files -> files against {PB.library_path() if PB else 'nothing (no PXZ_LIB)'}", flush=True)
    rows = []

    def keep(row):
        rows.append(row)
        print(json.dumps(row), flush=True)
        if args.json:  # (kept current row by row: a step limit ends the process)
            with open(args.json, "w") as f:
                json.dump(rows, f, indent=1)

    for ((sw, sh), (dw, dh)) in [PAIRS[int(i)] for i in args.pairs.split(",")]:
        for (mode, f1, _, label) in FACTORS:
            geoms = [g for g in all_geoms if mode == 0 or (g[0] % dw != 1 and g[1] % dh != 1 and g[0] % sw != 1 and g[1] % sh != 1)]
            sizes = [(g[0], g[1]) for g in geoms]
            n = len(geoms)
            image_batch_bytes = sum(g[0] * g[1] * 4 for g in geoms)
            T = int(P.varied_layout(geoms, dw, dh)[-1])
            _, vals, tw, th, slots = h.shrink_varied_frames_device(buf, sw, sh, mode, FILTER, f1, descs=geoms, channels=4)
            torch.cuda.synchronize()
            src_place = torch.tensor([min(sw, w - x) * min(sh, hh - y) for (w, hh) in sizes for y in range(0, hh, sh) for x in range(0, w, sw)], device="cuda")
            stored_full = round(float((tw * th == src_place).float().mean()), 4)
            del src_place
            single = (torch.empty(T, dtype=torch.float32, device="cuda"), torch.empty(T, dtype=torch.int32, device="cuda"),
                      torch.empty(T, dtype=torch.int32, device="cuda"), torch.empty((T, dw * dh * 4), dtype=torch.uint8, device="cuda"))
            files = None
            for K in ks:
                factors = factors_of(f1, K)
                what = f"{sw}x{sh} -> {dw}x{dh} files at {label.split(' ->')[0]}, K = {K}"

                def outputs():
                    return (torch.empty((K, T), dtype=torch.float32, device="cuda"), torch.empty((K, T), dtype=torch.int32, device="cuda"),
                            torch.empty((K, T), dtype=torch.int32, device="cuda"), torch.empty((K, T, dw * dh * 4), dtype=torch.uint8, device="cuda"))
                out_a, out_b = outputs(), outputs()

                def run_ladder():
                    h.retile_varied_ladder_frames_device(sizes, 4, sw, sh, dw, dh, mode, FILTER, factors, FILTER, tw, th, slots, out=out_a)

                def run_k_calls():
                    for f in factors:
                        h.retile_varied_frames_device(sizes, 4, sw, sh, dw, dh, mode, FILTER, f, FILTER, tw, th, slots, out=single)

                def run_expand_ladder():
                    h.expand_varied_frames_device(geoms, 4, sw, sh, FILTER, tw, th, slots, img)
                    h.shrink_varied_ladder_frames_device(img, dw, dh, mode, FILTER, factors, descs=geoms, channels=4, out=out_b)

                with StepLimit(args.step_limit, what + ": check"):
                    run_ladder()
                    run_expand_ladder()
                    torch.cuda.synchronize()
                    ok = h.decode_status() == 0
                    for r, f in enumerate(factors):
                        h.retile_varied_frames_device(sizes, 4, sw, sh, dw, dh, mode, FILTER, f, FILTER, tw, th, slots, out=single)
                        torch.cuda.synchronize()
                        ok = ok and same_rung(tuple(x[r] for x in out_a), single, 4) and same_rung(tuple(x[r] for x in out_a), tuple(x[r] for x in out_b), 4)
                    key = (out_a[1].to(torch.int64) << 32) | out_a[2].to(torch.int64)
                    srt = torch.sort(key, dim=0).values
                    distinct = 1 + (srt[1:] != srt[:-1]).sum(dim=0) if K > 1 else torch.ones(T, dtype=torch.int64, device="cuda")
                    resamples = round(float(distinct.float().mean()), 3)
                    del key, srt, distinct
                if not ok:
                    print(f"MISMATCH {what}: tiles -> tiles", flush=True)
                    sys.exit(1)
                row = dict(pair=f"{sw}x{sh} -> {dw}x{dh}", mode=mode, files=label.split(" ->")[0], file_factor=f1, K=K, factors=[round(f, 5) for f in factors],
                           images=n, source_tiles=int(tw.numel()), tiles=T, image_batch_bytes=image_batch_bytes, share_stored_full=stored_full,
                           distinct_sizes_per_tile=resamples, bit_exact=ok, lds_bytes=P.retile_ladder_lds_bytes(sw, sh, dw, dh, 4, mode, FILTER),
                           retile_lds_bytes=P.retile_lds_bytes(sw, sh, dw, dh, mode, FILTER))
                row["ladder"], row["k_calls"] = compare(torch, run_ladder, run_k_calls, args.warmup, args.reps, args.step_limit, what + ": against K calls")
                row["ladder_again"], row["expand_plus_varied_ladder"] = compare(torch, run_ladder, run_expand_ladder, args.warmup, args.reps,
                                                                                args.step_limit, what + ": against expand + varied ladder")
                row["speedup_over_k_calls"] = round(row["k_calls"]["ms"] / row["ladder"]["ms"], 2)
                row["speedup_over_expand_plus_varied_ladder"] = round(row["expand_plus_varied_ladder"]["ms"] / row["ladder_again"]["ms"], 2)
                if hv is not None:
                    out_v = outputs()

                    def run_variant():
                        hv.retile_varied_ladder_frames_device(sizes, 4, sw, sh, dw, dh, mode, FILTER, factors, FILTER, tw, th, slots, out=out_v)

                    with StepLimit(args.step_limit, what + ": variant check"):
                        run_variant()
                        torch.cuda.synchronize()
                        same = all(same_rung(tuple(x[r] for x in out_v), tuple(x[r] for x in out_a), 4) for r in range(K))
                    if not same:
                        print(f"MISMATCH {what}: variant build", flush=True)
                        sys.exit(1)
                    row["ladder_third"], row["ladder_variant_build"] = compare(torch, run_ladder, run_variant, args.warmup, args.reps, args.step_limit,
                                                                               what + ": this tree's ladder against the variant build's")
                    del out_v
                del out_a, out_b
                torch.cuda.empty_cache()

                if hp is not None and K in host_ks:
                    # files -> files: the first host-images files, on the host, through both libraries' host forms
                    k = min(args.host_images, n)
                    if files is None:
                        fo, fbuf = h.encode_varied_frames_device(sizes[:k], 4, sw, sh, vals, tw, th, slots)
                        torch.cuda.synchronize()
                        offs = fo.cpu().numpy()
                        raw = fbuf[: int(offs[-1])].cpu().numpy()
                        files = [raw[int(offs[i]):int(offs[i + 1])].tobytes() for i in range(k)]
                        del fo, fbuf, raw
                    res = {}
                    with StepLimit(args.step_limit, what + ": files size"):
                        total = int(h.transcode_varied_ladder_files(files, dw, dh, mode, FILTER, factors, FILTER, sizes_only=True).sum())
                    out_new, out_old = np.empty(total + 4096, np.uint8), np.empty(total + 4096, np.uint8)

                    def files_new():
                        res["new"] = h.transcode_varied_ladder_files(files, dw, dh, mode, FILTER, factors, FILTER, out=out_new)

                    def files_parent():
                        res["old"] = hp.transcode_varied_ladder_files(files, dw, dh, mode, FILTER, factors, FILTER, out=out_old)

                    with StepLimit(args.step_limit, what + ": files check"):
                        files_new()
                        files_parent()
                    if res["new"] != res["old"]:
                        print(f"MISMATCH {what}: files -> files", flush=True)
                        sys.exit(1)
                    row["host_form_files"] = k
                    row["host_form_in_bytes"] = sum(len(f) for f in files)
                    row["host_form_out_bytes"] = total
                    row["host_form_image_bytes_not_allocated"] = sum(w * hh * 4 for (w, hh) in sizes[:k])
                    res.clear()
                    row["files_host_form"], row["files_host_form_parent"] = wall_compare(files_new, files_parent, args.warmup, args.reps, args.step_limit,
                                                                                          what + ": files -> files", StepLimit)
                    row["files_speedup"] = round(row["files_host_form_parent"]["ms"] / row["files_host_form"]["ms"], 2)
                    del out_new, out_old
                    res.clear()
                keep(row)
            del single, vals, tw, th, slots, files
            torch.cuda.empty_cache()
    h.close()
    if hp is not None:
        hp.close()
    if hv is not None:
        hv.close()


if __name__ == "__main__":
    main()
