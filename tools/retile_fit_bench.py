"""Fit a .pixlzr archive to a budget at a NEW block size on one MI355X, without the images, by the protocol of
tools/archive_fit_bench.py and tools/retile_ladder_bench.py.  The folder is tools/varied_bench.py's (256 RGBA images, sides
64 .. 4096 log-uniform), shrunk once to tiles / files at the source block at factor f -- the reference's usual factors and the
strongly shrunk files of tools/retile_bench.py, both modes -- then re-tiled at the destination block at the reference's 20 factors
(f times whole-folder.rs' sweep); Lanczos3 down and for both expands.  Pairs: 64x64 -> 32x32 (new tiles split tiles of the files),
32x32 -> 64x64 (merge), 32x32 -> 48x20 (straddle).  The directional rows take the images that leave no 1-px edge tile against
either grid; their count is in the row.

(a) the device call alone, on tiles in HBM: pxz_retile_distortion_varied_device against what defines it on the same build --
    pxz_expand_varied_frames_device of the archive at the source block into a packed image and
    pxz_distortion_varied_frames_device over the K * n descriptors at the new block -- the sets being the re-tile ladder's rungs.
    Device time from HIP events around the calls (their host-side planning and table uploads inside).
(b) the host forms, files to files: pxz_rate_distortion_retile_files, pxz_retile_varied_files_fit and
    pxz_retile_varied_files_fit_tiles against today's detour, pxz_decode_varied_files + the image form at the new block
    (pxz_rate_distortion_varied_images, pxz_encode_varied_images_fit, pxz_encode_varied_images_fit_tiles).  Wall clock: the calls
    are synchronous, uploads and downloads included.  Targets: each file's median length over the rungs.
    With --variant-lib, which names a build of this tree with -DPXZ_EXP=41 (make exp EXP=41: the host forms send a pair whose
    new block divides the files' block through the re-tile ladder and pxz_retile_distortion_varied_device, nothing of image
    size allocated), the same three forms of both builds besides, files to files: on such a pair that is the image path, which
    this tree takes, against the re-tile route -- the measurement that decided the host forms' rule.

Both sides of a comparison run in this one process, alternating, after >= 60 ms of untimed load and W steps of each; median and
every sample of --reps runs.  Every row is checked for equality before anything is timed.  Each timed step runs under a limit of
its own (--step-limit seconds): a step that exceeds it ends the process with status 124, and nothing else is started.

    python tools/retile_fit_bench.py [--images 256] [--host-images 256] [--reps 5] [--warmup 2] [--pairs 0,1,2] [--parts ab]
                                    [--variant-lib <build with -DPXZ_EXP=41>] [--json out.json]
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

K = 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--host-images", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--step-limit", type=float, default=120.0)
    ap.add_argument("--pairs", default="0,1,2", help="indices into retile_bench.PAIRS")
    ap.add_argument("--parts", default="ab", help="a: the device call, b: the host forms")
    ap.add_argument("--variant-lib", default=None, help="a build of this tree with -DPXZ_EXP=41: its host forms, which take the re-tile route "
                    "where the new block divides the files' block, are timed against this tree's")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    assert args.reps >= 5, "a median of fewer than 5 is not reported"

    VBIND = other_binding(args.variant_lib, "pxz_variant_binding")
    import torch
    import varied_bench as VB
    from transcode_bench import StepLimit, compare
    P = VB.P
    assert torch.cuda.is_available(), "this tool measures on the MI355X; there is nothing to report without one"
    h = P.Handle(0)
    hv = VBIND.Handle(0) if VBIND is not None else None
    buf, all_geoms = VB.folder(args.images, 2026)
    print(f"folder of {len(all_geoms)} RGBA images, {sum(g[0] * g[1] for g in all_geoms) / 1e6:.1f} Mpx", flush=True)
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
            factors = factors_of(f1, K)
            what = f"{sw}x{sh} -> {dw}x{dh} files at {label.split(' ->')[0]}"
            base = dict(pair=f"{sw}x{sh} -> {dw}x{dh}", mode=mode, files=label.split(" ->")[0], file_factor=f1, K=K, images=n)
            _, vals, tw, th, slots = h.shrink_varied_frames_device(buf, sw, sh, mode, FILTER, f1, descs=geoms, channels=4)
            torch.cuda.synchronize()

            if "a" in args.parts:
                T = int(P.varied_layout(geoms, dw, dh)[-1])
                _, _, ow, oh, rslots = h.retile_varied_ladder_frames_device(sizes, 4, sw, sh, dw, dh, mode, FILTER, factors, FILTER, tw, th, slots)
                packed, at = [], 0  # the image the old way needs: tightly packed, 256-byte aligned starts
                for (w, hh) in sizes:
                    packed.append((w, hh, w * 4, at))
                    at += (w * hh * 4 + 255) // 256 * 256
                image = torch.zeros(at, dtype=torch.uint8, device="cuda")
                new = torch.empty((K, n, 4), dtype=torch.int64, device="cuda")
                old = torch.empty((K * n, 4), dtype=torch.int64, device="cuda")
                flat = (ow.reshape(-1), oh.reshape(-1), rslots.reshape(K * T, dw * dh * 4))

                def run_new():
                    h.retile_distortion_varied_device(sizes, 4, sw, sh, dw, dh, FILTER, FILTER, tw, th, slots, ow, oh, rslots, out=(None, new))

                def run_old():
                    h.expand_varied_frames_device(packed, 4, sw, sh, FILTER, tw, th, slots, image)
                    h.distortion_varied_frames_device(image, dw, dh, FILTER, *flat, descs=packed * K, channels=4, out=(None, old))

                with StepLimit(args.step_limit, what + ": check"):
                    run_new(), run_old()
                    torch.cuda.synchronize()
                    ok = h.decode_status() == 0 and torch.equal(new.reshape(K * n, 4), old) and bool(new.any())
                if not ok:
                    print(f"MISMATCH {what}: device call", flush=True)
                    sys.exit(1)
                row = dict(base, part="a: device call", source_tiles=int(tw.numel()), tiles=T, image_bytes=at, exact=True,
                           lds_bytes=P.retile_distortion_lds_bytes(sw, sh, dw, dh, 4, FILTER, FILTER))
                row["new"], row["expand_plus_distortion"] = compare(torch, run_new, run_old, args.warmup, args.reps, args.step_limit, what + ": device call")
                row["old_over_new"] = round(row["expand_plus_distortion"]["ms"] / row["new"]["ms"], 3)
                keep(row)
                del image, new, old, flat, ow, oh, rslots
                torch.cuda.empty_cache()

            if "b" in args.parts:
                k = min(args.host_images, n)
                fo, fbuf = h.encode_varied_frames_device(sizes[:k], 4, sw, sh, vals, tw, th, slots)
                torch.cuda.synchronize()
                offs = fo.cpu().numpy()
                raw = fbuf[: int(offs[-1])].cpu().numpy()
                files = [raw[int(offs[i]):int(offs[i + 1])].tobytes() for i in range(k)]
                del fo, fbuf, raw, vals, tw, th, slots
                torch.cuda.empty_cache()
                with StepLimit(args.step_limit, what + ": targets"):
                    file_bytes, _ = h.rate_distortion_retile_files(files, dw, dh, mode, FILTER, FILTER, FILTER, factors)
                targets = [int(np.sort(file_bytes[:, i])[K // 2]) for i in range(k)]
                res = {}

                def decoded():
                    return h.decode_varied_files(files, 4, sw, sh, FILTER)[0]

                forms = {
                    "table": (lambda: res.__setitem__("new", h.rate_distortion_retile_files(files, dw, dh, mode, FILTER, FILTER, FILTER, factors)),
                              lambda: res.__setitem__("old", h.rate_distortion_varied_images(decoded(), dw, dh, mode, FILTER, FILTER, factors))),
                    "fit": (lambda: res.__setitem__("new", h.retile_varied_files_fit(files, dw, dh, mode, FILTER, FILTER, FILTER, factors, P.FIT_BYTES, targets)),
                            lambda: res.__setitem__("old", h.encode_varied_images_fit(decoded(), dw, dh, mode, FILTER, FILTER, factors, P.FIT_BYTES, targets))),
                    "fit_tiles": (lambda: res.__setitem__("new", h.retile_varied_files_fit_tiles(files, dw, dh, mode, FILTER, FILTER, FILTER, factors,
                                                                                                P.FIT_BYTES, targets)),
                                  lambda: res.__setitem__("old", h.encode_varied_images_fit_tiles(decoded(), dw, dh, mode, FILTER, FILTER, factors,
                                                                                                  P.FIT_BYTES, targets))),
                }
                for name, (new_form, old_form) in forms.items():
                    with StepLimit(args.step_limit, f"{what}: {name} check"):
                        new_form()
                        old_form()
                    same = all((np.asarray(x) == np.asarray(y)).all() if not isinstance(x, list) else x == y for x, y in zip(res["new"], res["old"]))
                    if not same:
                        print(f"MISMATCH {what}: host form {name}", flush=True)
                        sys.exit(1)
                    row = dict(base, part="b: host form", form=name, files_in=k, in_bytes=sum(len(f) for f in files),
                               image_bytes=sum(w * hh * 4 for (w, hh) in sizes[:k]), equal=True)
                    if name != "table":
                        row["out_bytes"] = sum(len(f) for f in res["new"][0])
                    res.clear()
                    row["new"], row["decode_plus_image_form"] = wall_compare(new_form, old_form, args.warmup, args.reps, args.step_limit,
                                                                             f"{what}: {name}", StepLimit)
                    row["old_over_new"] = round(row["decode_plus_image_form"]["ms"] / row["new"]["ms"], 3)
                    res.clear()
                    if hv is not None:
                        call = {"table": lambda x: x.rate_distortion_retile_files(files, dw, dh, mode, FILTER, FILTER, FILTER, factors),
                                "fit": lambda x: x.retile_varied_files_fit(files, dw, dh, mode, FILTER, FILTER, FILTER, factors, P.FIT_BYTES, targets),
                                "fit_tiles": lambda x: x.retile_varied_files_fit_tiles(files, dw, dh, mode, FILTER, FILTER, FILTER, factors, P.FIT_BYTES,
                                                                                       targets)}[name]
                        with StepLimit(args.step_limit, f"{what}: {name} variant check"):
                            mine, theirs = call(h), call(hv)
                        if not all((np.asarray(x) == np.asarray(y)).all() if not isinstance(x, list) else x == y for x, y in zip(mine, theirs)):
                            print(f"MISMATCH {what}: host form {name}, variant build", flush=True)
                            sys.exit(1)
                        del mine, theirs
                        row["new_again"], row["retile_route_build"] = wall_compare(lambda: call(h), lambda: call(hv), args.warmup, args.reps,
                                                                                 args.step_limit, f"{what}: {name} against the re-tile route", StepLimit)
                        row["retile_route_over_new"] = round(row["retile_route_build"]["ms"] / row["new_again"]["ms"], 3)
                    keep(row)
                del files
    h.close()
    if hv is not None:
        hv.close()


if __name__ == "__main__":
    main()
