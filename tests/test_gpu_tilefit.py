"""Fit to a budget per tile on the device (pxz_record_bytes_varied_device, pxz_fit_varied_tiles_device,
pxz_gather_varied_tile_rungs_device, pxz_encode_varied_images_fit_tiles, pxz_transcode_varied_files_fit_tiles).  Every comparison
is exact: the record bytes are what the writer's files and the oracle's hold; the device's choices, lambdas, totals and flags
equal pxz_fit_tiles_select on the downloaded tables; the gathered batch equals per-tile slices of the ladder's rungs -- value
bits, sizes, the valid slot bytes, and not a byte behind them; the host forms' files equal, byte for byte, the containers of the
tiles gathered on the host by the returned choices.  Every output is poisoned before each call, with a guard behind it that
must stay untouched."""
import ctypes as C

import numpy as np
import pytest

from test_fit_host import FIT_BYTES, FIT_SSE, U64
from test_gpu_fit import GATHER_CASES, OUT_POISON, POISON32, out_poisoned, out_still_poisoned, to_device_u64
from test_gpu_parity import assert_same_tiles
from test_gpu_varied import make_image, upload
from test_gpu_varied_ladder import FACTORS, POISON, host, poisoned, tile_geometry
from test_tilefit_host import LAMBDA_MAX, MISSED, NO_CANDIDATE, UNIFORM, candidates, check_table, directed_tables, random_tables, totals

pytestmark = pytest.mark.gpu

INVALID_ARG, UNSUPPORTED, BUFFER_TOO_SMALL = -1, -5, -7
POISON64 = 0x5A5A5A5A5A5A5A5A
DOWN, UP, FILTER_BYTE = 4, 2, 3


@pytest.fixture(scope="module")
def gpu(product):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    h = product.Handle(0)
    yield h
    h.close()


def last_error(gpu):
    return (gpu._L.pxz_last_error(gpu._h) or b"").decode()


def rows_of(sizes, bh):
    return [-(-h // bh) for (_, h) in sizes]


def groupings(n):
    """per image, the whole batch as one group, and an uneven split"""
    uneven = sorted({0, 1, n // 2 + 1, n})
    return {"per-image": None, "one-group": [0, n], "uneven": uneven}


def tables(gpu, product, images, c, bw, bh, mode, factors, guard=5):
    """one varied ladder with everything the per-tile fit reads of it: the rungs (device and host), the record bytes, the
    per-tile errors, the rung files' offsets; guards checked"""
    import torch
    sizes = [(i.shape[1], i.shape[0]) for i in images]
    n, Kf = len(images), len(factors)
    buf, geoms = upload(images, c, pad=3, misalign=5)
    T = int(product.varied_layout(geoms, bw, bh)[-1])
    out = poisoned((Kf, T), bw * bh * c, buf.device)
    gpu.shrink_varied_ladder_frames_device(buf, bw, bh, mode, DOWN, factors, descs=geoms, channels=c, out=out)
    flat = tuple(x.reshape((Kf * T,) + tuple(x.shape[2:])) for x in out)
    rec = torch.full((Kf * T + guard,), POISON32, dtype=torch.int32, device="cuda")
    offs = torch.full((Kf * n + 1 + guard,), POISON64, dtype=torch.int64, device="cuda")
    gpu.record_bytes_varied_device(sizes * Kf, c, bw, bh, *flat, out=(rec[:Kf * T], offs[:Kf * n + 1]))
    tile_sse, image_sse = gpu.distortion_varied_frames_device(buf, bw, bh, UP, flat[1], flat[2], flat[3], descs=geoms * Kf, channels=c)
    torch.cuda.synchronize()
    assert (rec[Kf * T:] == POISON32).all() and (offs[Kf * n + 1:] == POISON64).all(), "the guard behind an output was written"
    fw, fh, owner, _ = tile_geometry(geoms, bw, bh)
    tile0 = product.varied_layout(geoms, bw, bh).astype(np.int64)
    return dict(bw=bw, bh=bh, c=c, mode=mode, factors=factors, images=images, sizes=sizes, n=n, K=Kf, T=T, owner=owner, tile0=tile0, dev=out,
                flat=flat, host=host(out), d_rec=rec[:Kf * T].reshape(Kf, T), d_sse=tile_sse.reshape(Kf, T, c),
                rec=rec[:Kf * T].cpu().numpy().astype(np.uint32).reshape(Kf, T), sse=tile_sse.cpu().numpy().view(np.uint64).reshape(Kf, T, c),
                offs=offs[:Kf * n + 1].cpu().numpy().view(np.uint64), image_sse=image_sse.cpu().numpy().view(np.uint64).reshape(Kf, n, c),
                fixed=[26 + 4 * r for r in rows_of(sizes, bh)])


def case_images(bw, bh, c, sizes, mode):
    rng = np.random.default_rng(bw * 100 + bh + mode)
    if bw * bh < 64:  # (make_image's smooth areas are wider than these images: plain noise)
        return [rng.integers(0, 256, (h, w, c), dtype=np.uint8) for (w, h) in sizes]
    return [make_image(rng, w, h, c, ["partial", "opaque", "clear"][k % 3]) for k, (w, h) in enumerate(sizes)]


@pytest.fixture(scope="module", params=[(case, mode) for case in GATHER_CASES for mode in (0, 1)],
                ids=lambda p: f"{p[0][0]}x{p[0][1]}-c{p[0][2]}-{'by' if p[1] == 0 else 'dir'}")
def ladder(request, gpu, product):
    (bw, bh, c, sizes), mode = request.param
    return tables(gpu, product, case_images(bw, bh, c, sizes, mode), c, bw, bh, mode, FACTORS[mode])


@pytest.fixture(scope="module")
def big(gpu, product):
    """5x3 RGB blocks: 71 small images and one of 200x110 (1480 tiles) in the middle -- more than 64 groups, a group larger than
    any block of threads, groups that straddle waves"""
    rng = np.random.default_rng(99)
    sizes = [(int(rng.integers(2, 24)), int(rng.integers(2, 14))) for _ in range(71)]
    sizes.insert(40, (200, 110))
    images = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) // (1 + k % 4) * (1 + k % 4) for k, (w, h) in enumerate(sizes)]
    t = tables(gpu, product, images, 3, 5, 3, 0, FACTORS[0])
    assert t["n"] == 72 and int(np.diff(t["tile0"]).max()) == 1480 and t["T"] > 2000
    return t


# ---- 1. record bytes --------------------------------------------------------------------------------------------------------

def parse_records(data, cols, rows):
    """one .pixlzr file -> the bytes of its records, row-major (the line table is held against them)"""
    at = 26 + 4 * rows
    out = []
    for r in range(rows):
        start = at
        for _ in range(cols):
            assert data[at:at + 5] == b"block", "a record does not start where the one before it ended"
            ln = int.from_bytes(data[at + 9:at + 13], "big")
            out.append(data[at:at + 13 + ln])
            at += 13 + ln
        assert int.from_bytes(data[26 + 4 * r:30 + 4 * r], "big") == at - start, "line table"
    assert at == len(data)
    return out


def test_record_bytes_are_what_the_files_hold(gpu, product, oracle, ladder):
    import torch
    t = ladder
    bw, bh, c, n, Kf, T = t["bw"], t["bh"], t["c"], t["n"], t["K"], t["T"]
    e_offs, e_buf = gpu.encode_varied_frames_device(t["sizes"] * Kf, c, bw, bh, *t["flat"], filter_byte=FILTER_BYTE)
    torch.cuda.synchronize()
    e_offs, e_buf = e_offs.cpu().numpy().view(np.uint64), e_buf.cpu().numpy()
    assert (t["offs"] == e_offs).all(), "the optional offsets differ from the encoder's"
    vals, ow, oh, slots = t["host"]
    for r in range(Kf):
        for i, (w, h) in enumerate(t["sizes"]):
            k = r * n + i
            data = e_buf[int(e_offs[k]):int(e_offs[k + 1])].tobytes()
            a, b = int(t["tile0"][i]), int(t["tile0"][i + 1])
            ref = oracle.encode_container(w, h, bw, bh, c, FILTER_BYTE, vals[r, a:b], None, ow[r, a:b], oh[r, a:b], slots[r, a:b])
            assert data == ref, f"rung {r} image {i}: the writer's file differs from the oracle's"
            cols, rows = -(-w // bw), -(-h // bh)
            lens = [len(x) for x in parse_records(data, cols, rows)]
            assert t["rec"][r, a:b].tolist() == lens, f"rung {r} image {i}: record bytes"
            assert 26 + 4 * rows + int(t["rec"][r, a:b].sum()) == len(data) == int(e_offs[k + 1] - e_offs[k]), "the sum contract"
    # without the optional offsets: the same lengths
    rec = torch.full((Kf * T + 1,), POISON32, dtype=torch.int32, device="cuda")
    gpu.record_bytes_varied_device(t["sizes"] * Kf, c, bw, bh, *t["flat"], out=(rec[:Kf * T], None))
    torch.cuda.synchronize()
    assert (rec[:Kf * T].cpu().numpy().astype(np.uint32) == t["rec"].reshape(-1)).all() and int(rec[Kf * T]) == POISON32
    # the image sums are the tiles' (what makes group_sse the files' error)
    for i in range(n):
        a, b = int(t["tile0"][i]), int(t["tile0"][i + 1])
        assert (t["sse"][:, a:b].sum(axis=1) == t["image_sse"][:, i]).all()


# ---- 2. select --------------------------------------------------------------------------------------------------------------

def host_table(t, group_first, criterion, targets):
    gf = list(range(t["n"] + 1)) if group_first is None else group_first
    return dict(name="device", criterion=criterion, tile_bytes=t["rec"], tile_sse=t["sse"], offsets=[int(t["tile0"][i]) for i in gf],
                fixed=[sum(t["fixed"][gf[g]:gf[g + 1]]) for g in range(len(gf) - 1)], targets=targets)


def targets_from(t, group_first, criterion, kind):
    """targets taken from the tables, per group: the median of the uniform totals; exactly B(lambda) (S(lambda)) for lambda = 3;
    one below the least that any assignment gives (missed; an error of 0 cannot be undercut); 2^64-1"""
    ht = host_table(t, group_first, criterion, None)
    cands = candidates(t["rec"].tolist(), t["sse"].tolist())
    out = []
    for g, fixed in enumerate(ht["fixed"]):
        a, b = ht["offsets"][g], ht["offsets"][g + 1]
        if kind == "median":
            uni = sorted(fixed + int(t["rec"][r, a:b].sum()) if criterion == FIT_BYTES else int(t["sse"][r, a:b].sum()) for r in range(t["K"]))
            out.append(uni[len(uni) // 2])
        elif kind == "on-the-curve":
            tb, ts, _ = totals(cands[a:b], 3)
            out.append(fixed + tb if criterion == FIT_BYTES else ts)
        elif kind == "below":
            tb, ts, _ = totals(cands[a:b], LAMBDA_MAX if criterion == FIT_BYTES else 0)
            out.append(max((fixed + tb if criterion == FIT_BYTES else ts) - 1, 0))
        else:
            out.append(U64)
    return out


def device_select(gpu, t, group_first, criterion, targets, guard=3):
    """-> host (choice, lambda, bytes, sse, flags), every output poisoned before and the guards checked"""
    import torch
    G = t["n"] if group_first is None else len(group_first) - 1
    T = t["T"]
    choice = torch.full((T + guard,), POISON32, dtype=torch.int32, device="cuda")
    g64 = [torch.full((G + guard,), POISON64, dtype=torch.int64, device="cuda") for _ in range(3)]
    flags = torch.full((G + guard,), POISON32, dtype=torch.int32, device="cuda")
    gpu.fit_varied_tiles_device(t["sizes"], t["c"], t["bw"], t["bh"], t["d_rec"], t["d_sse"], criterion, targets, group_first=group_first,
                                out=(choice[:T],) + tuple(x[:G] for x in g64) + (flags[:G],))
    torch.cuda.synchronize()
    assert (choice[T:] == POISON32).all() and (flags[G:] == POISON32).all() and all((x[G:] == POISON64).all() for x in g64), \
        "the guard behind an output was written"
    return (choice[:T].cpu().numpy().astype(np.uint32),) + tuple(x[:G].cpu().numpy().view(np.uint64) for x in g64) + (
        flags[:G].cpu().numpy().astype(np.uint32),)


def check_select(gpu, product, t, python_too=False):
    seen = 0
    for name, gf in groupings(t["n"]).items():
        for criterion in (FIT_BYTES, FIT_SSE):
            for kind in ("median", "on-the-curve", "below", "max"):
                targets = targets_from(t, gf, criterion, kind)
                got = device_select(gpu, t, gf, criterion, targets)
                ht = host_table(t, gf, criterion, targets)
                exp = product.fit_tiles_select(ht["offsets"], ht["fixed"], ht["tile_bytes"], ht["tile_sse"], criterion, targets)
                for what, g, e in zip(("choice", "lambda", "bytes", "sse", "flags"), got, exp):
                    assert (g == e).all(), (name, criterion, kind, what)
                if python_too and kind == "median":
                    check_table(ht, got)
                fl = got[4]
                assert not (fl & NO_CANDIDATE).any()
                if kind == "below" and criterion == FIT_BYTES:
                    assert (fl & MISSED).all() and (got[1] == LAMBDA_MAX).all()
                if kind in ("max", "on-the-curve"):
                    assert not (fl & MISSED).any()
                if kind == "on-the-curve" and criterion == FIT_BYTES:
                    assert (got[1] <= 3).all()  # (B(3) fits, so the smallest lambda that fits is at most 3)
                if kind == "on-the-curve" and criterion == FIT_SSE:
                    assert (got[1] >= 3).all()
                for f in fl:
                    seen |= 8 if int(f) == 0 else int(f)
    return seen


def test_the_device_selects_what_the_host_selects(gpu, product, ladder):
    seen = check_select(gpu, product, ladder, python_too=True)
    assert seen & 8 and seen & MISSED


def test_the_device_selects_what_the_host_selects_over_many_groups(gpu, product, big):
    seen = check_select(gpu, product, big)
    assert seen & 8 and seen & MISSED


def test_the_device_selects_what_the_host_selects_on_directed_tables(gpu, product):
    """the tables of tests/test_tilefit_host.py as the device call takes them: every group one image of as many 4x4 blocks in a
    row as the group has tiles (so its fixed bytes are 30, and a byte target moves with them) -- unusable candidates, a tile
    without any, one rung for all, K = 1 and 32, 300 groups"""
    import torch
    seen = 0
    for t in directed_tables() + random_tables(60):
        off, G = t["offsets"], len(t["offsets"]) - 1
        Kf, T, c = t["tile_bytes"].shape[0], off[-1], t["tile_sse"].shape[2]
        sizes = [(4 * (off[g + 1] - off[g]), 4) for g in range(G)]
        targets = [x if (x == U64 or t["criterion"] == FIT_SSE) else max(x - t["fixed"][g] + 30, 0) for g, x in enumerate(t["targets"])]
        moved = dict(t, fixed=[30] * G, targets=targets)
        dev = dict(n=G, T=T, sizes=sizes, c=c, bw=4, bh=4, d_rec=torch.from_numpy(t["tile_bytes"].view(np.int32)).cuda(),
                   d_sse=to_device_u64(t["tile_sse"]))
        got = device_select(gpu, dev, None, t["criterion"], targets)
        exp = product.fit_tiles_select(off, moved["fixed"], t["tile_bytes"], t["tile_sse"], t["criterion"], targets)
        for what, g, e in zip(("choice", "lambda", "bytes", "sse", "flags"), got, exp):
            assert (g == e).all(), (t["name"], what)
        if T < 200:
            check_table(moved, got)
        for f in got[4]:
            seen |= 8 if int(f) == 0 else int(f)
    assert seen == 15  # (met, missed, a tile without a candidate and one rung for all: all of them on the device too)


# ---- 3. gather against per-tile slices ----------------------------------------------------------------------------------------

def gather(gpu, t, choice, want_pixels=True, flags=False, guard=3):
    import torch
    T, slot, n = t["T"], t["bw"] * t["bh"] * t["c"], t["n"]
    full = out_poisoned((T + guard,), slot, want_pixels)
    out = tuple(None if x is None else x[:T] for x in full)
    d_choice = torch.from_numpy(np.array(choice, np.uint32).view(np.int32)).cuda()
    d_flags = torch.full((n + 1,), POISON32, dtype=torch.int32, device="cuda") if flags else None
    gpu.gather_varied_tile_rungs_device(t["sizes"], t["c"], t["bw"], t["bh"], t["K"], d_choice, *t["dev"], out=out,
                                        image_flags=None if d_flags is None else d_flags[:n])
    torch.cuda.synchronize()
    assert out_still_poisoned(tuple(None if x is None else x[T:] for x in full)), "the guard behind the outputs was written"
    got_flags = None
    if flags:
        assert int(d_flags[n]) == POISON32, "the guard behind the flags was written"
        got_flags = d_flags[:n].cpu().numpy()
    return host(out), got_flags


def check_gather(t, got, rung_of_tile):
    vals, ow, oh, slots = t["host"]
    pick, k = np.array(rung_of_tile), np.arange(t["T"])
    gv, gw, gh, gs = got
    assert (gv.view(np.uint32) == vals[pick, k].view(np.uint32)).all(), "value bits"
    assert (gw == ow[pick, k]).all() and (gh == oh[pick, k]).all(), "sizes"
    if gs is not None:
        valid = np.arange(gs.shape[1])[None, :] < (gw.astype(np.int64) * gh * t["c"])[:, None]
        assert (gs[valid] == slots[pick, k][valid]).all(), "valid bytes"
        assert (gs[~valid] == OUT_POISON).all(), "a byte behind the valid ones was written"
        assert valid.any() and (~valid).any()
        assert (slots[pick, k][~valid] == POISON).all() and POISON != OUT_POISON


def test_gather_equals_per_tile_slices_of_the_rungs(gpu, ladder):
    t = ladder
    T, Kf = t["T"], t["K"]
    mixed = np.random.default_rng(T).integers(0, Kf, T).tolist()
    assert len(set(mixed[int(t["tile0"][0]):int(t["tile0"][1])])) > 1, "the first image takes one rung for all its tiles"
    for choice in ([0] * T, [Kf - 1] * T, mixed):
        got, _ = gather(gpu, t, choice)
        check_gather(t, got, choice)
    got, _ = gather(gpu, t, mixed, want_pixels=False)
    assert got[3] is None
    check_gather(t, got, mixed)
    # a choice beyond the ladder: the last rung, and bit 1 of the owning image's flag -- of no other
    beyond = list(mixed)
    last_image = t["n"] - 1
    beyond[0], beyond[int(t["tile0"][last_image + 1]) - 1] = Kf, 2 ** 32 - 1
    got, flags = gather(gpu, t, beyond, flags=True)
    read = list(beyond)
    read[0] = read[-1] = Kf - 1
    check_gather(t, got, read)
    assert flags.tolist() == [2] + [0] * (t["n"] - 2) + [2]


# ---- 4. the host forms --------------------------------------------------------------------------------------------------------

HOST_SIZES = [(150, 100), (9, 9), (70, 131), (100, 38), (66, 35)]
HOST_FACTORS = {0: [.25, .125, .5, 2, .05, .125, .5, .02], 1: [4, 2, 8, 32, .8, 2, 8, .32]}


def host_images(block, c, mode):
    rng = np.random.default_rng(block + 10 * c + mode)
    return [make_image(rng, w, h, c, ["partial", "opaque", "clear"][k % 3]) for k, (w, h) in enumerate(HOST_SIZES)]


def sse_between(a, b):
    return sum(int(((x.astype(np.int64) - y.astype(np.int64)) ** 2).sum()) for x, y in zip(a, b))


def group_runs(gf, n):
    gf = list(range(n + 1)) if gf is None else gf
    return [(gf[g], gf[g + 1]) for g in range(len(gf) - 1)]


@pytest.mark.parametrize("criterion", [FIT_BYTES, FIT_SSE], ids=["bytes", "sse"])
@pytest.mark.parametrize("mode", [0, 1], ids=["shrink_by", "directional"])
@pytest.mark.parametrize("block,c", [(32, 4), (16, 3)], ids=["32-rgba", "16-rgb"])
def test_files_equal_the_containers_of_the_chosen_tiles(gpu, product, oracle, block, c, mode, criterion):
    images, factors = host_images(block, c, mode), HOST_FACTORS[mode]
    n, Kf = len(images), len(factors)
    t = tables(gpu, product, images, c, block, block, mode, factors)
    vals, ow, oh, slots = t["host"]
    file_bytes, image_sse = np.diff(t["offs"].astype(np.int64)).reshape(Kf, n), t["image_sse"]
    for name, gf in groupings(n).items():
        runs = group_runs(gf, n)
        targets = targets_from(t, gf, criterion, "median")
        files, choice, lam, gb, gs, fl = gpu.encode_varied_images_fit_tiles(images, block, block, mode, DOWN, UP, factors, criterion, targets,
                                                                            group_first=gf, filter_byte=FILTER_BYTE)
        ht = host_table(t, gf, criterion, targets)
        exp = product.fit_tiles_select(ht["offsets"], ht["fixed"], ht["tile_bytes"], ht["tile_sse"], criterion, targets)
        for what, g, e in zip(("choice", "lambda", "bytes", "sse", "flags"), (choice, lam, gb, gs, fl), exp):
            assert (g == e).all(), (name, what)
        assert not fl.any() or set(fl.tolist()) <= {0, UNIFORM}, "a median target was missed"
        k = np.arange(t["T"])
        for i, img in enumerate(images):
            a, b = int(t["tile0"][i]), int(t["tile0"][i + 1])
            pick = choice[a:b].astype(np.int64)
            tiles = (vals[pick, k[a:b]], ow[pick, k[a:b]], oh[pick, k[a:b]], slots[pick, k[a:b]])
            ref = oracle.encode_container(img.shape[1], img.shape[0], block, block, c, FILTER_BYTE, tiles[0], None, *tiles[1:])
            assert files[i] == ref, f"{name} image {i}: differs from the oracle's container of the chosen tiles"
            assert files[i] == product.encode_container(img.shape[1], img.shape[0], block, block, c, FILTER_BYTE, tiles[0], None, *tiles[1:])
        decoded, _ = gpu.decode_varied_files(files, c, block, block, UP)
        for g, (i0, i1) in enumerate(runs):
            assert int(gb[g]) == sum(len(f) for f in files[i0:i1]), f"{name} group {g}: group_bytes"
            assert int(gs[g]) == sse_between(images[i0:i1], decoded[i0:i1]), f"{name} group {g}: group_sse"
        if gf is None:
            # against one factor per image under the same targets
            _, i_choice, i_flags = gpu.encode_varied_images_fit(images, block, block, mode, DOWN, UP, factors, criterion, targets,
                                                                filter_byte=FILTER_BYTE)
            for i in range(n):
                if fl[i] & MISSED:
                    assert i_flags[i] & 1, f"image {i}: the tile fit missed a target that one factor meets"
                if not i_flags[i] & 1:
                    ib, is_ = int(file_bytes[i_choice[i], i]), int(image_sse[i_choice[i], i].sum())
                    mine = (int(gs[i]), int(gb[i])) if criterion == FIT_BYTES else (int(gb[i]), int(gs[i]))
                    theirs = (is_, ib) if criterion == FIT_BYTES else (ib, is_)
                    assert mine[1] <= targets[i] and mine[0] <= theirs[0], f"image {i}: worse than one factor"


def test_one_factor_gives_the_files_of_encode_varied_images(gpu, product):
    images = host_images(32, 4, 0)
    for factor in (0.125, 2.0):
        files, choice, lam, gb, gs, fl = gpu.encode_varied_images_fit_tiles(images, 32, 32, 0, DOWN, UP, [factor], FIT_BYTES, [U64] * len(images),
                                                                            filter_byte=FILTER_BYTE)
        assert files == gpu.encode_varied_images(images, 32, 32, 0, DOWN, factor, filter_byte=FILTER_BYTE)
        assert not choice.any() and not fl.any() and [int(x) for x in gb] == [len(f) for f in files]


@pytest.mark.parametrize("criterion", [FIT_BYTES, FIT_SSE], ids=["bytes", "sse"])
@pytest.mark.parametrize("mode", [0, 1], ids=["shrink_by", "directional"])
def test_archive_files_are_the_chosen_records_of_the_rung_files(gpu, product, mode, criterion):
    """pxz_transcode_varied_files_fit_tiles: every output file is the header of its rung files, the records of the chosen rungs
    -- cut out of what pxz_transcode_varied_ladder_files writes -- and the line table that goes with them; the error is that
    against what the INPUT files decode to"""
    block, c, expand = 32, 4, 1
    images, factors = host_images(block, c, mode), HOST_FACTORS[mode]
    n = len(images)
    archive = gpu.encode_varied_images(images, block, block, mode, DOWN, [0.5, 8.0][mode], filter_byte=FILTER_BYTE)
    rung_files = gpu.transcode_varied_ladder_files(archive, block, block, mode, DOWN, factors, expand, filter_byte=FILTER_BYTE)
    now, _ = gpu.decode_varied_files(archive, c, block, block, expand)
    grids = [(-(-w // block), -(-h // block)) for (w, h) in HOST_SIZES]
    records = [[parse_records(rung_files[r][i], *grids[i]) for i in range(n)] for r in range(len(factors))]
    tile0 = product.varied_layout([(w, h, w * c, 0) for (w, h) in HOST_SIZES], block, block).astype(np.int64)
    for name, gf in groupings(n).items():
        runs = group_runs(gf, n)
        # per group the median of its uniform totals
        targets = []
        for (i0, i1) in runs:
            if criterion == FIT_BYTES:
                uni = sorted(sum(len(rung_files[r][i]) for i in range(i0, i1)) for r in range(len(factors)))
            else:
                uni = sorted(sse_between(now[i0:i1], gpu.decode_varied_files(rung_files[r][i0:i1], c, block, block, UP)[0]) for r in range(len(factors)))
            targets.append(uni[len(uni) // 2])
        files, choice, lam, gb, gs, fl = gpu.transcode_varied_files_fit_tiles(archive, block, block, mode, DOWN, expand, UP, factors, criterion,
                                                                              targets, group_first=gf, filter_byte=FILTER_BYTE)
        assert set(fl.tolist()) <= {0, UNIFORM}, "a median target was missed"
        for i in range(n):
            cols, rows = grids[i]
            recs = [records[int(choice[tile0[i] + k])][i][k] for k in range(cols * rows)]
            table = b"".join(sum(len(x) for x in recs[r * cols:(r + 1) * cols]).to_bytes(4, "big") for r in range(rows))
            assert files[i] == rung_files[0][i][:26] + table + b"".join(recs), f"{name} file {i}: not the chosen rungs' records"
        decoded, _ = gpu.decode_varied_files(files, c, block, block, UP)
        for g, (i0, i1) in enumerate(runs):
            assert int(gb[g]) == sum(len(f) for f in files[i0:i1]), f"{name} group {g}: group_bytes"
            assert int(gs[g]) == sse_between(now[i0:i1], decoded[i0:i1]), f"{name} group {g}: group_sse"
            con = int(gb[g]) if criterion == FIT_BYTES else int(gs[g])
            assert con <= targets[g]
    # a malformed file fails the whole call and writes nothing
    broken = list(archive)
    broken[2] = broken[2][:len(broken[2]) - 7]
    out = np.full(1 << 20, POISON, np.uint8)
    with pytest.raises(product.PxzError) as e:
        gpu.transcode_varied_files_fit_tiles(broken, block, block, mode, DOWN, expand, UP, factors, criterion, [U64] * n, out=out)
    assert e.value.code == INVALID_ARG and "image 2" in str(e.value) and (out == POISON).all()


# ---- 5. size query, errors, the handle ------------------------------------------------------------------------------------------

class RawFitTiles:
    """pxz_encode_varied_images_fit_tiles through ctypes, every output poisoned; fields may be overridden before call()"""

    def __init__(self, gpu, product, images, block_w, block_h, mode, factors, criterion, group_first, targets):
        self.gpu, self.product, n = gpu, product, len(images)
        self.images = [np.ascontiguousarray(i) for i in images]
        self.ch = self.images[0].shape[2]
        self.geoms = [(i.shape[1], i.shape[0], i.strides[0], 0) for i in self.images]
        self.block_w, self.block_h, self.mode, self.criterion = block_w, block_h, mode, criterion
        self.fac = np.ascontiguousarray(factors, np.float32)
        self.n_factors = self.fac.size
        self.gf = None if group_first is None else np.array(group_first, np.uint32)
        self.n_groups = n if group_first is None else len(group_first) - 1
        self.targets = np.array([int(t) for t in targets], np.uint64)
        G = max(self.n_groups, 1)
        self.offs = np.full(n + 1, U64, np.uint64)
        self.choice = np.full(4096, POISON32, np.uint32)
        self.g64 = [np.full(G + 4, U64, np.uint64) for _ in range(3)]
        self.flags = np.full(G + 4, POISON32, np.uint32)

    def call(self, out, capacity, null=()):
        ptr = lambda a: None if a is None else C.c_void_p(a.ctypes.data)  # noqa: E731
        n = len(self.images)
        ptrs = (C.c_void_p * n)(*[i.ctypes.data for i in self.images])
        descs = self.product.image_descs(self.geoms)
        outs = dict(offs=self.offs, choice=self.choice, lam=self.g64[0], gb=self.g64[1], gs=self.g64[2], flags=self.flags)
        o = [None if k in null else ptr(v) for k, v in outs.items()]
        return self.gpu._L.pxz_encode_varied_images_fit_tiles(
            self.gpu._h, C.cast(ptrs, C.c_void_p), C.cast(descs, C.c_void_p), n, self.ch, self.block_w, self.block_h, self.mode, DOWN, UP,
            None if "factors" in null else ptr(self.fac), self.n_factors, self.criterion, ptr(self.gf), self.n_groups,
            None if "targets" in null else ptr(self.targets), FILTER_BYTE, ptr(out), capacity, *o)

    def untouched(self):
        return bool((self.offs == U64).all() and (self.choice == POISON32).all() and (self.flags == POISON32).all() and
                    all((x == U64).all() for x in self.g64))


def test_size_query_then_exact_capacity(gpu, product):
    images, factors = host_images(32, 4, 0), HOST_FACTORS[0]
    gf, targets = [0, 2, 5], [9000, 20000]
    files, choice, lam, gb, gs, fl = gpu.encode_varied_images_fit_tiles(images, 32, 32, 0, DOWN, UP, factors, FIT_BYTES, targets, group_first=gf,
                                                                        filter_byte=FILTER_BYTE)
    total, T = sum(len(f) for f in files), len(choice)
    exp_offs = np.cumsum([0] + [len(f) for f in files]).astype(np.uint64)

    def same(raw):
        return ((raw.offs == exp_offs).all() and (raw.choice[:T] == choice).all() and (raw.choice[T:] == POISON32).all() and
                (raw.g64[0][:2] == lam).all() and (raw.g64[1][:2] == gb).all() and (raw.g64[2][:2] == gs).all() and (raw.flags[:2] == fl).all() and
                all((x[2:] == U64).all() for x in raw.g64) and (raw.flags[2:] == POISON32).all())

    for out, cap in ((None, 0), (None, 10 ** 9), (np.full(total, POISON, np.uint8), total - 1)):
        raw = RawFitTiles(gpu, product, images, 32, 32, 0, factors, FIT_BYTES, gf, targets)
        assert raw.call(out, cap) == BUFFER_TOO_SMALL, (cap, last_error(gpu))
        assert same(raw)
        assert out is None or (out == POISON).all(), "a call that was short of room wrote to out"
    raw = RawFitTiles(gpu, product, images, 32, 32, 0, factors, FIT_BYTES, gf, targets)
    out = np.full(total + 16, POISON, np.uint8)
    assert raw.call(out, total) == 0, last_error(gpu)
    assert out[:total].tobytes() == b"".join(files) and (out[total:] == POISON).all() and same(raw)
    # tile_choice is optional
    raw = RawFitTiles(gpu, product, images, 32, 32, 0, factors, FIT_BYTES, gf, targets)
    assert raw.call(out, total, null=("choice",)) == 0 and (raw.choice == POISON32).all() and (raw.offs == exp_offs).all()


def test_host_form_errors_write_nothing(gpu, product):
    images, factors = host_images(32, 4, 0)[:4], HOST_FACTORS[0]

    def refused(code, text=None, group_first=None, targets=(100,) * 4, null=(), images=images, block=(32, 32), factors=factors, **kw):
        raw = RawFitTiles(gpu, product, images, block[0], block[1], 0, factors, FIT_BYTES, group_first, targets)
        for key, v in kw.items():
            setattr(raw, key, v)
        out = np.full(1 << 20, POISON, np.uint8)
        assert raw.call(out, out.size, null=null) == code, (kw, null, last_error(gpu))
        assert raw.untouched() and (out == POISON).all(), (kw, null, "an error case wrote its outputs")
        assert text is None or text in last_error(gpu), last_error(gpu)

    refused(INVALID_ARG, criterion=2)
    refused(INVALID_ARG, null=("targets",))
    refused(INVALID_ARG, null=("factors",))
    for k in ("offs", "lam", "gb", "gs", "flags"):
        refused(INVALID_ARG, null=(k,))
    refused(INVALID_ARG, n_factors=0)
    refused(INVALID_ARG, factors=[1.0] * 33)
    refused(INVALID_ARG, factors=[0.5, float("nan")])
    refused(INVALID_ARG, "n_groups", n_groups=3)  # null group_first: every image its own group
    refused(INVALID_ARG, "group_first", group_first=[1, 2, 4], targets=(100, 100))
    refused(INVALID_ARG, "group_first", group_first=[0, 2, 3], targets=(100, 100))
    refused(INVALID_ARG, "group 1", group_first=[0, 2, 2, 4], targets=(100,) * 3)  # an empty group
    refused(INVALID_ARG, "group 1", group_first=[0, 3, 2, 4], targets=(100,) * 3)  # descending
    refused(INVALID_ARG, "n_groups", group_first=[0, 1, 2, 3, 4, 4], targets=(100,) * 5)  # more groups than images
    g = [(i.shape[1], i.shape[0], i.strides[0], 0) for i in images]
    refused(INVALID_ARG, "image 2", geoms=[g[0], g[1], g[2] + (1,), g[3]])  # reserved
    refused(UNSUPPORTED, block=(129, 128))  # 129*128*4 > 65536


def test_device_form_errors_write_nothing(gpu, product, ladder):
    import torch
    t = ladder
    n, T, Kf = t["n"], t["T"], t["K"]

    def fit_refused(code, sizes=None, block=None, c=None, group_first=None, targets=None, criterion=FIT_BYTES, **kw):
        G = n if group_first is None else len(group_first) - 1
        out = (torch.full((T,), POISON32, dtype=torch.int32, device="cuda"),) + tuple(
            torch.full((max(G, 1),), POISON64, dtype=torch.int64, device="cuda") for _ in range(3)) + (
            torch.full((max(G, 1),), POISON32, dtype=torch.int32, device="cuda"),)
        with pytest.raises(product.PxzError) as e:
            gpu.fit_varied_tiles_device(sizes or t["sizes"], c or t["c"], *(block or (t["bw"], t["bh"])), t["d_rec"], t["d_sse"], criterion,
                                        [100] * G if targets is None else targets or None, group_first=group_first, out=out, **kw)
        assert e.value.code == code, (kw, last_error(gpu))
        torch.cuda.synchronize()
        assert bool((out[0] == POISON32).all() and (out[4] == POISON32).all() and all((x == POISON64).all() for x in out[1:4])), "outputs written"

    fit_refused(INVALID_ARG, criterion=2)
    fit_refused(INVALID_ARG, targets=[])
    fit_refused(INVALID_ARG, n_factors=0)
    fit_refused(INVALID_ARG, n_factors=33)
    fit_refused(INVALID_ARG, c=5)
    fit_refused(INVALID_ARG, n_groups=n - 1)
    fit_refused(INVALID_ARG, group_first=[0, 1, 1, n])
    fit_refused(INVALID_ARG, group_first=[0, 1, n + 1])
    fit_refused(INVALID_ARG, block=(0, 16))
    fit_refused(UNSUPPORTED, block=(257, 256), c=3)  # 257*256*3 > 65536
    full = [(w, h, w * t["c"], 0) for (w, h) in t["sizes"]]
    fit_refused(INVALID_ARG, sizes=[full[0], full[1] + (1,)] + full[2:])
    assert "image 1" in last_error(gpu)

    def gather_refused(code, sizes=None, n_factors=Kf, c=None, block=None):
        out = out_poisoned((T,), t["bw"] * t["bh"] * t["c"])
        flags = torch.full((n,), POISON32, dtype=torch.int32, device="cuda")
        choice = torch.zeros(T, dtype=torch.int32, device="cuda")
        with pytest.raises(product.PxzError) as e:
            gpu.gather_varied_tile_rungs_device(sizes or t["sizes"], c or t["c"], *(block or (t["bw"], t["bh"])), n_factors, choice, *t["dev"], out=out,
                                                image_flags=flags)
        assert e.value.code == code, last_error(gpu)
        torch.cuda.synchronize()
        assert out_still_poisoned(out) and bool((flags == POISON32).all()), "an error case wrote its outputs"

    gather_refused(INVALID_ARG, n_factors=0)
    gather_refused(INVALID_ARG, n_factors=33)
    gather_refused(INVALID_ARG, c=5)
    gather_refused(INVALID_ARG, block=(0, 16))
    gather_refused(INVALID_ARG, sizes=[full[0], full[1] + (1,)] + full[2:])
    assert "image 1" in last_error(gpu)

    def record_refused(code, sizes=None, c=None, block=None):
        rec = torch.full((Kf * T,), POISON32, dtype=torch.int32, device="cuda")
        offs = torch.full((Kf * n + 1,), POISON64, dtype=torch.int64, device="cuda")
        with pytest.raises(product.PxzError) as e:
            gpu.record_bytes_varied_device(sizes or t["sizes"] * Kf, c or t["c"], *(block or (t["bw"], t["bh"])), *t["flat"], out=(rec, offs))
        assert e.value.code == code, last_error(gpu)
        torch.cuda.synchronize()
        assert bool((rec == POISON32).all() and (offs == POISON64).all()), "an error case wrote its outputs"

    record_refused(INVALID_ARG, c=5)
    record_refused(INVALID_ARG, block=(0, 16))
    record_refused(INVALID_ARG, sizes=[(0, 5)] + t["sizes"][1:] + t["sizes"] * (Kf - 1))
    with pytest.raises(product.PxzError) as e:
        gpu.record_bytes_varied_device(t["sizes"] * Kf, t["c"], t["bw"], t["bh"], *t["flat"], out=(None, None))
    assert e.value.code == INVALID_ARG


def test_the_handle_is_left_alone(gpu, product):
    import torch
    frames = gpu.synth_frames_device(2, 200, 328, 4, dist=product.DIST_ALPHA)
    images, factors = host_images(32, 4, 0)[:4], HOST_FACTORS[0]

    def single():
        vals, ow, oh, slots = host(gpu.shrink_frames_device(frames, 32, 32, 0, 4, 1.0))
        return vals.reshape(-1), ow.reshape(-1), oh.reshape(-1), slots.reshape(-1, slots.shape[-1])

    def calls():
        """the device calls on one ladder, then the host form -> what they returned"""
        t = tables(gpu, product, images, 4, 32, 32, 0, factors)
        got = list(device_select(gpu, t, [0, 1, 4], FIT_BYTES, [3000, 9000]))
        gathered, _ = gather(gpu, t, got[0].tolist())
        files = gpu.encode_varied_images_fit_tiles(images, 32, 32, 0, DOWN, UP, factors, FIT_SSE, [10 ** 5, 10 ** 6], group_first=[0, 1, 4])
        return [t["rec"], t["offs"]] + got + list(gathered) + [np.frombuffer(b"".join(files[0]), np.uint8)] + list(files[1:])

    single()  # (the first launch on a handle has no statistics of a launch before it)
    before, state = single(), gpu.state()
    first = calls()
    torch.cuda.synchronize()
    assert gpu.state() == state, "a tile-fit call changed what pxz_handle_state reports"
    assert_same_tiles(single(), before, 4, "the single-geometry call after the tile-fit calls")
    gpu.trim()
    again = calls()
    assert len(first) == len(again) == 17
    assert_same_tiles(tuple(again[7:11]), tuple(first[7:11]), 4, "the gather after a trim")
    for k in list(range(7)) + list(range(11, 17)):
        assert first[k].tobytes() == again[k].tobytes(), f"result {k} differs after a trim"
