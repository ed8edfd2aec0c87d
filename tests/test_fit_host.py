"""Fit to a budget (pxz_fit_select, pxz_fit_varied_ladder_device, pxz_gather_varied_rungs_device,
pxz_encode_varied_images_fit), the part that needs no GPU: the symbols, the selection rule on the host against a selection
written here with Python integers, its error codes, and sse_for_psnr.  The tables built here are the inputs of the device
form's test too (tests/test_gpu_fit.py uploads them), so each says what it holds.

The rule (include/pixlzr_hip.h): per image, bytes[r] and sse[r] = the sum over the channels.  FIT_BYTES: eligible when bytes <=
target, the smallest (sse, bytes, r) among the eligible, else the smallest (bytes, sse, r) and flag 1.  FIT_SSE: eligible when
sse <= target, the smallest (bytes, sse, r) among the eligible, else the smallest (sse, bytes, r) and flag 1."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pixlzr_hip.h")
NAMES = ["pxz_fit_select", "pxz_fit_varied_ladder_device", "pxz_gather_varied_rungs_device", "pxz_encode_varied_images_fit"]
FIT_BYTES, FIT_SSE = 0, 1
INVALID_ARG = -1
U64 = 2 ** 64 - 1
POISON = 0xA5A5A5A5


# ---- the rule, in Python integers -----------------------------------------------------------------------------------------

def select(file_bytes, sse, criterion, targets):
    """-> (choice, flags) as lists; file_bytes [K][n], sse [K][n][C], any integer type"""
    K, n = len(file_bytes), len(file_bytes[0])
    choice, flags = [], []
    for i in range(n):
        rungs = [(int(file_bytes[r][i]), sum(int(x) for x in sse[r][i]), r) for r in range(K)]
        if criterion == FIT_BYTES:
            eligible = [(s, b, r) for (b, s, r) in rungs if b <= int(targets[i])]
            fallback = [(b, s, r) for (b, s, r) in rungs]
        else:
            eligible = [(b, s, r) for (b, s, r) in rungs if s <= int(targets[i])]
            fallback = [(s, b, r) for (b, s, r) in rungs]
        choice.append(min(eligible)[2] if eligible else min(fallback)[2])
        flags.append(0 if eligible else 1)
    return choice, flags


# ---- the tables -----------------------------------------------------------------------------------------------------------

def table(name, criterion, rows, targets, split=None, channels=3):
    """rows[i] = the rungs (bytes, sse) of image i; the sse goes to channel 0 unless split[i][r] gives the channels"""
    n, K = len(rows), len(rows[0])
    fb = np.zeros((K, n), np.uint64)
    ss = np.zeros((K, n, channels), np.uint64)
    for i, rungs in enumerate(rows):
        assert len(rungs) == K
        for r, (b, s) in enumerate(rungs):
            fb[r, i] = b
            parts = split[i][r] if split else [s] + [0] * (channels - 1)
            assert len(parts) == channels and sum(parts) == s
            ss[r, i] = parts
    return dict(name=name, criterion=criterion, file_bytes=fb, sse=ss, targets=[int(t) for t in targets])


def directed_tables():
    out = []
    for crit in (FIT_BYTES, FIT_SSE):
        c = "bytes" if crit == FIT_BYTES else "sse"
        # one rung, one image: met, and missed
        out.append(table(f"K1-n1-met-{c}", crit, [[(10, 10)]], [10]))
        out.append(table(f"K1-n1-missed-{c}", crit, [[(10, 10)]], [9]))
        # targets 0 and 2^64-1: nothing but a zero is eligible; everything is
        rows = [[(7, 3), (5, 9), (0, 12), (9, 0)]] * 4
        out.append(table(f"target-0-and-max-{c}", crit, rows, [0, U64, 0, U64]))
        # above 2^32, near and above 2^63: a 32-bit or a signed comparison orders these wrongly
        big = [[(2 ** 32 + 5, 2 ** 63 + 5), (2 ** 32 - 1, 2 ** 63 + 9), (5, U64 - 3), (2 ** 63 + 7, 2 ** 33), (2 ** 63 - 7, 2 ** 33 + 1)]] * 6
        out.append(table(f"large-values-{c}", crit, big, [2 ** 32 + 5, 2 ** 63, 2 ** 63 + 6, 2 ** 33, U64, 4]))
    # ties, with the constrained quantity eligible everywhere (the minimised one decides, then the other, then the index)
    #   image 0: equal sse, different bytes       image 1: equal bytes, different sse
    #   image 2: both equal: the lowest index     image 3: the tie is among rungs 1..3 only, rung 0 is worse
    ties = [[(30, 5), (20, 5), (25, 5), (20, 5)], [(20, 8), (20, 4), (20, 6), (20, 4)], [(9, 9), (9, 9), (9, 9), (9, 9)],
            [(50, 50), (9, 9), (9, 9), (9, 9)]]
    out.append(table("ties-bytes", FIT_BYTES, ties, [100] * 4))
    out.append(table("ties-sse", FIT_SSE, ties, [100] * 4))
    # no rung eligible: the fallback's own order -- the constrained quantity first, then the other, then the index
    #   image 0: a single smallest       image 1: tied on the constrained, the other decides
    #   image 2: tied on both: rung 1, the lowest of the tied      image 3: what the eligible order would take (rung 0) loses
    miss_b = [[(30, 1), (20, 9), (25, 0)], [(20, 9), (20, 3), (20, 5)], [(40, 7), (20, 7), (20, 7)], [(30, 0), (20, 9), (21, 1)]]
    out.append(table("none-eligible-bytes", FIT_BYTES, miss_b, [19, 19, 0, 5]))
    miss_s = [[(b, s) for (s, b) in rungs] for rungs in miss_b]
    out.append(table("none-eligible-sse", FIT_SSE, miss_s, [19, 19, 0, 5]))
    # the sum over the channels decides, not one of them: channel 0 (and each single channel) orders the rungs the other way
    for ch, parts in ((3, [[[9, 0, 0], [1, 5, 5], [0, 0, 10]]]), (4, [[[9, 0, 0, 1], [1, 4, 4, 4], [0, 12, 0, 0]]])):
        rows = [[(10, sum(p)) for p in parts[0]]]
        out.append(table(f"uneven-channels-C{ch}-bytes", FIT_BYTES, rows, [10], split=parts, channels=ch))
        rows = [[(30 - 10 * r, sum(p)) for r, p in enumerate(parts[0])]]
        out.append(table(f"uneven-channels-C{ch}-sse", FIT_SSE, rows, [sum(parts[0][0])], split=parts, channels=ch))
    # 32 rungs, 300 images, 4 channels: every size at once, large values and frequent ties among them
    rng = np.random.default_rng(7)
    pool = [0, 1, 2, 3, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 40, 2 ** 61 - 1, 2 ** 61, 2 ** 61 + 1]
    fb = np.array(pool, np.uint64)[rng.integers(0, len(pool), (32, 300))]
    ss = np.array(pool, np.uint64)[rng.integers(0, len(pool), (32, 300, 4))]  # (four times 2^61 + 1 stays below 2^64)
    for crit in (FIT_BYTES, FIT_SSE):
        targets = [[0, U64, 2 ** 32, 2 ** 61, 2 ** 62 + 1, 2 ** 63 + 3, 3][k % 7] for k in range(300)]
        out.append(dict(name=f"K32-n300-{'bytes' if crit == FIT_BYTES else 'sse'}", criterion=crit, file_bytes=fb, sse=ss, targets=targets))
    return out


def random_tables(count=200):
    """small tables over a small value range: ties everywhere"""
    rng = np.random.default_rng(11)
    out = []
    for k in range(count):
        K, n, ch = int(rng.integers(1, 9)), int(rng.integers(1, 6)), int(rng.integers(3, 5))
        out.append(dict(name=f"random-{k}", criterion=k % 2, file_bytes=rng.integers(0, 6, (K, n)).astype(np.uint64),
                        sse=rng.integers(0, 3, (K, n, ch)).astype(np.uint64), targets=[int(t) for t in rng.integers(0, 9, n)]))
    return out


def check_table(t, got_choice, got_flags):
    exp_choice, exp_flags = select(t["file_bytes"].tolist(), t["sse"].tolist(), t["criterion"], t["targets"])
    assert [int(x) for x in got_choice] == exp_choice, (t["name"], "choice")
    assert [int(x) for x in got_flags] == exp_flags, (t["name"], "flags")


# ---- 1. exports and declarations ------------------------------------------------------------------------------------------

def test_symbols_are_exported_and_declared(product):
    """fails before the fit exists"""
    lib = product.load_library()
    text = open(HEADER).read()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert f"int {name}(" in text, name
        assert name in product.EXPORTED_SYMBOLS, name
    out = subprocess.run(["nm", "-D", "--defined-only", product.library_path()], capture_output=True, text=True, check=True).stdout
    for name in NAMES:
        assert f" T {name}" in out, name
    assert "PXZ_FIT_BYTES = 0" in text and "PXZ_FIT_SSE = 1" in text and "} pxz_fit;" in text
    assert (product.FIT_BYTES, product.FIT_SSE) == (FIT_BYTES, FIT_SSE)
    for method in ("fit_varied_ladder_device", "gather_varied_rungs_device", "encode_varied_images_fit"):
        assert hasattr(product.Handle, method), method


# ---- 2. the rule ------------------------------------------------------------------------------------------------------------

def test_the_tables_hold_what_they_are_for():
    """A check of this file's own fixtures, not of the product: it runs no product code (and passes without the feature).  The
    expected results, from the Python rule, of the directed tables: each shows the case it was made for."""
    by_name = {t["name"]: t for t in directed_tables()}
    sel = lambda name: select(by_name[name]["file_bytes"].tolist(), by_name[name]["sse"].tolist(), by_name[name]["criterion"],  # noqa: E731
                              by_name[name]["targets"])
    assert sel("ties-bytes") == ([1, 1, 0, 1], [0] * 4)  # equal sse: fewer bytes; equal bytes: the smaller sse; the index
    assert sel("ties-sse") == ([1, 1, 0, 1], [0] * 4)
    assert sel("none-eligible-bytes") == ([1, 1, 1, 1], [1] * 4)
    assert sel("none-eligible-sse") == ([1, 1, 1, 1], [1] * 4)
    assert sel("uneven-channels-C3-bytes") == ([0], [0]) and sel("uneven-channels-C4-bytes") == ([0], [0])
    # (by channel 0 alone every rung would be eligible, and the last, the shortest, would win)
    assert sel("uneven-channels-C3-sse") == ([0], [0]) and sel("uneven-channels-C4-sse") == ([0], [0])
    assert sel("target-0-and-max-bytes") == ([2, 3, 2, 3], [0] * 4) and sel("target-0-and-max-sse") == ([3, 2, 3, 2], [0] * 4)
    for name in ("K32-n300-bytes", "K32-n300-sse"):
        choice, flags = sel(name)
        assert 0 < sum(flags) < 300 and len(set(choice)) > 8, name
    assert by_name["K32-n300-sse"]["file_bytes"].shape == (32, 300) and by_name["K1-n1-met-sse"]["file_bytes"].shape == (1, 1)


@pytest.mark.parametrize("t", directed_tables(), ids=lambda t: t["name"])
def test_fit_select_on_directed_tables(product, t):
    check_table(t, *product.fit_select(t["file_bytes"], t["sse"], t["criterion"], t["targets"]))


def test_fit_select_on_random_tables(product):
    tables = random_tables()
    assert len(tables) == 200
    missed = 0
    for t in tables:
        choice, flags = product.fit_select(t["file_bytes"], t["sse"], t["criterion"], t["targets"])
        check_table(t, choice, flags)
        missed += int(flags.sum())
    assert missed > 20  # (the fallback is exercised too)


# ---- 3. error codes ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("what,kw", [
    ("null targets", dict(targets=None)), ("null file_bytes", dict(file_bytes=None)), ("null sse", dict(sse=None)),
    ("null choice", dict(null_out=0)), ("null fit_flags", dict(null_out=1)),
    ("no images", dict(n_images=0)), ("no factors", dict(n_factors=0)), ("33 factors", dict(n_factors=33)),
    ("2 channels", dict(channels=2)), ("5 channels", dict(channels=5)), ("unknown criterion", dict(criterion=2)),
    ("criterion 2^32-1", dict(criterion=2 ** 32 - 1))], ids=lambda x: x if isinstance(x, str) else "")
def test_fit_select_errors_write_nothing(product, what, kw):
    import ctypes as C
    K, n, ch = 3, 2, 3
    fb = np.ones((K, n), np.uint64)
    ss = np.ones((K, n, ch), np.uint64)
    tg = np.ones(n, np.uint64)
    choice, flags = np.full(n, POISON, np.uint32), np.full(n, POISON, np.uint32)
    ptr = lambda a: None if a is None else C.c_void_p(a.ctypes.data)  # noqa: E731
    args = dict(n_images=n, n_factors=K, channels=ch, criterion=FIT_BYTES, targets=tg, file_bytes=fb, sse=ss)
    null_out = kw.pop("null_out", None)
    args.update(kw)
    L = product.load_library()
    rc = L.pxz_fit_select(args["n_images"], args["n_factors"], args["channels"], args["criterion"], ptr(args["targets"]),
                          ptr(args["file_bytes"]), ptr(args["sse"]), None if null_out == 0 else ptr(choice),
                          None if null_out == 1 else ptr(flags))
    assert rc == INVALID_ARG, what
    assert (choice == POISON).all() and (flags == POISON).all(), what
    # the same arguments without the fault are taken
    assert L.pxz_fit_select(n, K, ch, FIT_BYTES, ptr(tg), ptr(fb), ptr(ss), ptr(choice), ptr(flags)) == 0
    assert (choice == 0).all() and (flags == 0).all()


# ---- 4. the gather's tile copy, on the host -----------------------------------------------------------------------------------

def test_the_tile_copy_writes_exactly_the_valid_bytes_at_every_alignment():
    """pxz_fit_check.bin runs gather_copy (pxz_fit.h: the text gather_rungs_kernel runs) lane by lane for all 256 pairs of
    source and destination alignments and 34 lengths, into a destination poisoned with what the source does not hold there,
    and holds gather_split against its alignment rules"""
    tool = os.path.join(ROOT, "pixlzr-rust_amd", "csrc", "pxz_fit_check.bin")
    assert os.path.exists(tool), "run __graft_entry__.build()"
    r = subprocess.run([tool], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == f"ok {16 * 16 * 34}", r.stdout + r.stderr


# ---- 5. sse_for_psnr --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("q", [10.0, 24.5, 30.0, 33.3, 40.0, 48.13, 60.0])
@pytest.mark.parametrize("n", [3, 27 * 31 * 3, 640 * 480 * 4, 4096 * 4096 * 3])
def test_sse_for_psnr_is_the_inverse_rounded_down(product, q, n):
    s = product.sse_for_psnr(q, n)
    assert isinstance(s, int) and 0 <= s <= U64
    assert product.psnr(s, n) >= q > product.psnr(s + 1, n), (q, n, s)
