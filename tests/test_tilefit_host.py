"""Fit to a budget per tile (pxz_fit_tiles_select and the calls around it), the part that needs no GPU: the symbols, the rule on
the host against a restatement written here with Python integers, properties of the result checked by exhaustion over every
assignment of small tables, the error codes, and pxz_tilefit_check.bin.  The tables built here are the inputs of the device
form's test too (tests/test_gpu_tilefit.py uploads them).

The rule (include/pixlzr_hip.h): candidate (t, r) has b = tile_bytes[r][t] and s = the sum over the channels of tile_sse[r][t];
usable when no channel is 2^64-1, s < 2^32 and b < 2^24.  pick(t, lambda) = the usable r with the smallest (s + lambda b, b, r).
B(lambda) = fixed + sum b(pick), S(lambda) = sum s(pick).  FIT_BYTES: lambda* = the smallest lambda in [0, 2^32] with B <= target
(none: 2^32 and bit 0); FIT_SSE: the largest with S <= target (none: 0 and bit 0).  Not missed: the uniform rungs usable for
every tile go through fit_select's rule; the group takes that rung (bit 2) when it is eligible and strictly better than the
pick at lambda*.  A tile with no usable candidate: choice 0, in no total, bit 1."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

from test_fit_host import FIT_BYTES, FIT_SSE, U64, select

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pixlzr_hip.h")
NAMES = ["pxz_fit_tiles_select", "pxz_record_bytes_varied_device", "pxz_fit_varied_tiles_device", "pxz_gather_varied_tile_rungs_device",
         "pxz_encode_varied_images_fit_tiles", "pxz_transcode_varied_files_fit_tiles"]
INVALID_ARG, UNSUPPORTED = -1, -5
LAMBDA_MAX = 2 ** 32
MISSED, NO_CANDIDATE, UNIFORM = 1, 2, 4
POISON32, POISON64 = 0xA5A5A5A5, 0xA5A5A5A5A5A5A5A5


# ---- the rule, in Python integers -----------------------------------------------------------------------------------------

def candidates(tile_bytes, tile_sse):
    """-> cands[t][r] = (s, b) or None; tile_bytes [K][T], tile_sse [K][T][C]"""
    K, T = len(tile_bytes), len(tile_bytes[0])
    out = []
    for t in range(T):
        row = []
        for r in range(K):
            ch = [int(x) for x in tile_sse[r][t]]
            s, b = sum(ch), int(tile_bytes[r][t])
            row.append(None if (U64 in ch or s >= 2 ** 32 or b >= 2 ** 24) else (s, b))
        out.append(row)
    return out


def pick(row, lam):
    keys = [(c[0] + lam * c[1], c[1], r) for r, c in enumerate(row) if c is not None]
    return min(keys)[2] if keys else None


def totals(cands, lam):
    """-> (sum b, sum s, choices) of the picks at lam; a tile without a candidate: choice 0, in no total"""
    b = s = 0
    choice = []
    for row in cands:
        r = pick(row, lam)
        choice.append(0 if r is None else r)
        if r is not None:
            s, b = s + row[r][0], b + row[r][1]
    return b, s, choice


def group_select(cands, fixed, criterion, target):
    """one group -> (choice, lambda, bytes, sse, flags).  The search for lambda* is written as the textbook bisection between
    a lambda that fails and one that fits, not as the library's halving of an interval."""
    flags = NO_CANDIDATE if any(all(c is None for c in row) for row in cands) else 0
    if criterion == FIT_BYTES:
        fits = lambda lam: fixed + totals(cands, lam)[0] <= target  # noqa: E731
        if not fits(LAMBDA_MAX):
            lam = LAMBDA_MAX
        elif fits(0):
            lam = 0
        else:
            bad, good = 0, LAMBDA_MAX
            while good - bad > 1:
                mid = (bad + good) // 2
                bad, good = (bad, mid) if fits(mid) else (mid, good)
            lam = good
    else:
        fits = lambda lam: totals(cands, lam)[1] <= target  # noqa: E731
        if not fits(0):
            lam = 0
        elif fits(LAMBDA_MAX):
            lam = LAMBDA_MAX
        else:
            good, bad = 0, LAMBDA_MAX
            while bad - good > 1:
                mid = (bad + good) // 2
                good, bad = (mid, bad) if fits(mid) else (good, mid)
            lam = good
    b, s, choice = totals(cands, lam)
    b += fixed
    if not fits(lam):
        return choice, lam, b, s, flags | MISSED
    K = len(cands[0])
    whole = [r for r in range(K) if all(row[r] is not None for row in cands)]
    if whole:
        ub = [[fixed + sum(row[r][1] for row in cands)] for r in whole]
        us = [[[sum(row[r][0] for row in cands)]] for r in whole]
        u_choice, u_flags = select(ub, us, criterion, [target])
        if not u_flags[0]:
            k = u_choice[0]
            u_b, u_s = ub[k][0], us[k][0][0]
            mine, theirs = ((s, b), (u_s, u_b)) if criterion == FIT_BYTES else ((b, s), (u_b, u_s))
            if theirs < mine:
                return [whole[k]] * len(cands), lam, u_b, u_s, flags | UNIFORM
    return choice, lam, b, s, flags


def select_tiles(t):
    """a table -> (choice[T], lambda[G], bytes[G], sse[G], flags[G]) as lists"""
    cands = candidates(t["tile_bytes"].tolist(), t["tile_sse"].tolist())
    off = t["offsets"]
    out = ([], [], [], [], [])
    for g in range(len(off) - 1):
        res = group_select(cands[off[g]:off[g + 1]], t["fixed"][g], t["criterion"], t["targets"][g])
        out[0].extend(res[0])
        for k in range(1, 5):
            out[k].append(res[k])
    return out


# ---- the tables -----------------------------------------------------------------------------------------------------------

def table(name, criterion, tiles, offsets, fixed, targets, channels=3, split=None):
    """tiles[t] = the candidates (bytes, sse) of tile t; the sse goes to channel 0 unless split[t][r] gives the channels (which
    may hold what makes a candidate unusable)"""
    T, K = len(tiles), len(tiles[0])
    tb = np.zeros((K, T), np.uint32)
    ts = np.zeros((K, T, channels), np.uint64)
    for t, cs in enumerate(tiles):
        assert len(cs) == K
        for r, (b, s) in enumerate(cs):
            tb[r, t] = b
            ts[r, t] = split[t][r] if split and split[t][r] is not None else [s] + [0] * (channels - 1)
    assert offsets[0] == 0 and offsets[-1] == T and len(fixed) == len(targets) == len(offsets) - 1
    return dict(name=name, criterion=criterion, tile_bytes=tb, tile_sse=ts, offsets=[int(x) for x in offsets], fixed=[int(x) for x in fixed],
                targets=[int(x) for x in targets])


# three candidates of which the middle one lies above the line between the other two: no lambda picks it, so two such tiles go
# from 20 bytes straight to 4 -- and one rung for both, the middle, fits a target of 12 with less error
HULL = [(10, 0), (6, 60), (2, 100)]


def directed_tables():
    out = []
    for crit in (FIT_BYTES, FIT_SSE):
        c = "bytes" if crit == FIT_BYTES else "sse"
        # one rung: nothing to choose, met and missed; a group of one tile
        out.append(table(f"K1-met-{c}", crit, [[(10, 10)]], [0, 1], [5], [15]))
        out.append(table(f"K1-missed-{c}", crit, [[(10, 10)]], [0, 1], [5], [9]))
        # targets 0 and 2^64-1, in four groups of three tiles
        tiles = [[(7, 3), (5, 9), (0, 12), (9, 0)], [(8, 1), (3, 7), (1, 30), (2, 29)], [(4, 4), (4, 4), (6, 2), (2, 6)]] * 4
        out.append(table(f"target-0-and-max-{c}", crit, tiles, [0, 3, 6, 9, 12], [0, 0, 30, 30], [0, U64, 0, U64]))
        # every byte total between the smallest and the largest as the target, one group each: lambda* moves through its range
        tiles = [[(40, 0), (22, 90), (9, 700), (3, 5000)], [(35, 10), (20, 50), (12, 2000), (11, 2100)], [(50, 1), (10, 3), (9, 999), (1, 10 ** 6)]]
        n = 12
        tg = [int(x) for x in (np.linspace(15 + 26, 125 + 26, n) if crit == FIT_BYTES else np.geomspace(11, 1_007_100, n))]
        out.append(table(f"sweep-of-targets-{c}", crit, tiles * n, list(range(0, 3 * n + 1, 3)), [26] * n, tg))
        # the largest usable values: s = 2^32-1 and b = 2^24-1 (a cost just below 2^57)
        big = [[(2 ** 24 - 1, 0), (1, 2 ** 32 - 1)], [(2 ** 24 - 1, 2 ** 32 - 1), (2 ** 24 - 2, 2 ** 32 - 1)]] * 2
        out.append(table(f"largest-usable-{c}", crit, big, [0, 2, 4], [2 ** 40, 0], [2 ** 40 + 2 ** 24, 2 ** 33] if crit == FIT_BYTES else [2 ** 32, 0]))
    # ties: equal cost at lambda = 0 (equal s): fewer bytes; equal cost and bytes: the lower index; rung 0 worse than the tied ones
    ties = [[(30, 5), (20, 5), (25, 5), (20, 5)], [(20, 8), (20, 4), (20, 6), (20, 4)], [(9, 9), (9, 9), (9, 9), (9, 9)],
            [(50, 50), (9, 9), (9, 9), (9, 9)]]
    out.append(table("ties-bytes", FIT_BYTES, ties, [0, 4], [0], [1000]))
    out.append(table("ties-sse", FIT_SSE, ties, [0, 1, 4], [0, 7], [5, 1000]))
    # equal cost at a lambda that is not 0: (s, b) = (10, 4) and (2, 8) cost the same at lambda = 2, where the fewer bytes win
    out.append(table("tie-at-lambda-2", FIT_BYTES, [[(4, 10), (8, 2)], [(4, 10), (8, 2)]], [0, 2], [0], [8]))
    # the sum over the channels decides, not one of them
    for ch, parts in ((3, [[9, 0, 0], [1, 5, 5], [0, 0, 10]]), (4, [[9, 0, 0, 1], [1, 4, 4, 4], [0, 12, 0, 0]])):
        tiles = [[(10, sum(p)) for p in parts]]
        out.append(table(f"uneven-channels-C{ch}-bytes", FIT_BYTES, tiles, [0, 1], [0], [10], channels=ch, split=[parts]))
        tiles = [[(30 - 10 * r, sum(p)) for r, p in enumerate(parts)]]
        out.append(table(f"uneven-channels-C{ch}-sse", FIT_SSE, tiles, [0, 1], [0], [sum(parts[0])], channels=ch, split=[parts]))
    # unusable candidates: a channel of all ones, s = 2^32 (as one channel, and only as the sum), b = 2^24; tile 3 has none usable.
    # Each would be the best of its tile if it counted.
    ones, half = [0, U64, 0], [2 ** 31, 2 ** 31, 0]
    tiles = [[(1, 0), (5, 50), (9, 9)], [(1, 0), (5, 50), (9, 9)], [(2 ** 24, 0), (7, 70), (1, 0)], [(2 ** 24, 0), (1, 0), (1, 0)], [(3, 3), (2, 9), (1, 99)]]
    split = [[ones, None, None], [[2 ** 32, 0, 0], None, None], [None, None, half], [None, ones, half], [None, None, None]]
    for crit, tg in ((FIT_BYTES, [1000, 25]), (FIT_SSE, [1000, 200])):
        out.append(table(f"unusable-{'bytes' if crit == FIT_BYTES else 'sse'}", crit, tiles * 2, [0, 5, 10], [4, 4], tg, split=split * 2))
    # one rung for the whole group wins (bit 2) -- and where it only ties with the pick at lambda*, it does not
    out.append(table("uniform-wins-bytes", FIT_BYTES, [HULL, HULL], [0, 2], [30], [42]))
    out.append(table("uniform-wins-sse", FIT_SSE, [HULL, HULL], [0, 2], [30], [120]))
    out.append(table("uniform-ties-bytes", FIT_BYTES, [HULL, HULL], [0, 2], [30], [50]))
    out.append(table("uniform-ties-sse", FIT_SSE, [HULL, HULL], [0, 2], [30], [200]))
    # 32 rungs, 300 groups of 1..7 tiles, 4 channels: ties and unusable candidates among them
    rng = np.random.default_rng(7)
    sizes = rng.integers(1, 8, 300)
    off = np.concatenate([[0], np.cumsum(sizes)])
    T = int(off[-1])
    tb = rng.integers(13, 400, (32, T)).astype(np.uint32)
    ts = rng.integers(0, 3000, (32, T, 4)).astype(np.uint64) // 7 * 7
    tb[rng.random((32, T)) < 0.02] = 2 ** 24
    ts[rng.random((32, T)) < 0.02, 1] = U64
    tb[:, 5] = 2 ** 24  # (one tile without a usable candidate)
    for crit in (FIT_BYTES, FIT_SSE):
        tg = [[0, U64, 40 * int(s), 120 * int(s), 2000 * int(s), 300, 4000][k % 7] for k, s in enumerate(sizes)]
        out.append(dict(name=f"K32-G300-{'bytes' if crit == FIT_BYTES else 'sse'}", criterion=crit, tile_bytes=tb, tile_sse=ts,
                        offsets=[int(x) for x in off], fixed=[26 + 4 * int(s) for s in sizes], targets=tg))
    # one group over everything
    for crit, tg in ((FIT_BYTES, 26 + 90 * T), (FIT_SSE, 3500 * T)):
        out.append(dict(name=f"K32-one-group-{'bytes' if crit == FIT_BYTES else 'sse'}", criterion=crit, tile_bytes=tb, tile_sse=ts, offsets=[0, T],
                        fixed=[26], targets=[tg]))
    return out


def random_tables(count=200, max_tiles=12, max_k=8):
    """small tables over a small value range: ties everywhere, a few unusable candidates"""
    rng = np.random.default_rng(11)
    out = []
    for k in range(count):
        K, G, ch = int(rng.integers(1, max_k + 1)), int(rng.integers(1, 4)), int(rng.integers(3, 5))
        sizes = rng.integers(1, max_tiles // 3 + 2, G)
        off = np.concatenate([[0], np.cumsum(sizes)])
        T = int(off[-1])
        tb = rng.integers(0, 7, (K, T)).astype(np.uint32)
        ts = rng.integers(0, 4, (K, T, ch)).astype(np.uint64)
        ts[rng.random((K, T)) < 0.08, 0] = U64
        out.append(dict(name=f"random-{k}", criterion=k % 2, tile_bytes=tb, tile_sse=ts, offsets=[int(x) for x in off],
                        fixed=[int(x) for x in rng.integers(0, 5, G)], targets=[int(x) for x in rng.integers(0, 30, G)]))
    return out


def run(product, t):
    return product.fit_tiles_select(t["offsets"], t["fixed"], t["tile_bytes"], t["tile_sse"], t["criterion"], t["targets"])


def check_table(t, got):
    exp = select_tiles(t)
    for what, g, e in zip(("choice", "lambda", "bytes", "sse", "flags"), got, exp):
        assert [int(x) for x in g] == e, (t["name"], what)


# ---- 1. exports and declarations ------------------------------------------------------------------------------------------

def test_symbols_are_exported_and_declared(product):
    """fails before the per-tile fit exists"""
    lib = product.load_library()
    text = open(HEADER).read()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert f"int {name}(" in text, name
        assert name in product.EXPORTED_SYMBOLS, name
    out = subprocess.run(["nm", "-D", "--defined-only", product.library_path()], capture_output=True, text=True, check=True).stdout
    for name in NAMES:
        assert f" T {name}" in out, name
    assert "#define PXZ_TILEFIT_LAMBDA_MAX 4294967296ull" in text and product.TILEFIT_LAMBDA_MAX == LAMBDA_MAX
    assert (product.TILEFIT_MISSED, product.TILEFIT_NO_CANDIDATE, product.TILEFIT_UNIFORM) == (MISSED, NO_CANDIDATE, UNIFORM)
    for method in ("record_bytes_varied_device", "fit_varied_tiles_device", "gather_varied_tile_rungs_device", "encode_varied_images_fit_tiles",
                   "transcode_varied_files_fit_tiles"):
        assert hasattr(product.Handle, method), method


# ---- 2. the rule ------------------------------------------------------------------------------------------------------------

def test_the_tables_hold_what_they_are_for():
    """A check of this file's own fixtures, not of the product: it runs no product code.  The expected results, from the
    Python rule, of the directed tables: each shows the case it was made for."""
    by_name = {t["name"]: t for t in directed_tables()}
    sel = lambda name: select_tiles(by_name[name])  # noqa: E731
    assert sel("K1-met-bytes") == ([0], [0], [15], [10], [0]) and sel("K1-missed-bytes") == ([0], [LAMBDA_MAX], [15], [10], [MISSED])
    assert sel("K1-met-sse") == ([0], [LAMBDA_MAX], [15], [10], [0]) and sel("K1-missed-sse") == ([0], [0], [15], [10], [MISSED])
    assert sel("ties-bytes")[0] == [1, 1, 0, 1] and sel("ties-bytes")[1] == [0]
    assert sel("ties-sse")[0] == [1, 1, 0, 1]
    choice, lam, b, s, fl = sel("tie-at-lambda-2")
    assert (choice, lam, b, s, fl) == ([0, 0], [2], [8], [20], [0])
    for ch in (3, 4):
        assert sel(f"uneven-channels-C{ch}-bytes")[0] == [0] and sel(f"uneven-channels-C{ch}-sse")[0] == [0]
    choice, lam, b, s, fl = sel("unusable-bytes")
    assert fl == [NO_CANDIDATE, NO_CANDIDATE] and choice[:5] == [2, 2, 1, 0, 0] and lam[0] == 0 and 0 < lam[1] < LAMBDA_MAX
    assert b[0] == 4 + 9 + 9 + 7 + 3 and s[0] == 9 + 9 + 70 + 3  # (tile 3 counts in neither)
    # (both tiles leave rung 0 for rung 2 at lambda = 13: 100 + 2 * 13 < 10 * 13; the pick at lambda* has 34 bytes and an error of 200)
    assert sel("uniform-wins-bytes") == ([1, 1], [13], [42], [120], [UNIFORM])
    assert sel("uniform-wins-sse") == ([1, 1], [12], [42], [120], [UNIFORM])
    assert sel("uniform-ties-bytes") == ([0, 0], [0], [50], [0], [0]) and sel("uniform-ties-sse") == ([2, 2], [LAMBDA_MAX], [34], [200], [0])
    assert sel("target-0-and-max-bytes")[4] == [MISSED, 0, MISSED, 0] and sel("target-0-and-max-sse")[4] == [MISSED, 0, MISSED, 0]
    for c in ("bytes", "sse"):
        lam = sel(f"sweep-of-targets-{c}")[1]
        assert len(set(lam)) >= 6 and any(0 < x < LAMBDA_MAX for x in lam), (c, lam)
        fl = sel(f"K32-G300-{c}")[4]
        assert {0, MISSED}.issubset(set(fl)) and sum(1 for f in fl if f & NO_CANDIDATE) == 1, c
        assert len(set(sel(f"K32-one-group-{c}")[0])) > 8 and 0 < sel(f"K32-one-group-{c}")[1][0] < LAMBDA_MAX
    assert by_name["K32-G300-sse"]["tile_bytes"].shape[0] == 32 and len(by_name["K32-G300-sse"]["offsets"]) == 301


@pytest.mark.parametrize("t", directed_tables(), ids=lambda t: t["name"])
def test_fit_tiles_select_on_directed_tables(product, t):
    check_table(t, run(product, t))


def test_fit_tiles_select_on_random_tables(product):
    tables = random_tables()
    assert len(tables) == 200
    seen = 0
    for t in tables:
        got = run(product, t)
        check_table(t, got)
        for f in got[4]:
            seen |= 8 if int(f) == 0 else int(f)
    assert seen == 15  # (met, missed, a tile without a candidate and one rung for all are all exercised)


# ---- 3. properties, by exhaustion over every assignment ---------------------------------------------------------------------

def test_properties_hold_against_every_assignment(product):
    """one group, T <= 5 tiles, K <= 4 rungs: all K^T assignments of usable candidates"""
    rng = np.random.default_rng(5)
    kept = uniform = missed = 0
    for k in range(150):
        K, T, crit = int(rng.integers(1, 5)), int(rng.integers(1, 6)), k % 2
        tb = rng.integers(0, 9, (K, T)).astype(np.uint32)
        ts = rng.integers(0, 5, (K, T, 3)).astype(np.uint64)
        fixed, target = int(rng.integers(0, 9)), int(rng.integers(0, 45))
        if k % 5 == 0:  # tiles whose middle rung no lambda picks: one rung for all can win
            K = 3
            tb, ts = np.zeros((K, T), np.uint32), np.zeros((K, T, 3), np.uint64)
            tb[:], ts[:, :, 0] = np.array([10, 6, 2])[:, None], np.array([0, 6, 10])[:, None]
            target = fixed + 6 * T + int(rng.integers(0, 3)) if crit == FIT_BYTES else 6 * T + int(rng.integers(0, 3))
        t = dict(name=f"exhaustive-{k}", criterion=crit, tile_bytes=tb, tile_sse=ts, offsets=[0, T], fixed=[fixed], targets=[target])
        choice, lam, gb, gs, fl = [x.tolist() for x in run(product, t)]
        cands = candidates(tb.tolist(), ts.tolist())
        every = [(fixed + sum(cands[i][r][1] for i, r in enumerate(a)), sum(cands[i][r][0] for i, r in enumerate(a)))
                 for a in itertools.product(range(K), repeat=T)]
        con, mini = (0, 1) if crit == FIT_BYTES else (1, 0)
        mine = (gb[0], gs[0])
        assert mine == (fixed + sum(cands[i][r][1] for i, r in enumerate(choice)), sum(cands[i][r][0] for i, r in enumerate(choice)))
        # missed <=> no assignment fits
        assert bool(fl[0] & MISSED) == (not any(a[con] <= target for a in every)), t["name"]
        # B is monotone over a sweep of lambda (and S the other way)
        sweep = [totals(cands, x)[:2] for x in (0, 1, 2, 3, 4, 6, 9, 20, 1000, 2 ** 31, LAMBDA_MAX)]
        assert all(p[0] >= q[0] and p[1] <= q[1] for p, q in zip(sweep, sweep[1:])), t["name"]
        if fl[0] & MISSED:
            missed += 1
            continue
        assert mine[con] <= target
        # never worse than fit_select on the group's uniform totals
        ub = [[fixed + int(tb[r].sum())] for r in range(K)]
        us = [[[int(ts[r].sum()), 0, 0]] for r in range(K)]
        u_choice, u_flags = product.fit_select(np.array(ub, np.uint64), np.array(us, np.uint64), crit, [target])
        if not u_flags[0]:
            u = (ub[int(u_choice[0])][0], us[int(u_choice[0])][0][0])
            assert (mine[mini], mine[con]) <= (u[mini], u[con]), t["name"]
        if fl[0] & UNIFORM:
            uniform += 1
            assert len(set(choice)) == 1
        else:
            kept += 1
            # the pick at lambda* is optimal for what it uses of the constrained quantity
            assert not any(a[con] <= mine[con] and a[mini] < mine[mini] for a in every), t["name"]
    assert kept > 40 and uniform > 0 and missed > 5


# ---- 4. error codes ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("what,code,kw", [
    ("null offsets", INVALID_ARG, dict(offsets=None)), ("null fixed", INVALID_ARG, dict(fixed=None)), ("null targets", INVALID_ARG, dict(targets=None)),
    ("null tile_bytes", INVALID_ARG, dict(tile_bytes=None)), ("null tile_sse", INVALID_ARG, dict(tile_sse=None)),
    ("null choice", INVALID_ARG, dict(null_out=0)), ("null lambda", INVALID_ARG, dict(null_out=1)), ("null bytes", INVALID_ARG, dict(null_out=2)),
    ("null sse", INVALID_ARG, dict(null_out=3)), ("null flags", INVALID_ARG, dict(null_out=4)),
    ("no groups", INVALID_ARG, dict(n_groups=0)), ("no factors", INVALID_ARG, dict(n_factors=0)), ("33 factors", INVALID_ARG, dict(n_factors=33)),
    ("2 channels", INVALID_ARG, dict(channels=2)), ("5 channels", INVALID_ARG, dict(channels=5)), ("unknown criterion", INVALID_ARG, dict(criterion=2)),
    ("criterion 2^32-1", INVALID_ARG, dict(criterion=2 ** 32 - 1)),
    ("offsets from 1", INVALID_ARG, dict(offsets=[1, 2, 4])), ("offsets descend", INVALID_ARG, dict(offsets=[0, 3, 2])),
    ("an empty group", INVALID_ARG, dict(offsets=[0, 0, 4])), ("an empty last group", INVALID_ARG, dict(offsets=[0, 4, 4])),
    ("2^32 candidates", UNSUPPORTED, dict(offsets=[0, 1, 2 ** 32 // 3 + 1]))], ids=lambda x: x if isinstance(x, str) else "")
def test_fit_tiles_select_errors_write_nothing(product, what, code, kw):
    K, G, T, ch = 3, 2, 4, 3
    args = dict(offsets=[0, 1, T], fixed=[1, 1], targets=[100, 100], tile_bytes=np.ones((K, T), np.uint32), tile_sse=np.ones((K, T, ch), np.uint64),
                n_groups=G, n_factors=K, channels=ch, criterion=FIT_BYTES)
    null_out = kw.pop("null_out", None)
    args.update(kw)
    outs = [np.full(T, POISON32, np.uint32), np.full(G, POISON64, np.uint64), np.full(G, POISON64, np.uint64), np.full(G, POISON64, np.uint64),
            np.full(G, POISON32, np.uint32)]
    u64 = lambda a: None if a is None else np.array(a, np.uint64)  # noqa: E731
    ptr = lambda a: None if a is None else C.c_void_p(a.ctypes.data)  # noqa: E731
    keep = [u64(args["offsets"]), u64(args["fixed"]), u64(args["targets"])]
    L = product.load_library()
    rc = L.pxz_fit_tiles_select(args["n_groups"], ptr(keep[0]), ptr(keep[1]), args["n_factors"], args["channels"], args["criterion"], ptr(keep[2]),
                                ptr(args["tile_bytes"]), ptr(args["tile_sse"]), *[None if null_out == k else ptr(o) for k, o in enumerate(outs)])
    assert rc == code, what
    assert all((o == (POISON32 if o.dtype == np.uint32 else POISON64)).all() for o in outs), what
    # the same arguments without the fault are taken
    good = [np.array([0, 1, T], np.uint64), np.array([1, 1], np.uint64), np.array([100, 100], np.uint64)]
    assert L.pxz_fit_tiles_select(G, ptr(good[0]), ptr(good[1]), K, ch, FIT_BYTES, ptr(good[2]), ptr(np.ones((K, T), np.uint32)),
                                  ptr(np.ones((K, T, ch), np.uint64)), *[ptr(o) for o in outs]) == 0
    assert (outs[0] == 0).all() and outs[2].tolist() == [2, 4] and outs[3].tolist() == [3, 9] and (outs[4] == 0).all()


# ---- 5. the rule's header on its own ------------------------------------------------------------------------------------------

def test_the_rule_holds_against_an_exhaustive_search_in_the_stand_alone_program():
    """pxz_tilefit_check.bin runs pxz_tilefit.h (the text the kernels run) on 400 small random tables, both criteria and eleven
    targets each, against every assignment of rungs"""
    tool = os.path.join(ROOT, "pixlzr-rust_amd", "csrc", "pxz_tilefit_check.bin")
    assert os.path.exists(tool), "run __graft_entry__.build()"
    r = subprocess.run([tool], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == f"ok {400 * 2 * 11}", r.stdout + r.stderr
