"""The decode side of varied batches without a GPU: pxz_file_header (the header query a caller fills its descriptors from)
against the oracle's reader, the refused files, and the (full size, stored size) table directories of varied_expand_kernel:
every table equal to the one build_expand_tables makes for a tile of that full size -- the tables expand_kernel reads, which
the GPU suite checks against the oracle -- and pinned as digests of the lines pxz_tables_dump.bin prints with the argument
`varied_expand`.  Also home of the tile generator the GPU tests of the varied reader share."""
import collections
import hashlib
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "pixlzr-rust_amd", "csrc", "pxz_tables_dump.bin")

INVALID_ARG = -1
SIDES = [64, 32, 20, 17, 5, 1]

# filter -> (lines of the varied directory: one for the set, one per (full, stored) pair; SHA-256 of them)
PINNED = {
    0: (134, "9afd000e5ca2a538a7332b5d2ea25fef915624fabb6834990144020078e2f190"),
    1: (134, "4553e6a6dfe0b189c9f97d28bc8385a4757076e434a439932e3f3fdbb5fa7f78"),
    2: (134, "78a2f722914d4f831208916672bdb50c3d882744b5e0a6a1cd5702a7359c38b7"),
    3: (134, "9721e33045cc8356f9e55cb418c86f03ca4f94ce402570d2bf0856c7861be1bf"),
    4: (134, "270e2f7d9e86abddca2679cd18d895b24cdcc9ace2f1c2309774d2e1f8f54bf5"),
}

FULL, HALVED, ANY = 0, 1, 2


def draw_tiles(rng, width, height, bw, bh, c, classes=None):
    """Stored tiles of one image, not taken from a shrinker (whose sizes would leave most resamples untested): per tile one of
    three classes -- the full place, a halving ceil(side / 2^m) on one or both axes, any size in 1 .. place on each axis --
    dealt evenly and shuffled (or as `classes` says: a batch deals them over all its tiles); random pixel bytes, alpha 255 in about half of the RGBA tiles; values as random 32-bit patterns.
    -> (values float32[n], tw uint32[n], th uint32[n], slots uint8[n, bw*bh*c], classes int[n])"""
    cols, rows = -(-width // bw), -(-height // bh)
    n = cols * rows
    if classes is None:
        classes = rng.permutation(np.arange(n) % 3)
    assert len(classes) == n
    vals = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32).view(np.float32)
    tw = np.zeros(n, np.uint32)
    th = np.zeros(n, np.uint32)
    slots = np.zeros((n, bw * bh * c), np.uint8)
    for t in range(n):
        ty, tx = divmod(t, cols)
        fw = bw if tx < cols - 1 else width - (cols - 1) * bw
        fh = bh if ty < rows - 1 else height - (rows - 1) * bh
        if classes[t] == FULL:
            w, h = fw, fh
        elif classes[t] == HALVED:
            which = int(rng.integers(0, 3))  # x, y, both
            mx = int(rng.integers(1, 8)) if which != 1 else 0
            my = int(rng.integers(1, 8)) if which != 0 else 0
            w, h = max(-(-fw // (1 << mx)), 1), max(-(-fh // (1 << my)), 1)
        else:
            w, h = int(rng.integers(1, fw + 1)), int(rng.integers(1, fh + 1))
        tw[t], th[t] = w, h
        px = rng.integers(0, 256, (w * h, c), dtype=np.uint8)
        if c == 4 and rng.integers(0, 2) == 0:
            px[:, 3] = 255
        slots[t, : w * h * c] = px.ravel()
    return vals, tw, th, slots, classes


def make_file(oracle, rng, width, height, bw, bh, c, filter_byte=0):
    """-> (.pixlzr bytes of the oracle's writer, the tiles they hold as draw_tiles returns them)"""
    tiles = draw_tiles(rng, width, height, bw, bh, c)
    vals, tw, th, slots, _ = tiles
    return oracle.encode_container(width, height, bw, bh, c, filter_byte, vals, None, tw, th, slots), tiles


def check_header(product, oracle, raw):
    d = oracle.decode_container(raw)
    got = product.file_header(raw)
    assert got == (d["width"], d["height"], d["bw"], d["bh"], int(d["tc"][0]), d["filter"]), got


def test_file_header_of_the_reference_files(product, oracle, golden_dir):
    for name in ("base.pixlzr", "Big-Ruscher.pix"):
        check_header(product, oracle, open(os.path.join(golden_dir, name), "rb").read())


@pytest.mark.parametrize("seed", range(10))
def test_file_header_of_written_files(product, oracle, seed):
    rng = np.random.default_rng(1000 + seed)
    bw, bh = [(16, 16), (32, 32), (64, 64), (48, 20), (37, 61)][seed % 5]
    width, height = [(1, 1), (bw - 1, bh), (bw + 1, bh + 1)][seed % 3] if seed < 3 else (int(rng.integers(1, 301)), int(rng.integers(1, 301)))
    c = 3 + seed % 2
    raw, _ = make_file(oracle, rng, width, height, bw, bh, c, filter_byte=seed % 5)
    check_header(product, oracle, raw)
    assert product.file_header(raw) == (width, height, bw, bh, c, seed % 5)


def test_file_header_refuses_what_decode_file_refuses(product, oracle):
    rng = np.random.default_rng(5)
    raw, _ = make_file(oracle, rng, 70, 40, 32, 32, 4)
    rows = 2
    first = 26 + 4 * rows
    bad = {
        "empty": b"",
        "shorter than the header": raw[:25],
        "ends inside the first record": raw[:first + 22],
        "wrong magic": b"QIXLZR" + raw[6:],
        "wrong version": raw[:8] + b"\x03" + raw[9:],
        "zero width": raw[:10] + bytes(4) + raw[14:],
        "zero height": raw[:14] + bytes(4) + raw[18:],
        "zero block width": raw[:18] + bytes(4) + raw[22:],
        "zero block height": raw[:22] + bytes(4) + raw[26:],
        "channel byte 5": raw[:first + 21] + b"\x05" + raw[first + 22:],
    }
    for what, data in bad.items():
        with pytest.raises(product.PxzError) as e:
            product.file_header(data)
        assert e.value.code == INVALID_ARG, what
    assert product.file_header(raw[:first + 23])[:2] == (70, 40)  # the header query needs no more than this


@pytest.fixture(scope="module")
def directories(product):
    product.build_library()
    r = subprocess.run([TOOL, "varied_expand"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    sets = collections.defaultdict(lambda: collections.defaultdict(list))
    for line in r.stdout.splitlines():
        family, filt = line.split()[:2]
        sets[int(filt.split("=")[1])][family].append(line)
    return sets


@pytest.mark.parametrize("filt", sorted(PINNED))
def test_every_table_is_the_single_geometry_table(directories, filt):
    """(full, stored) for every pair of the sides: starts, sizes, window, precision and coefficients of the varied directory's
    table equal those of build_expand_tables for a tile whose full size is that side"""
    mine, ref = directories[filt]["vexpand"], directories[filt]["expand1"]
    pairs = [(full, stored) for full in SIDES for stored in range(1, full)]
    assert len(mine) == len(ref) == len(pairs)
    for (full, stored), a, b in zip(pairs, mine, ref):
        fa = a.split()
        assert fa[2] == f"full={full}" and fa[3] == f"stored={stored}", a
        assert fa[1:] == b.split()[1:], f"filter {filt} {stored} -> {full}: {a} / {b}"


@pytest.mark.parametrize("filt", sorted(PINNED))
def test_directories_match_the_pinned_digest(directories, filt):
    lines = directories[filt]["vexpand-set"] + directories[filt]["vexpand"]
    count, digest = PINNED[filt]
    assert len(lines) == count
    assert hashlib.sha256("".join(l + "\n" for l in lines).encode()).hexdigest() == digest, \
        f"the varied expand tables of filter {filt} changed"


def test_the_new_argument_prints_only_its_own_families(directories):
    """the lines tests/test_tables_host.py and tests/test_varied_host.py pin come from other arguments; this one prints only
    its own three families"""
    for fams in directories.values():
        assert set(fams) == {"vexpand-set", "vexpand", "expand1"}
