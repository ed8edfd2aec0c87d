"""Batches of differently sized images without a GPU: pxz_varied_layout (the flat tile space of a batch) against pxz_grid, the
refused descriptors, and the (source size, level) table directories of varied_kernel, pinned as digests of the lines
pxz_tables_dump.bin prints with the argument `varied`."""
import collections
import hashlib
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "pixlzr-rust_amd", "csrc", "pxz_tables_dump.bin")

INVALID_ARG, UNSUPPORTED = -1, -5

# filter -> (directories, SHA-256 of their lines)
PINNED = {
    0: (11, "e281ee4bab48a3bfd5de28b70d4e87165e39fb7d7e195702a3b8950df6e9c786"),
    1: (11, "1f103555b5cde1469f1cd69c7e7262ae31c99f6d6f4d4b1699ec538ac9c518b3"),
    2: (11, "e460ca5f4e734353faf1ca89e501a04e5fdf92ccd3f2a9e186ad0c293ee3d453"),
    3: (11, "bc618be54a252fce170c4e7584e89070317d0787d24f99423d232e258013cbf3"),
    4: (11, "f41da553c79dd094aac38b76b30d852a8a65cf7c69eae59b5e291f7890a999c1"),
}


def layout(product, geoms, bw, bh):
    return product.varied_layout(geoms, bw, bh)


@pytest.mark.parametrize("seed", range(6))
def test_layout_is_the_sum_of_the_grids(product, seed):
    rng = np.random.default_rng(seed)
    bw, bh = [(16, 16), (32, 32), (64, 64), (48, 20), (37, 61), (1, 1)][seed]
    n = int(rng.integers(1, 300))
    geoms = []
    for i in range(n):
        kind = i % 4
        if kind == 0:
            w, h = 1, 1
        elif kind == 1:
            w, h = int(rng.integers(1, bw + 1)), int(rng.integers(1, bh + 1))  # smaller than one tile
        else:
            w, h = int(rng.integers(1, 3001)), int(rng.integers(1, 3001))
        geoms.append((w, h, w * 4 + int(rng.integers(0, 64)), int(rng.integers(0, 1 << 40))))
    offs = layout(product, geoms, bw, bh)
    expect = [0]
    for (w, h, _, _) in geoms:
        c, r = product.grid(w, h, bw, bh)
        expect.append(expect[-1] + c * r)
    assert offs.dtype == np.uint64 and offs.tolist() == expect


def test_layout_of_one_image_is_its_grid(product):
    for (w, h, bw, bh) in [(1, 1, 64, 64), (1080, 1617, 64, 64), (7680, 4320, 32, 32), (100, 1, 16, 16)]:
        c, r = product.grid(w, h, bw, bh)
        assert layout(product, [(w, h, w * 4, 0)], bw, bh).tolist() == [0, c * r]


@pytest.mark.parametrize("geoms,bw,bh,code", [
    ([(0, 10, 40, 0)], 16, 16, INVALID_ARG),                       # zero width
    ([(10, 10, 40, 0), (10, 0, 40, 0)], 16, 16, INVALID_ARG),      # zero height, second image
    ([(10, 10, 40, 0, 1)], 16, 16, INVALID_ARG),                   # reserved field set
    ([(10, 10, 40, 0)], 0, 16, INVALID_ARG),                       # zero block side
    ([(1 << 24 | 1, 10, 1 << 27, 0)], 16, 16, UNSUPPORTED),        # side above 2^24
    ([(1 << 24, 1 << 24, 1 << 26, 0)] * 2, 1, 1, UNSUPPORTED),     # more than 2^32 - 1 tiles in all
])
def test_layout_refuses_invalid_descriptors(product, geoms, bw, bh, code):
    with pytest.raises(product.PxzError) as e:
        layout(product, geoms, bw, bh)
    assert e.value.code == code


def test_layout_refuses_an_empty_batch(product):
    with pytest.raises(product.PxzError) as e:
        layout(product, [], 16, 16)
    assert e.value.code == INVALID_ARG


@pytest.fixture(scope="module")
def directories(product):
    product.build_library()
    r = subprocess.run([TOOL, "varied"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    sets = collections.defaultdict(list)
    for line in r.stdout.splitlines():
        family, filt = line.split()[:2]
        assert family == "varied"
        sets[int(filt.split("=")[1])].append(line)
    return sets


@pytest.mark.parametrize("filt", sorted(PINNED))
def test_directories_match_the_pinned_digest(directories, filt):
    lines = directories[filt]
    count, digest = PINNED[filt]
    assert len(lines) == count
    assert hashlib.sha256("".join(l + "\n" for l in lines).encode()).hexdigest() == digest, \
        f"the varied tables of filter {filt} changed"


def test_directory_holds_every_reduction_of_every_side(directories):
    """one entry per (side, level) whose reduced size differs from the side; nothing for sides the batch does not hold"""
    for lines in directories.values():
        for line in lines:
            f = dict(kv.split("=", 1) for kv in line.split()[1:])
            sides = [int(s) for s in f["sides"].split(",")]
            used = sum(1 for s in sides for m in range(1, 18) if max((s + (1 << m) - 1) >> m, 1) != s)
            assert int(f["used"]) == used, line
            assert int(f["n_dir"]) == (max(sides) + 1) * 18, line
