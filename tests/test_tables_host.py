"""The device table formats without a GPU.  pxz_tables_dump.bin runs the library's table builders (pxz_tables.h) over a
fixed sweep of tile geometries, ragged edges and filters, one line per table set with a hash of every array.  A digest of
those lines is pinned per (table family, filter): the values were recorded from the code before the builders moved out of
pxz_api.cpp, so a changed byte in any table or operand layout names its family and filter here."""
import collections
import hashlib
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "pixlzr-rust_amd", "csrc", "pxz_tables_dump.bin")

# (family, filter) -> (table sets, SHA-256 of their lines)
PINNED = {
    ("shrink", 0): (85, "44ce178fd386d3832fe7cf3c095f5911dc3cb5f38685b6f8f43dfcc5593e3cfd"),
    ("shrink", 1): (85, "9547200e927de213e14a324fc421da5fc8fed6680cf2afed6b9a3bbf83b5ff28"),
    ("shrink", 2): (85, "d82b4cc745f200cb2794a2adc0ae2472fb7ba3a92c42986dfa675fe975530024"),
    ("shrink", 3): (85, "858171c963c494eea3a4821173adf2dfb2738e163392c7bf7e7181ed19855060"),
    ("shrink", 4): (85, "b7d39c26c9533337eafe8e375dc1326fafbb921ba3e62536c8ce2a9b2bfe090d"),
    ("expand", 0): (77, "8ebf673e3b9b6579757da0a8118c4e3f4588bbdc29c29b4af8fee98384256ca8"),
    ("expand", 1): (77, "4bdea40ad3ea50e75c490995ea17d82439c1afa5c4e080666de1c818866759e5"),
    ("expand", 2): (77, "758134e7ced8c1a6ab6bc2d106f70f24163e700591518d869bd54aacd969b7d6"),
    ("expand", 3): (77, "2429fe8966ef2cdc3e672e2eb8d6257d59bb1cdfa2076a1f6e3792a49ad5248e"),
    ("expand", 4): (77, "33a0193376056e7ed6573f03a0b1888f2ae7d74e726d1784db1dd22ac3585073"),
    ("tree", 0): (15, "b26bae483b40ab89d795e076ce72f2aa71e848b487c26666c52fb80031fd865e"),
    ("tree", 1): (15, "721dc7820eef4724f4f685011760e78cf5717adf726c32ac12f7b12043862e7a"),
    ("tree", 2): (15, "44a1bf17635a230aeccbb39bb953b3e794d53d9a5bcdffdc227c87a04c4115f4"),
    ("tree", 3): (15, "c707e3c2b3865b055e5a2739b875dbafa470ac8cc3b38c68fde64b00e38c11fb"),
    ("tree", 4): (15, "00171654286d3fce0d8686db9db4ea442222f8f2fe4a46920d602827dfa050a4"),
}


@pytest.fixture(scope="module")
def table_sets(product):
    product.build_library()
    r = subprocess.run([TOOL], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    sets = collections.defaultdict(list)
    for line in r.stdout.splitlines():
        family, filt = line.split()[:2]
        sets[(family, int(filt.split("=")[1]))].append(line)
    return sets


def _fields(line):
    return dict(kv.split("=", 1) for kv in line.split()[1:])


@pytest.mark.parametrize("family,filt", sorted(PINNED), ids=lambda v: str(v))
def test_tables_match_the_pinned_digest(table_sets, family, filt):
    lines = table_sets[(family, filt)]
    count, digest = PINNED[(family, filt)]
    assert len(lines) == count
    assert hashlib.sha256("".join(l + "\n" for l in lines).encode()).hexdigest() == digest, \
        f"the {family} tables of filter {filt} changed"


def test_sweep_has_no_other_sets(table_sets):
    assert set(table_sets) == set(PINNED)


def test_operand_tables_go_to_the_matrix_core_tiles_only(table_sets):
    """Convolutions on 16x16, 32x32 and 64x64 tiles get matrix-core operands (AxisTab::mf_off on the shrink side, the 64x64
    blob, xmf / xmf16 / xmf64 on the expand side), at every ragged edge; Nearest and every other tile get none."""
    for (family, filt), lines in table_sets.items():
        for line in lines:
            f = _fields(line)
            conv = filt != 0
            if family == "shrink":
                assert (int(f["mf_tabs"]) > 0) == (conv and f["tile"] in ("16x16", "32x32", "64x64")), line
                assert (f["mf64"] != "-") == (conv and f["tile"] == "64x64"), line
            elif family == "expand":
                for key, tile in (("xmf", "32x32"), ("xmf16", "16x16"), ("xmf64", "64x64")):
                    assert (f[key] != "-") == (conv and f["tile"] == tile), line


def test_level_thresholds_are_the_oracles_breakpoints(product, oracle):
    """build_level_thresholds against the oracle's reduce_dims (operations.rs:145-151), bit for bit: with a side of 2^31 the
    reduced side is 2^(31-k) at the k-th threshold and half of that at the float just below it, and the level is constant over
    the 4096 bit patterns on either side."""
    import numpy as np
    product.build_library()
    r = subprocess.run([TOOL, "thresholds"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    bits = {}
    for line in r.stdout.splitlines():
        f = _fields(line)
        bits[int(f["k"])] = int(f["bits"], 16)
    assert sorted(bits) == list(range(32))
    side = 1 << 31

    def reduced(b):
        v = np.array([b], np.uint32).view(np.float32)[0]
        nw, nh, _ = oracle.reduce_dims(v, v, side, side)
        assert nw == nh
        return nw

    for k in range(31):
        t = bits[k]
        at, below = side >> k, side >> (k + 1)
        assert reduced(t) == at and reduced(t - 1) == below, (k, hex(t), reduced(t), reduced(t - 1))
        for d in range(1, 4097):
            assert reduced(t + d - 1) == at and reduced(t - d) == below, (k, hex(t), d)


def test_breakpoint_helpers_of_the_gpu_tests(oracle):
    """the bisection and the tile builder of tests/test_gpu_level_breakpoints.py need the oracle only: the same check here,
    where a broken helper shows without a GPU"""
    import test_gpu_level_breakpoints as helpers
    helpers.test_helper_finds_the_known_flips(oracle)
