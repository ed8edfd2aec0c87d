"""The varied ladder's ABI without a GPU: the library exports both entry points, the header declares the rung limit the
binding assumes, and the single-geometry ladder keeps its own."""
import os
import re


def header_text():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return open(os.path.join(root, "include", "pixlzr_hip.h")).read()


def test_library_exports_the_varied_ladder(product):
    L = product.load_library()
    for name in ("pxz_shrink_varied_ladder_frames_device", "pxz_rate_distortion_varied_images"):
        assert hasattr(L, name), name
        assert name in product.EXPORTED_SYMBOLS, name
        assert re.search(r"\bint\s+" + name + r"\s*\(", header_text()), name


def test_header_declares_the_varied_rung_limit(product):
    m = re.search(r"#define\s+PXZ_VARIED_LADDER_MAX_RUNGS\s+(\d+)u?\b", header_text())
    assert m, "PXZ_VARIED_LADDER_MAX_RUNGS is not defined"
    assert int(m.group(1)) == product.VARIED_LADDER_MAX_RUNGS == 32


def test_the_single_geometry_ladder_keeps_its_limit(product):
    m = re.search(r"#define\s+PXZ_LADDER_MAX_RUNGS\s+(\d+)u?\b", header_text())
    assert m and int(m.group(1)) == product.LADDER_MAX_RUNGS == 16
