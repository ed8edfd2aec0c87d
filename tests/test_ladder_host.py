"""The factor ladder's ABI without a GPU: the library exports both entry points and the header declares the rung limit the
binding assumes."""
import os
import re


def test_library_exports_the_ladder(product):
    L = product.load_library()
    for name in ("pxz_shrink_ladder_frames_device", "pxz_shrink_image_ladder"):
        assert hasattr(L, name), name
        assert name in product.EXPORTED_SYMBOLS, name


def test_header_declares_the_rung_limit(product):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "pixlzr_hip.h")).read()
    m = re.search(r"#define\s+PXZ_LADDER_MAX_RUNGS\s+(\d+)u?\b", header)
    assert m, "PXZ_LADDER_MAX_RUNGS is not defined"
    assert int(m.group(1)) == product.LADDER_MAX_RUNGS == 16
