"""The distortion calls' ABI without a GPU: the library exports the three entry points, and psnr() is the formula the header
leaves to the caller."""
import math

import numpy as np

NAMES = ("pxz_distortion_frames_device", "pxz_distortion_varied_frames_device", "pxz_rate_distortion_image")


def test_library_exports_the_distortion_calls(product):
    L = product.load_library()
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in product.EXPORTED_SYMBOLS, name


def test_handle_has_the_three_methods(product):
    for name in ("distortion_frames_device", "distortion_varied_frames_device", "rate_distortion_image"):
        assert callable(getattr(product.Handle, name)), name


def test_psnr_against_hand_computed_values(product):
    # every one of 3 samples off by 255: mse = 255^2 -> 0 dB; mse = 255^2 / 100 -> 20 dB
    assert product.psnr(3 * 255 * 255, 3) == 0.0
    assert abs(product.psnr(65025, 100) - 20.0) < 1e-12
    # 1000 samples, sse 4000: mse 4 -> 10 log10(65025 / 4) = 42.110204 dB
    assert abs(product.psnr(4000, 1000) - 10.0 * math.log10(16256.25)) < 1e-12
    assert abs(product.psnr(4000, 1000) - 42.110204) < 1e-6
    assert product.psnr(0, 1000) == math.inf
    both = product.psnr(np.array([0, 4000], np.uint64), 1000)
    assert both[0] == math.inf and abs(both[1] - 42.110204) < 1e-6
