"""ctypes binding of csrc/libpixlzr_hip.so (C ABI: include/pixlzr_hip.h)."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_HERE, "csrc")
_LIB_PATH = os.environ.get("PXZ_LIB") or os.path.join(_CSRC, "libpixlzr_hip.so")  # PXZ_LIB: diagnostic builds

FILTER_NEAREST, FILTER_TRIANGLE, FILTER_CATMULLROM, FILTER_GAUSSIAN, FILTER_LANCZOS3 = range(5)
MODE_SHRINK_BY, MODE_SHRINK_DIRECTIONALLY = 0, 1
DIST_OPAQUE, DIST_ALPHA, DIST_FLAT, DIST_NOISE = range(4)

# every symbol include/pixlzr_hip.h declares
EXPORTED_SYMBOLS = [
    "pxz_version", "pxz_device_count", "pxz_create", "pxz_destroy", "pxz_last_error", "pxz_set_stream",
    "pxz_synchronize", "pxz_grid", "pxz_shrink_image", "pxz_shrink_image_packed", "pxz_fetch_packed", "pxz_shrink_images", "pxz_shrink_images_packed", "pxz_shrink_frames_device", "pxz_lod_frames_device", "pxz_oklab_pixels_device",
    "pxz_pack_tiles_device", "pxz_encode_frames_device", "pxz_encode_container", "pxz_qoi_encode", "pxz_qoi_bound", "pxz_synth_frames_device", "pxz_axis_table",
    "pxz_enable_timing", "pxz_last_kernel_ms", "pxz_last_first_kernel_ms", "pxz_handle_state",
    "pxz_debug_read_work", "pxz_expand_frames_device", "pxz_expand_image", "pxz_decode_frames_device", "pxz_decode_file", "pxz_decode_status", "pxz_process_frames_device", "pxz_tree_process_frames_device", "pxz_trim", "pxz_debug_read_status",
    "pxz_shrink_ladder_frames_device", "pxz_shrink_image_ladder",
    "pxz_varied_layout", "pxz_shrink_varied_frames_device", "pxz_encode_varied_frames_device", "pxz_encode_varied_images",
    "pxz_file_header", "pxz_decode_varied_frames_device", "pxz_expand_varied_frames_device", "pxz_decode_varied_files",
    "pxz_distortion_frames_device", "pxz_distortion_varied_frames_device", "pxz_rate_distortion_image",
    "pxz_shrink_varied_ladder_frames_device", "pxz_rate_distortion_varied_images",
    "pxz_window_layout", "pxz_decode_windows_device", "pxz_expand_windows_device", "pxz_decode_windows_files",
    "pxz_reshrink_varied_frames_device", "pxz_reshrink_lds_bytes", "pxz_transcode_varied_files",
    "pxz_reshrink_varied_ladder_frames_device", "pxz_reshrink_ladder_lds_bytes", "pxz_transcode_varied_ladder_files",
    "pxz_fit_select", "pxz_fit_varied_ladder_device", "pxz_gather_varied_rungs_device", "pxz_encode_varied_images_fit",
    "pxz_reshrink_distortion_varied_device", "pxz_reshrink_distortion_lds_bytes", "pxz_rate_distortion_varied_files",
    "pxz_transcode_varied_files_fit",
    "pxz_fit_tiles_select", "pxz_record_bytes_varied_device", "pxz_fit_varied_tiles_device", "pxz_gather_varied_tile_rungs_device",
    "pxz_encode_varied_images_fit_tiles", "pxz_transcode_varied_files_fit_tiles",
    "pxz_retile_varied_frames_device", "pxz_retile_lds_bytes",
    "pxz_retile_varied_ladder_frames_device", "pxz_retile_ladder_lds_bytes",
    "pxz_retile_distortion_varied_device", "pxz_retile_distortion_lds_bytes", "pxz_rate_distortion_retile_files",
    "pxz_retile_varied_files_fit", "pxz_retile_varied_files_fit_tiles",
    "pxz_scaled_size", "pxz_scaled_axis_table", "pxz_expand_scaled_lds_bytes", "pxz_expand_varied_scaled_frames_device",
    "pxz_expand_windows_scaled_device", "pxz_decode_varied_files_scaled", "pxz_decode_windows_files_scaled",
    "pxz_patch_check", "pxz_patch_windows_device", "pxz_splice_windows_device", "pxz_patch_windows_files",
]
NO_WINDOW = 0xffffffff  # PXZ_NO_WINDOW

LADDER_MAX_RUNGS = 16  # PXZ_LADDER_MAX_RUNGS
VARIED_LADDER_MAX_RUNGS = 32  # PXZ_VARIED_LADDER_MAX_RUNGS
FIT_BYTES, FIT_SSE = 0, 1  # pxz_fit
TILEFIT_LAMBDA_MAX = 2 ** 32  # PXZ_TILEFIT_LAMBDA_MAX
TILEFIT_MISSED, TILEFIT_NO_CANDIDATE, TILEFIT_UNIFORM = 1, 2, 4  # bits of a group's flags (pxz_fit_tiles_select)

STATUS = {0: "PXZ_OK", -1: "PXZ_ERR_INVALID_ARG", -2: "PXZ_ERR_NO_DEVICE", -3: "PXZ_ERR_HIP",
          -4: "PXZ_ERR_TILE_TOO_SMALL", -5: "PXZ_ERR_UNSUPPORTED", -6: "PXZ_ERR_NOMEM",
          -7: "PXZ_ERR_BUFFER_TOO_SMALL", -8: "PXZ_ERR_INTERNAL"}


class PxzError(RuntimeError):
    def __init__(self, code, text=""):
        self.code = code
        super().__init__(f"{STATUS.get(code, code)}: {text}" if text else STATUS.get(code, str(code)))


class Frames(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("channels", C.c_uint32),
                ("pitch_bytes", C.c_uint32), ("n_frames", C.c_uint32), ("reserved", C.c_uint32),
                ("frame_stride_bytes", C.c_uint64)]


class Params(C.Structure):
    _fields_ = [("block_w", C.c_uint32), ("block_h", C.c_uint32), ("mode", C.c_uint32),
                ("filter", C.c_uint32), ("factor", C.c_float), ("reserved", C.c_uint32)]


class ImageDesc(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("pitch_bytes", C.c_uint32), ("reserved", C.c_uint32),
                ("offset_bytes", C.c_uint64)]


def image_descs(geoms):
    """(width, height, pitch_bytes, offset_bytes[, reserved]) tuples -> a ctypes array of pxz_image_desc."""
    arr = (ImageDesc * max(len(geoms), 1))()
    for i, g in enumerate(geoms):
        arr[i] = ImageDesc(g[0], g[1], g[2], g[4] if len(g) > 4 else 0, g[3])
    return arr


class Window(C.Structure):
    _fields_ = [("image", C.c_uint32), ("x", C.c_uint32), ("y", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32),
                ("pitch_bytes", C.c_uint32), ("offset_bytes", C.c_uint64)]


def window_descs(windows):
    """(image, x, y, width, height, pitch_bytes, offset_bytes) tuples -> a ctypes array of pxz_window."""
    arr = (Window * max(len(windows), 1))()
    for k, w in enumerate(windows):
        arr[k] = Window(*w)
    return arr


def library_path():
    return _LIB_PATH


def build_library(force=False):
    """hipcc --offload-arch=gfx950 (cross-compiles without a GPU)."""
    srcs = [os.path.join(_CSRC, f) for f in os.listdir(_CSRC)
            if f.endswith((".hip", ".cpp", ".h", ".inc")) or f == "Makefile"]
    srcs.append(os.path.join(os.path.dirname(_HERE), "include", "pixlzr_hip.h"))
    srcs.append(os.path.join(os.path.dirname(_HERE), "include", "pixlzr.hpp"))
    if (not force and os.path.exists(_LIB_PATH)
            and all(os.path.getmtime(_LIB_PATH) >= os.path.getmtime(s) for s in srcs)):
        return _LIB_PATH
    r = subprocess.run(["make", "-j8", "-C", _CSRC, "all"], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("building libpixlzr_hip.so failed:\n" + r.stdout + r.stderr)
    return _LIB_PATH


_lib = None


def load_library():
    """Loads the HIP library; raises if it is missing (no fallback of any kind)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB_PATH):
        raise ImportError(f"{_LIB_PATH} is missing: run __graft_entry__.build() (hipcc --offload-arch=gfx950)")
    try:  # share torch's HIP runtime when torch is in the process (same SONAME, must come first)
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(_LIB_PATH)
    vp, u32, f32 = C.c_void_p, C.c_uint32, C.c_float
    L.pxz_version.restype = C.c_char_p
    L.pxz_device_count.restype = C.c_int
    L.pxz_create.restype = C.c_int
    L.pxz_create.argtypes = [C.c_int, C.POINTER(vp)]
    L.pxz_destroy.restype = None
    L.pxz_destroy.argtypes = [vp]
    L.pxz_last_error.restype = C.c_char_p
    L.pxz_last_error.argtypes = [vp]
    L.pxz_set_stream.restype = C.c_int
    L.pxz_set_stream.argtypes = [vp, vp]
    L.pxz_synchronize.restype = C.c_int
    L.pxz_synchronize.argtypes = [vp]
    L.pxz_trim.restype = C.c_int
    L.pxz_trim.argtypes = [vp]
    L.pxz_grid.restype = C.c_int
    L.pxz_grid.argtypes = [u32] * 4 + [C.POINTER(u32)] * 2
    L.pxz_shrink_image.restype = C.c_int
    L.pxz_shrink_image.argtypes = [vp, vp] + [u32] * 8 + [f32] + [vp] * 4
    L.pxz_shrink_image_packed.restype = C.c_int
    L.pxz_shrink_image_packed.argtypes = [vp, vp] + [u32] * 8 + [f32] + [vp] * 4
    L.pxz_shrink_images.restype = C.c_int
    L.pxz_shrink_images.argtypes = [vp, vp] + [u32] * 9 + [f32] + [vp] * 4
    L.pxz_shrink_images_packed.restype = C.c_int
    L.pxz_shrink_images_packed.argtypes = [vp, vp] + [u32] * 9 + [f32] + [vp] * 4 + [C.c_uint64, vp]
    L.pxz_fetch_packed.restype = C.c_int
    L.pxz_fetch_packed.argtypes = [vp, vp, C.c_uint64]
    L.pxz_shrink_frames_device.restype = C.c_int
    L.pxz_shrink_frames_device.argtypes = [vp, C.POINTER(Frames), C.POINTER(Params)] + [vp] * 5
    L.pxz_shrink_ladder_frames_device.restype = C.c_int
    L.pxz_shrink_ladder_frames_device.argtypes = [vp, C.POINTER(Frames), C.POINTER(Params), vp, u32] + [vp] * 5
    L.pxz_shrink_image_ladder.restype = C.c_int
    L.pxz_shrink_image_ladder.argtypes = [vp, vp] + [u32] * 8 + [vp, u32] + [vp] * 4
    L.pxz_varied_layout.restype = C.c_int
    L.pxz_varied_layout.argtypes = [vp, u32, u32, u32, vp]
    L.pxz_shrink_varied_frames_device.restype = C.c_int
    L.pxz_shrink_varied_frames_device.argtypes = [vp, vp, u32, u32, C.POINTER(Params)] + [vp] * 5
    L.pxz_encode_varied_frames_device.restype = C.c_int
    L.pxz_encode_varied_frames_device.argtypes = [vp, vp, u32, u32, C.POINTER(Params), u32] + [vp] * 5 + [C.c_uint64, vp]
    L.pxz_encode_varied_images.restype = C.c_int
    L.pxz_encode_varied_images.argtypes = [vp, vp, vp, u32, u32, C.POINTER(Params), u32, vp, C.c_uint64, vp]
    if hasattr(L, "pxz_file_header"):  # (a build of an earlier commit named by PXZ_LIB lacks the varied decode side)
        L.pxz_file_header.restype = C.c_int
        L.pxz_file_header.argtypes = [vp, C.c_size_t] + [C.POINTER(u32)] * 6
        L.pxz_decode_varied_frames_device.restype = C.c_int
        L.pxz_decode_varied_frames_device.argtypes = [vp, vp, u32, u32, C.POINTER(Params)] + [vp] * 7
        L.pxz_expand_varied_frames_device.restype = C.c_int
        L.pxz_expand_varied_frames_device.argtypes = [vp, vp, u32, u32, C.POINTER(Params)] + [vp] * 5
        L.pxz_decode_varied_files.restype = C.c_int
        L.pxz_decode_varied_files.argtypes = [vp, vp, vp, vp, u32, u32, C.POINTER(Params), vp, vp]
    if hasattr(L, "pxz_distortion_frames_device"):  # (a build of an earlier commit named by PXZ_LIB lacks the distortion calls)
        L.pxz_distortion_frames_device.restype = C.c_int
        L.pxz_distortion_frames_device.argtypes = [vp, C.POINTER(Frames), C.POINTER(Params), u32] + [vp] * 6
        L.pxz_distortion_varied_frames_device.restype = C.c_int
        L.pxz_distortion_varied_frames_device.argtypes = [vp, vp, u32, u32, C.POINTER(Params)] + [vp] * 7
        L.pxz_rate_distortion_image.restype = C.c_int
        L.pxz_rate_distortion_image.argtypes = [vp, vp] + [u32] * 9 + [vp, u32, vp, vp]
    if hasattr(L, "pxz_window_layout"):  # (a build of an earlier commit named by PXZ_LIB lacks the windows)
        L.pxz_window_layout.restype = C.c_int
        L.pxz_window_layout.argtypes = [vp, u32, vp, u32, u32, u32, vp]
        L.pxz_decode_windows_device.restype = C.c_int
        L.pxz_decode_windows_device.argtypes = [vp, vp, u32, vp, u32, u32, C.POINTER(Params)] + [vp] * 7
        L.pxz_expand_windows_device.restype = C.c_int
        L.pxz_expand_windows_device.argtypes = [vp, vp, u32, vp, u32, u32, C.POINTER(Params)] + [vp] * 5
        L.pxz_decode_windows_files.restype = C.c_int
        L.pxz_decode_windows_files.argtypes = [vp, vp, vp, vp, u32, vp, u32, u32, C.POINTER(Params), vp, C.c_uint64, vp]
    if hasattr(L, "pxz_patch_check"):  # (a build of an earlier commit named by PXZ_LIB lacks the patch)
        L.pxz_patch_check.restype = C.c_int
        L.pxz_patch_check.argtypes = [vp, u32, vp, u32, u32, u32, vp, C.POINTER(u32)]
        L.pxz_patch_windows_device.restype = C.c_int
        L.pxz_patch_windows_device.argtypes = [vp, vp, u32, vp, u32, u32, C.POINTER(Params), u32] + [vp] * 9
        L.pxz_splice_windows_device.restype = C.c_int
        L.pxz_splice_windows_device.argtypes = [vp, vp, u32, vp, u32, u32, C.POINTER(Params)] + [vp] * 9 + [C.c_uint64, vp, vp]
        L.pxz_patch_windows_files.restype = C.c_int
        L.pxz_patch_windows_files.argtypes = [vp, vp, vp, u32, vp, u32, vp, C.POINTER(Params), u32, vp, C.c_uint64, vp]
    if hasattr(L, "pxz_shrink_varied_ladder_frames_device"):  # (a build of an earlier commit named by PXZ_LIB lacks the varied ladder)
        L.pxz_shrink_varied_ladder_frames_device.restype = C.c_int
        L.pxz_shrink_varied_ladder_frames_device.argtypes = [vp, vp, u32, u32, C.POINTER(Params), vp, u32] + [vp] * 5
        L.pxz_rate_distortion_varied_images.restype = C.c_int
        L.pxz_rate_distortion_varied_images.argtypes = [vp, vp, vp] + [u32] * 7 + [vp, u32, vp, vp]
    if hasattr(L, "pxz_reshrink_varied_frames_device"):  # (a build of an earlier commit named by PXZ_LIB lacks the re-shrink)
        L.pxz_reshrink_varied_frames_device.restype = C.c_int
        L.pxz_reshrink_varied_frames_device.argtypes = [vp, vp, u32, u32, C.POINTER(Params), u32] + [vp] * 8
        L.pxz_reshrink_lds_bytes.restype = C.c_int
        L.pxz_reshrink_lds_bytes.argtypes = [u32] * 4 + [C.POINTER(u32)]
        L.pxz_transcode_varied_files.restype = C.c_int
        L.pxz_transcode_varied_files.argtypes = [vp, vp, vp, u32, C.POINTER(Params), u32, u32, vp, C.c_uint64, vp]
    if hasattr(L, "pxz_reshrink_varied_ladder_frames_device"):  # (a build of an earlier commit named by PXZ_LIB lacks the re-shrink ladder)
        L.pxz_reshrink_varied_ladder_frames_device.restype = C.c_int
        L.pxz_reshrink_varied_ladder_frames_device.argtypes = [vp, vp, u32, u32, C.POINTER(Params), u32, vp, u32] + [vp] * 8
        L.pxz_reshrink_ladder_lds_bytes.restype = C.c_int
        L.pxz_reshrink_ladder_lds_bytes.argtypes = [u32] * 5 + [C.POINTER(u32)]
        L.pxz_transcode_varied_ladder_files.restype = C.c_int
        L.pxz_transcode_varied_ladder_files.argtypes = [vp, vp, vp, u32, C.POINTER(Params), u32, vp, u32, u32, vp, C.c_uint64, vp]
    if hasattr(L, "pxz_retile_varied_frames_device"):  # (a build of an earlier commit named by PXZ_LIB lacks the re-tile)
        L.pxz_retile_varied_frames_device.restype = C.c_int
        L.pxz_retile_varied_frames_device.argtypes = [vp, vp, u32, u32, u32, u32, C.POINTER(Params), u32] + [vp] * 8
        L.pxz_retile_lds_bytes.restype = C.c_int
        L.pxz_retile_lds_bytes.argtypes = [u32] * 6 + [C.POINTER(u32)]
    if hasattr(L, "pxz_retile_varied_ladder_frames_device"):  # (a build of an earlier commit named by PXZ_LIB lacks the re-tile ladder)
        L.pxz_retile_varied_ladder_frames_device.restype = C.c_int
        L.pxz_retile_varied_ladder_frames_device.argtypes = [vp, vp, u32, u32, u32, u32, C.POINTER(Params), u32, vp, u32] + [vp] * 8
        L.pxz_retile_ladder_lds_bytes.restype = C.c_int
        L.pxz_retile_ladder_lds_bytes.argtypes = [u32] * 7 + [C.POINTER(u32)]
    if hasattr(L, "pxz_fit_select"):  # (a build of an earlier commit named by PXZ_LIB lacks the fit)
        L.pxz_fit_select.restype = C.c_int
        L.pxz_fit_select.argtypes = [u32] * 4 + [vp] * 5
        L.pxz_fit_varied_ladder_device.restype = C.c_int
        L.pxz_fit_varied_ladder_device.argtypes = [vp] + [u32] * 4 + [vp] * 5
        L.pxz_gather_varied_rungs_device.restype = C.c_int
        L.pxz_gather_varied_rungs_device.argtypes = [vp, vp, u32, u32, C.POINTER(Params), u32] + [vp] * 10
        L.pxz_encode_varied_images_fit.restype = C.c_int
        L.pxz_encode_varied_images_fit.argtypes = [vp, vp, vp] + [u32] * 7 + [vp, u32, u32, vp, u32, vp, C.c_uint64] + [vp] * 5
    if hasattr(L, "pxz_retile_distortion_varied_device"):  # (a build of an earlier commit named by PXZ_LIB lacks the archive fit at a new block)
        L.pxz_retile_distortion_varied_device.restype = C.c_int
        L.pxz_retile_distortion_varied_device.argtypes = [vp, vp, u32, u32, u32, u32, C.POINTER(Params), u32, u32] + [vp] * 9
        L.pxz_retile_distortion_lds_bytes.restype = C.c_int
        L.pxz_retile_distortion_lds_bytes.argtypes = [u32] * 7 + [C.POINTER(u32)]
        L.pxz_rate_distortion_retile_files.restype = C.c_int
        L.pxz_rate_distortion_retile_files.argtypes = [vp, vp, vp, u32, C.POINTER(Params), u32, u32, vp, u32, vp, vp]
        L.pxz_retile_varied_files_fit.restype = C.c_int
        L.pxz_retile_varied_files_fit.argtypes = [vp, vp, vp, u32, C.POINTER(Params), u32, u32, vp, u32, u32, vp, u32, vp, C.c_uint64] + [vp] * 5
        L.pxz_retile_varied_files_fit_tiles.restype = C.c_int
        L.pxz_retile_varied_files_fit_tiles.argtypes = ([vp, vp, vp, u32, C.POINTER(Params), u32, u32, vp, u32, u32, vp, u32, vp, u32, vp,
                                                         C.c_uint64] + [vp] * 6)
    if hasattr(L, "pxz_reshrink_distortion_varied_device"):  # (a build of an earlier commit named by PXZ_LIB lacks the archive fit)
        L.pxz_reshrink_distortion_varied_device.restype = C.c_int
        L.pxz_reshrink_distortion_varied_device.argtypes = [vp, vp, u32, u32, C.POINTER(Params), u32, u32] + [vp] * 9
        L.pxz_reshrink_distortion_lds_bytes.restype = C.c_int
        L.pxz_reshrink_distortion_lds_bytes.argtypes = [u32] * 5 + [C.POINTER(u32)]
        L.pxz_rate_distortion_varied_files.restype = C.c_int
        L.pxz_rate_distortion_varied_files.argtypes = [vp, vp, vp, u32, C.POINTER(Params), u32, u32, vp, u32, vp, vp]
        L.pxz_transcode_varied_files_fit.restype = C.c_int
        L.pxz_transcode_varied_files_fit.argtypes = [vp, vp, vp, u32, C.POINTER(Params), u32, u32, vp, u32, u32, vp, u32, vp, C.c_uint64] + [vp] * 5
    if hasattr(L, "pxz_fit_tiles_select"):  # (a build of an earlier commit named by PXZ_LIB lacks the per-tile fit)
        L.pxz_fit_tiles_select.restype = C.c_int
        L.pxz_fit_tiles_select.argtypes = [u32, vp, vp, u32, u32, u32] + [vp] * 8
        L.pxz_record_bytes_varied_device.restype = C.c_int
        L.pxz_record_bytes_varied_device.argtypes = [vp, vp, u32, u32, C.POINTER(Params)] + [vp] * 6
        L.pxz_fit_varied_tiles_device.restype = C.c_int
        L.pxz_fit_varied_tiles_device.argtypes = [vp, vp, u32, u32, C.POINTER(Params), vp, u32, u32, u32] + [vp] * 8
        L.pxz_gather_varied_tile_rungs_device.restype = C.c_int
        L.pxz_gather_varied_tile_rungs_device.argtypes = [vp, vp, u32, u32, C.POINTER(Params), u32] + [vp] * 10
        L.pxz_encode_varied_images_fit_tiles.restype = C.c_int
        L.pxz_encode_varied_images_fit_tiles.argtypes = ([vp, vp, vp] + [u32] * 7 + [vp, u32, u32, vp, u32, vp, u32, vp, C.c_uint64]
                                                         + [vp] * 6)
        L.pxz_transcode_varied_files_fit_tiles.restype = C.c_int
        L.pxz_transcode_varied_files_fit_tiles.argtypes = ([vp, vp, vp, u32, C.POINTER(Params), u32, u32, vp, u32, u32, vp, u32, vp, u32, vp,
                                                            C.c_uint64] + [vp] * 6)
    L.pxz_lod_frames_device.restype = C.c_int
    L.pxz_lod_frames_device.argtypes = [vp, C.POINTER(Frames), C.POINTER(Params)] + [vp] * 3
    L.pxz_oklab_pixels_device.restype = C.c_int
    L.pxz_oklab_pixels_device.argtypes = [vp, vp, u32, vp]
    L.pxz_pack_tiles_device.restype = C.c_int
    L.pxz_pack_tiles_device.argtypes = [vp, u32, u32, u32, vp, vp, vp, vp, vp, C.c_uint64]
    L.pxz_encode_frames_device.restype = C.c_int
    L.pxz_encode_frames_device.argtypes = [vp, C.POINTER(Frames), C.POINTER(Params), u32, vp, vp, vp, vp, vp, C.c_uint64, vp]
    L.pxz_encode_container.restype = C.c_int64
    L.pxz_encode_container.argtypes = [u32] * 6 + [vp] * 5 + [vp, C.c_size_t]
    L.pxz_qoi_encode.restype = C.c_int64
    L.pxz_qoi_encode.argtypes = [vp, u32, u32, u32, vp, C.c_size_t]
    L.pxz_qoi_bound.restype = C.c_size_t
    L.pxz_qoi_bound.argtypes = [u32] * 3
    L.pxz_expand_frames_device.restype = C.c_int
    L.pxz_expand_frames_device.argtypes = [vp, C.POINTER(Frames), C.POINTER(Params)] + [vp] * 4
    L.pxz_decode_file.restype = C.c_int
    L.pxz_decode_file.argtypes = [vp, vp, C.c_size_t] + [C.POINTER(u32)] * 6 + [vp] * 4
    L.pxz_process_frames_device.restype = C.c_int
    L.pxz_process_frames_device.argtypes = [vp, C.POINTER(Frames), C.POINTER(Params), u32, vp, vp, u32, C.c_uint64]
    L.pxz_tree_process_frames_device.restype = C.c_int
    L.pxz_tree_process_frames_device.argtypes = [vp, C.POINTER(Frames), C.POINTER(Params), u32, f32, u32, u32, vp, vp, u32, C.c_uint64]
    L.pxz_decode_status.restype = C.c_int
    L.pxz_decode_status.argtypes = [vp, C.POINTER(u32)]
    L.pxz_decode_frames_device.restype = C.c_int
    L.pxz_decode_frames_device.argtypes = [vp, C.POINTER(Frames), C.POINTER(Params)] + [vp] * 6
    L.pxz_expand_image.restype = C.c_int
    L.pxz_expand_image.argtypes = [vp] + [u32] * 7 + [vp] * 4
    L.pxz_synth_frames_device.restype = C.c_int
    L.pxz_synth_frames_device.argtypes = [vp, C.POINTER(Frames), vp, u32, u32]
    L.pxz_axis_table.restype = C.c_int
    L.pxz_axis_table.argtypes = [u32] * 3 + [vp] * 3 + [C.POINTER(C.c_int32)] * 2
    if hasattr(L, "pxz_scaled_size"):  # (a build of an earlier commit named by PXZ_LIB lacks the scaled decode)
        L.pxz_scaled_size.restype = C.c_int
        L.pxz_scaled_size.argtypes = [u32] * 5 + [C.POINTER(u32)] * 2
        L.pxz_scaled_axis_table.restype = C.c_int
        L.pxz_scaled_axis_table.argtypes = [u32] * 4 + [vp] * 3 + [C.POINTER(C.c_int32)] * 2
        L.pxz_expand_scaled_lds_bytes.restype = C.c_int
        L.pxz_expand_scaled_lds_bytes.argtypes = [u32] * 5 + [C.POINTER(u32)]
        L.pxz_expand_varied_scaled_frames_device.restype = C.c_int
        L.pxz_expand_varied_scaled_frames_device.argtypes = [vp, vp, u32, u32, C.POINTER(Params)] + [vp] * 6
        L.pxz_expand_windows_scaled_device.restype = C.c_int
        L.pxz_expand_windows_scaled_device.argtypes = [vp, vp, u32, vp, u32, u32, C.POINTER(Params)] + [vp] * 6
        L.pxz_decode_varied_files_scaled.restype = C.c_int
        L.pxz_decode_varied_files_scaled.argtypes = [vp, vp, vp, vp, u32, u32, C.POINTER(Params), vp, vp, vp]
        L.pxz_decode_windows_files_scaled.restype = C.c_int
        L.pxz_decode_windows_files_scaled.argtypes = [vp, vp, vp, vp, u32, vp, u32, u32, C.POINTER(Params), vp, vp, C.c_uint64, vp]
    L.pxz_enable_timing.restype = C.c_int
    L.pxz_enable_timing.argtypes = [vp, C.c_int]
    L.pxz_last_first_kernel_ms.restype = C.c_int
    L.pxz_last_first_kernel_ms.argtypes = [vp, C.POINTER(f32)]
    L.pxz_last_kernel_ms.restype = C.c_int
    L.pxz_last_kernel_ms.argtypes = [vp, C.POINTER(f32)]
    if hasattr(L, "pxz_handle_state"):  # (an older diagnostic build named by PXZ_LIB may lack it)
        L.pxz_handle_state.restype = C.c_int
        L.pxz_handle_state.argtypes = [vp, C.POINTER(C.c_uint32)]
    _lib = L
    return L


def _p(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def grid(width, height, bw, bh):
    c, r = C.c_uint32(), C.c_uint32()
    rc = load_library().pxz_grid(width, height, bw, bh, C.byref(c), C.byref(r))
    if rc != 0:
        raise PxzError(rc)
    return c.value, r.value


def varied_layout(geoms, bw, bh):
    """pxz_varied_layout: geoms = [(width, height, pitch_bytes, offset_bytes), ...] -> uint64[n+1] tile offsets."""
    n = len(geoms)
    out = np.zeros(n + 1, np.uint64)
    rc = load_library().pxz_varied_layout(C.cast(image_descs(geoms), C.c_void_p) if n else None, n, bw, bh, _p(out))
    if rc != 0:
        raise PxzError(rc)
    return out


def window_layout(sizes, windows, bw, bh):
    """pxz_window_layout: sizes = [(width, height), ...] of the images, windows = [(image, x, y, width, height, pitch_bytes,
    offset_bytes), ...] -> uint64[n_windows+1] offsets of the windows' covered tiles.  No GPU."""
    n, k = len(sizes), len(windows)
    geoms = [(w, h, 0, 0) for (w, h) in sizes]
    out = np.zeros(k + 1, np.uint64)
    rc = load_library().pxz_window_layout(C.cast(image_descs(geoms), C.c_void_p) if n else None, n,
                                          C.cast(window_descs(windows), C.c_void_p) if k else None, k, bw, bh, _p(out))
    if rc != 0:
        raise PxzError(rc)
    return out


def patch_check(sizes, windows, bw, bh):
    """pxz_patch_check: window_layout, and the patch's rule that the covered tiles of the windows of one image are disjoint.
    -> uint64[n_windows+1] offsets; raises PxzError whose .window is the first offending window (NO_WINDOW: another reason).
    No GPU."""
    n, k = len(sizes), len(windows)
    geoms = [(w, h, 0, 0) for (w, h) in sizes]
    out = np.zeros(k + 1, np.uint64)
    bad = C.c_uint32(0)
    rc = load_library().pxz_patch_check(C.cast(image_descs(geoms), C.c_void_p) if n else None, n,
                                        C.cast(window_descs(windows), C.c_void_p) if k else None, k, bw, bh, _p(out), C.byref(bad))
    if rc != 0:
        err = PxzError(rc)
        err.window = bad.value
        raise err
    return out


def scaled_size(width, height, bw, bh, scale_log2):
    """pxz_scaled_size: the size (width, height) of an image decoded at 1/2^scale_log2; the scale must divide the block."""
    w, h = C.c_uint32(), C.c_uint32()
    rc = load_library().pxz_scaled_size(width, height, bw, bh, scale_log2, C.byref(w), C.byref(h))
    if rc != 0:
        raise PxzError(rc)
    return w.value, h.value


def scaled_window_size(window, scale_log2):
    """the output size (width, height) of the full-resolution window (image, x, y, width, height, ...) at 1/2^scale_log2"""
    _, x, y, w, h = window[:5]
    s = 1 << scale_log2
    return -(-(x + w) // s) - x // s, -(-(y + h) // s) - y // s


def scaled_axis_table(in_size, out_size, filt, other_axis_grows=False):
    """pxz_scaled_axis_table: (starts, sizes, coeffs[out, window], precision) of the table the scaled kernels use for an axis
    of in_size stored samples resized to out_size; other_axis_grows sets PixlzrBlock::resize's flag for this axis too."""
    L = load_library()
    window, prec = C.c_int32(), C.c_int32()
    rc = L.pxz_scaled_axis_table(in_size, out_size, filt, int(other_axis_grows), None, None, None, C.byref(window), C.byref(prec))
    if rc != 0:
        raise PxzError(rc)
    starts = np.zeros(out_size, np.int32)
    sizes = np.zeros(out_size, np.int32)
    k = np.zeros((out_size, window.value), np.int16)
    L.pxz_scaled_axis_table(in_size, out_size, filt, int(other_axis_grows), _p(starts), _p(sizes), _p(k), C.byref(window), C.byref(prec))
    return starts, sizes, k, prec.value


def expand_scaled_lds_bytes(bw, bh, channels, filt, max_scale_log2):
    """pxz_expand_scaled_lds_bytes: LDS bytes of one wave's image of the scaled kernels (host only).  Raises PxzError (with
    .lds_bytes) when it does not fit."""
    out = C.c_uint32(0)
    rc = load_library().pxz_expand_scaled_lds_bytes(bw, bh, channels, filt, max_scale_log2, C.byref(out))
    if rc != 0:
        err = PxzError(rc)
        err.lds_bytes = out.value
        raise err
    return out.value


def _u32s(values):
    return (C.c_uint32 * max(len(values), 1))(*[int(v) for v in values])


def _lds_query(entry, *args, out=None):
    """one of the pxz_*_lds_bytes size queries (host only): what it answers.  out: a ctypes c_uint32 to write into."""
    out = C.c_uint32(0) if out is None else out
    rc = getattr(load_library(), entry)(*args, C.byref(out))
    if rc != 0:
        raise PxzError(rc)
    return out.value


def reshrink_lds_bytes(bw, bh, mode, expand_filter):
    """pxz_reshrink_lds_bytes: LDS bytes of one block of the re-shrink kernel (host only; above 163840: unsupported)."""
    return _lds_query("pxz_reshrink_lds_bytes", bw, bh, mode, expand_filter)


def retile_lds_bytes(src_bw, src_bh, bw, bh, mode, expand_filter):
    """pxz_retile_lds_bytes: LDS bytes of one block of the re-tile kernel for source blocks of src_bw x src_bh and destination
    blocks of bw x bh (host only; above 163840: unsupported)."""
    return _lds_query("pxz_retile_lds_bytes", src_bw, src_bh, bw, bh, mode, expand_filter)


def retile_ladder_lds_bytes(src_bw, src_bh, bw, bh, channels, mode, expand_filter):
    """pxz_retile_ladder_lds_bytes: LDS bytes of one block of the re-tile ladder kernel for source blocks of src_bw x src_bh and
    destination blocks of bw x bh (host only; above 163840: unsupported)."""
    return _lds_query("pxz_retile_ladder_lds_bytes", src_bw, src_bh, bw, bh, channels, mode, expand_filter)


def reshrink_ladder_lds_bytes(bw, bh, channels, mode, expand_filter):
    """pxz_reshrink_ladder_lds_bytes: LDS bytes of one block of the re-shrink ladder kernel (host only; above 163840:
    unsupported)."""
    return _lds_query("pxz_reshrink_ladder_lds_bytes", bw, bh, channels, mode, expand_filter)


def retile_distortion_lds_bytes(src_bw, src_bh, bw, bh, channels, expand_filter, filter_up, out=None):
    """pxz_retile_distortion_lds_bytes: LDS bytes of one block of retile_distortion_varied_device for source blocks of
    src_bw x src_bh and destination blocks of bw x bh (host only; above 163840: unsupported).  out: a ctypes c_uint32 to write
    into (for the error cases)."""
    return _lds_query("pxz_retile_distortion_lds_bytes", src_bw, src_bh, bw, bh, channels, expand_filter, filter_up, out=out)


def reshrink_distortion_lds_bytes(bw, bh, channels, expand_filter, filter_up, out=None):
    """pxz_reshrink_distortion_lds_bytes: LDS bytes of a one-wave block of reshrink_distortion_varied_device (host only; above
    163840: unsupported).  out: a ctypes c_uint32 to write into (for the error cases)."""
    return _lds_query("pxz_reshrink_distortion_lds_bytes", bw, bh, channels, expand_filter, filter_up, out=out)


def file_header(data):
    """pxz_file_header: one .pixlzr file (bytes) -> (width, height, block_w, block_h, channels, filter_byte).  No GPU."""
    buf = np.frombuffer(bytes(data), np.uint8)
    v = [C.c_uint32() for _ in range(6)]
    rc = load_library().pxz_file_header(_p(buf) if buf.size else None, buf.size, *[C.byref(x) for x in v])
    if rc != 0:
        raise PxzError(rc)
    return tuple(x.value for x in v)


def qoi_encode(tile):
    tile = np.ascontiguousarray(tile, np.uint8)
    h, w, c = tile.shape
    L = load_library()
    out = np.empty(L.pxz_qoi_bound(w, h, c), np.uint8)
    n = L.pxz_qoi_encode(_p(tile), w, h, c, _p(out), out.size)
    if n < 0:
        raise PxzError(int(n))
    return out[:n].tobytes()


def encode_container(width, height, bw, bh, channels, filter_byte, values, has_value, tw, th, slots):
    """Pixlzr::encode_to_vec: tiles (slots + dims + values) -> .pixlzr bytes."""
    L = load_library()
    values = np.ascontiguousarray(values, np.float32)
    tw = np.ascontiguousarray(tw, np.uint32)
    th = np.ascontiguousarray(th, np.uint32)
    slots = np.ascontiguousarray(slots, np.uint8)
    hv = None if has_value is None else np.ascontiguousarray(has_value, np.uint8)
    head = [width, height, bw, bh, channels, filter_byte, _p(values), _p(hv), _p(tw), _p(th), _p(slots)]
    bound = L.pxz_encode_container(*head, None, 0)
    if bound < 0:
        raise PxzError(int(bound))
    out = np.empty(bound, np.uint8)
    n = L.pxz_encode_container(*head, _p(out), out.size)
    if n < 0:
        raise PxzError(int(n))
    return out[:n].tobytes()


def psnr(sse, n_samples):
    """10 log10(255^2 n / sse) in dB for a squared error summed over n_samples 8-bit samples (pixels x channels): what a
    caller makes of the sums the distortion calls return.  inf for an sse of 0; numpy arrays go through element by element."""
    sse = np.asarray(sse, np.float64)
    with np.errstate(divide="ignore"):
        out = 10.0 * np.log10(255.0 * 255.0 * np.asarray(n_samples, np.float64) / sse)
    return float(out) if out.ndim == 0 else out


def sse_for_psnr(db, n_samples):
    """The inverse of psnr, rounded down: the largest summed squared error (a Python int, at most 2^64-1) over n_samples
    8-bit samples that still has a PSNR of at least db -- the target of FIT_SSE for "at least db dB":
    psnr(sse_for_psnr(q, n), n) >= q > psnr(sse_for_psnr(q, n) + 1, n)."""
    top = 2 ** 64 - 1
    est = 255.0 * 255.0 * float(n_samples) / 10.0 ** (float(db) / 10.0)
    s = top if est >= float(top) else max(int(est), 0)
    for _ in range(8):  # (the estimate is an ulp or two off at the most; psnr itself has the last word)
        if s > 0 and psnr(s, n_samples) < db:
            s -= 1
        elif s < top and psnr(s + 1, n_samples) >= db:
            s += 1
        else:
            break
    return s


def fit_select(file_bytes, sse, criterion, targets, n_images=None, n_factors=None, channels=None, out=None):
    """pxz_fit_select: the rung of every image under its target, on the host.  file_bytes uint64[K, n] and sse uint64[K, n, C]
    as rate_distortion_varied_images returns them, targets n integers (a budget in bytes under FIT_BYTES, a summed squared
    error under FIT_SSE) -> (choice uint32[n], fit_flags uint32[n]; bit 0: no rung met the target).  No GPU.  n_images,
    n_factors and channels override what the shapes say, None among the arrays passes a null pointer, and out = (choice,
    fit_flags) is written in place (all for the error cases)."""
    fb = None if file_bytes is None else np.ascontiguousarray(file_bytes, np.uint64)
    ss = None if sse is None else np.ascontiguousarray(sse, np.uint64)
    tg = None if targets is None else np.array([int(t) for t in targets], np.uint64)
    K = n_factors if n_factors is not None else fb.shape[0]
    n = n_images if n_images is not None else fb.shape[1]
    ch = channels if channels is not None else ss.shape[2]
    choice, flags = out if out is not None else (np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.uint32))
    rc = load_library().pxz_fit_select(n, K, ch, criterion, _p(tg), _p(fb), _p(ss), _p(choice), _p(flags))
    if rc != 0:
        raise PxzError(rc)
    return choice[:n], flags[:n]


def fit_tiles_select(group_tile_offsets, group_fixed_bytes, tile_bytes, tile_sse, criterion, targets, n_groups=None, n_factors=None,
                     channels=None, out=None):
    """pxz_fit_tiles_select: the rung of every tile under its group's target, on the host.  group_tile_offsets (G + 1 integers
    from 0 on), group_fixed_bytes and targets (G integers), tile_bytes uint32[K, T] and tile_sse uint64[K, T, C] -> (tile_choice
    uint32[T], lambda uint64[G], bytes uint64[G], sse uint64[G], flags uint32[G]; TILEFIT_MISSED | TILEFIT_NO_CANDIDATE |
    TILEFIT_UNIFORM).  No GPU.  n_groups, n_factors and channels override what the shapes say, None among the arrays passes a
    null pointer, and out = such a 5-tuple is written in place (all for the error cases)."""
    u64 = lambda a: None if a is None else np.array([int(x) for x in a], np.uint64)  # noqa: E731
    off, fixed, tg = u64(group_tile_offsets), u64(group_fixed_bytes), u64(targets)
    tb = None if tile_bytes is None else np.ascontiguousarray(tile_bytes, np.uint32)
    ts = None if tile_sse is None else np.ascontiguousarray(tile_sse, np.uint64)
    G = n_groups if n_groups is not None else len(off) - 1
    K = n_factors if n_factors is not None else tb.shape[0]
    ch = channels if channels is not None else ts.shape[2]
    T = int(off[-1]) if off is not None and len(off) else 0
    if out is None:
        out = (np.zeros(max(T, 1), np.uint32), np.zeros(max(G, 1), np.uint64), np.zeros(max(G, 1), np.uint64), np.zeros(max(G, 1), np.uint64),
               np.zeros(max(G, 1), np.uint32))
    choice, lam, gb, gs, fl = out
    rc = load_library().pxz_fit_tiles_select(G, _p(off), _p(fixed), K, ch, criterion, _p(tg), _p(tb), _p(ts), _p(choice), _p(lam), _p(gb),
                                             _p(gs), _p(fl))
    if rc != 0:
        raise PxzError(rc)
    return choice[:T], lam[:G], gb[:G], gs[:G], fl[:G]


def axis_table(in_size, out_size, filt):
    L = load_library()
    window, prec = C.c_int32(), C.c_int32()
    rc = L.pxz_axis_table(in_size, out_size, filt, None, None, None, C.byref(window), C.byref(prec))
    if rc != 0:
        raise PxzError(rc)
    starts = np.zeros(out_size, np.int32)
    sizes = np.zeros(out_size, np.int32)
    k = np.zeros((out_size, max(window.value, 1)), np.int16)
    L.pxz_axis_table(in_size, out_size, filt, _p(starts), _p(sizes), _p(k), C.byref(window), C.byref(prec))
    return starts, sizes, k, prec.value


class Handle:
    """One GPU.  Device entry points take/return torch CUDA tensors (plumbing only)."""

    def __init__(self, device_id=0):
        self._L = load_library()
        self._h = C.c_void_p()
        rc = self._L.pxz_create(device_id, C.byref(self._h))
        if rc != 0:
            raise PxzError(rc, "pxz_create: no usable gfx950 device (there is no CPU fallback)")
        self.device_id = device_id

    def close(self):
        if self._h:
            self._L.pxz_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise PxzError(rc, (self._L.pxz_last_error(self._h) or b"").decode())

    def set_stream(self, stream_ptr):
        self._check(self._L.pxz_set_stream(self._h, C.c_void_p(stream_ptr)))

    def use_torch_stream(self):
        import torch
        self.set_stream(torch.cuda.current_stream(self.device_id).cuda_stream)

    def trim(self):
        """pxz_trim: the handle's scratch buffers go back to the device (the next call grows them again)"""
        self._check(self._L.pxz_trim(self._h))

    def synchronize(self):
        self._check(self._L.pxz_synchronize(self._h))

    def enable_timing(self, on=True, every=1):
        """every = n > 1: only every n-th step is bracketed by events."""
        self._check(self._L.pxz_enable_timing(self._h, (max(int(every), 1) if on else 0)))

    def last_first_kernel_ms(self):
        ms = C.c_float()
        self._check(self._L.pxz_last_first_kernel_ms(self._h, C.byref(ms)))
        return ms.value

    def state(self):
        """which kernels the fast paths pick (pxz_handle_state): a timing is comparable only with one taken in the same state"""
        st = (C.c_uint32 * 4)()
        if not hasattr(self._L, "pxz_handle_state"):
            return None
        self._check(self._L.pxz_handle_state(self._h, st))
        return {"transparent_tiles_seen_by_last_finished_launch": int(st[0]),
                "tiles_listed_by_last_finished_launch": None if st[1] == 0xffffffff else int(st[1]),
                "alpha_kernel": bool(st[2]), "alpha_first": bool(st[3])}

    def last_kernel_ms(self):
        ms = C.c_float()
        self._check(self._L.pxz_last_kernel_ms(self._h, C.byref(ms)))
        return ms.value

    # ---- host-buffer entry point (Pixlzr::from_image + shrink_*) ----
    def shrink_image(self, img, bw, bh, mode, filt, factor, want_pixels=True):
        H, W, Cc = img.shape
        assert img.dtype == np.uint8 and img.strides[2] == 1 and img.strides[1] == Cc
        cols, rows = grid(W, H, bw, bh)
        n = cols * rows
        vals = np.zeros(n, np.float32)
        ow = np.zeros(n, np.uint32)
        oh = np.zeros(n, np.uint32)
        slots = np.zeros((n, bw * bh * Cc), np.uint8) if want_pixels else None
        self._check(self._L.pxz_shrink_image(self._h, C.c_void_p(img.ctypes.data), W, H, Cc, img.strides[0], bw, bh,
                                             mode, filt, C.c_float(factor), _p(vals), _p(ow), _p(oh), _p(slots)))
        return vals, ow, oh, slots

    def shrink_image_ladder(self, img, bw, bh, mode, filt, factors, want_pixels=True):
        """pxz_shrink_image_ladder: shrink_image at every factor of `factors` in one call.
        Returns (values[K,T], w[K,T], h[K,T], slots[K,T,bw*bh*C] | None); rung r equals shrink_image(..., factors[r])."""
        H, W, Cc = img.shape
        assert img.dtype == np.uint8 and img.strides[2] == 1 and img.strides[1] == Cc
        fac = np.ascontiguousarray(factors, np.float32)
        K = fac.size
        cols, rows = grid(W, H, bw, bh)
        n = cols * rows
        vals = np.zeros((K, n), np.float32)
        ow = np.zeros((K, n), np.uint32)
        oh = np.zeros((K, n), np.uint32)
        slots = np.zeros((K, n, bw * bh * Cc), np.uint8) if want_pixels else None
        self._check(self._L.pxz_shrink_image_ladder(self._h, C.c_void_p(img.ctypes.data), W, H, Cc, img.strides[0], bw, bh,
                                                    mode, filt, _p(fac) if K else None, K, _p(vals), _p(ow), _p(oh), _p(slots)))
        return vals, ow, oh, slots

    def shrink_image_packed(self, img, bw, bh, mode, filt, factor):
        """pxz_shrink_image_packed + pxz_fetch_packed: (values, w, h, stream) with the tiles' pixels back to back."""
        H, W, Cc = img.shape
        assert img.dtype == np.uint8 and img.strides[2] == 1 and img.strides[1] == Cc
        cols, rows = grid(W, H, bw, bh)
        n = cols * rows
        vals = np.zeros(n, np.float32)
        ow = np.zeros(n, np.uint32)
        oh = np.zeros(n, np.uint32)
        total = C.c_uint64(0)
        self._check(self._L.pxz_shrink_image_packed(self._h, C.c_void_p(img.ctypes.data), W, H, Cc, img.strides[0], bw, bh,
                                                    mode, filt, C.c_float(factor), _p(vals), _p(ow), _p(oh), C.byref(total)))
        stream = np.empty(total.value, np.uint8)
        self._check(self._L.pxz_fetch_packed(self._h, _p(stream), total.value))
        return vals, ow, oh, stream

    def shrink_images(self, imgs, bw, bh, mode, filt, factor, want_pixels=True, packed=False):
        """pxz_shrink_images[_packed]: a list of equally sized (H, W, C) uint8 images through the pipelined host boundary.
        Returns a list of (values, w, h, slots | stream | None) per image."""
        n = len(imgs)
        H, W, Cc = imgs[0].shape
        for im in imgs:
            assert im.shape == (H, W, Cc) and im.dtype == np.uint8 and im.strides == imgs[0].strides and im.strides[2] == 1 and im.strides[1] == Cc
        cols, rows = grid(W, H, bw, bh)
        T = cols * rows
        vals = [np.zeros(T, np.float32) for _ in range(n)]
        ow = [np.zeros(T, np.uint32) for _ in range(n)]
        oh = [np.zeros(T, np.uint32) for _ in range(n)]
        ptrs = lambda arrs: (C.c_void_p * n)(*[a.ctypes.data for a in arrs])
        src = ptrs(imgs)
        if packed:
            cap = H * W * Cc
            px = [np.empty(cap, np.uint8) for _ in range(n)]
            lens = np.zeros(n, np.uint64)
            self._check(self._L.pxz_shrink_images_packed(self._h, src, n, W, H, Cc, imgs[0].strides[0], bw, bh, mode, filt, C.c_float(factor),
                                                         ptrs(vals), ptrs(ow), ptrs(oh), ptrs(px), cap, _p(lens)))
            return [(vals[k], ow[k], oh[k], px[k][: int(lens[k])]) for k in range(n)]
        px = [np.zeros((T, bw * bh * Cc), np.uint8) for _ in range(n)] if want_pixels else None
        self._check(self._L.pxz_shrink_images(self._h, src, n, W, H, Cc, imgs[0].strides[0], bw, bh, mode, filt, C.c_float(factor),
                                              ptrs(vals), ptrs(ow), ptrs(oh), ptrs(px) if px else None))
        return [(vals[k], ow[k], oh[k], px[k] if px else None) for k in range(n)]

    def oklab_pixels_device(self, rgba):
        """rgba: uint8 CUDA tensor [n, 4] -> float32 [n, 4] = (l, a, b, alpha) per pixel."""
        import torch
        assert rgba.is_cuda and rgba.dtype == torch.uint8 and rgba.dim() == 2 and rgba.shape[1] == 4 and rgba.is_contiguous()
        out = torch.empty((rgba.shape[0], 4), dtype=torch.float32, device=rgba.device)
        self.use_torch_stream()
        self._check(self._L.pxz_oklab_pixels_device(self._h, C.c_void_p(rgba.data_ptr()), rgba.shape[0], C.c_void_p(out.data_ptr())))
        return out

    # ---- device entry points ----
    @staticmethod
    def _frames_desc(frames):
        assert frames.is_cuda and frames.dim() == 4 and frames.dtype.is_floating_point is False
        N, H, W, Cc = frames.shape
        assert frames.stride(3) == 1 and frames.stride(2) == Cc
        return Frames(W, H, Cc, frames.stride(1), N, 0, frames.stride(0)), (N, H, W, Cc)

    def shrink_frames_device(self, frames, bw, bh, mode, filt, factor, want_pixels=True, out=None, transparency_hint=False):
        """frames: uint8 CUDA tensor [N,H,W,C].  Returns (values[N,T], w[N,T], h[N,T], slots[N,T,bw*bh*C]|None).
        transparency_hint: PXZ_HINT_TRANSPARENCY (many tiles with alpha < 255; a pure performance hint)."""
        import torch
        fd, (N, H, W, Cc) = self._frames_desc(frames)
        cols, rows = grid(W, H, bw, bh)
        T = cols * rows
        dev = frames.device
        if out is None:
            vals = torch.empty((N, T), dtype=torch.float32, device=dev)
            ow = torch.empty((N, T), dtype=torch.int32, device=dev)
            oh = torch.empty((N, T), dtype=torch.int32, device=dev)
            slots = torch.empty((N, T, bw * bh * Cc), dtype=torch.uint8, device=dev) if want_pixels else None
        else:
            vals, ow, oh, slots = out
        pd = Params(bw, bh, mode, filt, factor, 1 if transparency_hint else 0)
        self.use_torch_stream()
        self._check(self._L.pxz_shrink_frames_device(
            self._h, C.byref(fd), C.byref(pd), C.c_void_p(frames.data_ptr()), C.c_void_p(vals.data_ptr()),
            C.c_void_p(ow.data_ptr()), C.c_void_p(oh.data_ptr()),
            C.c_void_p(slots.data_ptr()) if slots is not None else None))
        return vals, ow, oh, slots

    def shrink_ladder_frames_device(self, frames, bw, bh, mode, filt, factors, want_pixels=True, out=None, transparency_hint=False):
        """pxz_shrink_ladder_frames_device: shrink_frames_device at every factor of `factors` (a host sequence, 1..16 of them)
        in one call.  Returns (values[K,N,T], w[K,N,T], h[K,N,T], slots[K,N,T,bw*bh*C] | None); rung r equals
        shrink_frames_device(..., factors[r]).  out: a 4-tuple of such tensors (slots may be None)."""
        import torch
        fd, (N, H, W, Cc) = self._frames_desc(frames)
        fac = np.ascontiguousarray(factors, np.float32)
        K = fac.size
        cols, rows = grid(W, H, bw, bh)
        T = cols * rows
        dev = frames.device
        if out is None:
            vals = torch.empty((K, N, T), dtype=torch.float32, device=dev)
            ow = torch.empty((K, N, T), dtype=torch.int32, device=dev)
            oh = torch.empty((K, N, T), dtype=torch.int32, device=dev)
            slots = torch.empty((K, N, T, bw * bh * Cc), dtype=torch.uint8, device=dev) if want_pixels else None
        else:
            vals, ow, oh, slots = out
        pd = Params(bw, bh, mode, filt, 0.0, 1 if transparency_hint else 0)
        self.use_torch_stream()
        self._check(self._L.pxz_shrink_ladder_frames_device(
            self._h, C.byref(fd), C.byref(pd), _p(fac) if K else None, K, C.c_void_p(frames.data_ptr()),
            C.c_void_p(vals.data_ptr()), C.c_void_p(ow.data_ptr()), C.c_void_p(oh.data_ptr()),
            C.c_void_p(slots.data_ptr()) if slots is not None else None))
        return vals, ow, oh, slots

    # ---- batches of differently sized images ----
    @staticmethod
    def _varied_batch(images, descs):
        """images: a list of uint8 CUDA tensors [H, W, C] (rows may be padded: stride(0) is the pitch), or one uint8 CUDA
        buffer with descs = [(width, height, pitch_bytes, offset_bytes), ...].  -> (base pointer, geoms, channels, keep-alive)"""
        import torch
        if descs is not None:
            buf = images
            assert buf.is_cuda and buf.dtype == torch.uint8
            ch = None
            return buf.data_ptr(), [tuple(d) for d in descs], ch, buf
        assert len(images) > 0
        base = min(t.data_ptr() for t in images)
        geoms = []
        for t in images:
            assert t.is_cuda and t.dtype == torch.uint8 and t.dim() == 3 and t.stride(2) == 1 and t.stride(1) == t.shape[2]
            geoms.append((t.shape[1], t.shape[0], t.stride(0), t.data_ptr() - base))
        return base, geoms, images[0].shape[2], images

    def shrink_varied_frames_device(self, images, bw, bh, mode, filt, factor, want_pixels=True, descs=None, channels=None, out=None):
        """pxz_shrink_varied_frames_device: every image of a list of differently sized CUDA images in one call.
        Returns (tile_offsets uint64[n+1], values[T], w[T], h[T], slots[T, bw*bh*C] | None); image i's tiles are
        [tile_offsets[i], tile_offsets[i+1]).  With descs, `images` is one uint8 CUDA buffer and channels must be given."""
        import torch
        base, geoms, ch, keep = self._varied_batch(images, descs)
        ch = channels if channels is not None else ch
        dev = torch.device("cuda", self.device_id)
        offs = None
        if out is None:
            offs = varied_layout(geoms, bw, bh)
            T = int(offs[-1])
            vals = torch.empty(T, dtype=torch.float32, device=dev)
            ow = torch.empty(T, dtype=torch.int32, device=dev)
            oh = torch.empty(T, dtype=torch.int32, device=dev)
            slots = torch.empty((T, bw * bh * ch), dtype=torch.uint8, device=dev) if want_pixels else None
        else:
            vals, ow, oh, slots = out
        pd = Params(bw, bh, mode, filt, factor, 0)
        self.use_torch_stream()
        self._check(self._L.pxz_shrink_varied_frames_device(
            self._h, C.cast(image_descs(geoms), C.c_void_p), len(geoms), ch, C.byref(pd), C.c_void_p(base),
            C.c_void_p(vals.data_ptr()), C.c_void_p(ow.data_ptr()), C.c_void_p(oh.data_ptr()),
            C.c_void_p(slots.data_ptr()) if slots is not None else None))
        del keep
        if offs is None:  # (given outputs: the library checks the descriptors first and names a failing image)
            offs = varied_layout(geoms, bw, bh)
        return offs, vals, ow, oh, slots

    def shrink_varied_ladder_frames_device(self, images, bw, bh, mode, filt, factors, want_pixels=True, descs=None, channels=None,
                                           out=None, n_factors=None):
        """pxz_shrink_varied_ladder_frames_device: shrink_varied_frames_device at every factor of `factors` (a host sequence,
        1..32 of them) in one launch.  Returns (tile_offsets uint64[n+1], values[K,T], w[K,T], h[K,T], slots[K,T,bw*bh*C] |
        None); rung r equals shrink_varied_frames_device(..., factors[r]), and the arrays flattened are the varied layout of
        the images repeated K times.  out: a 4-tuple of such tensors (slots may be None).  factors None with n_factors passes
        a null pointer."""
        import torch
        base, geoms, ch, keep = self._varied_batch(images, descs)
        ch = channels if channels is not None else ch
        fac = None if factors is None else np.ascontiguousarray(factors, np.float32)
        K = n_factors if n_factors is not None else (0 if fac is None else fac.size)
        dev = torch.device("cuda", self.device_id)
        offs = None
        if out is None:
            offs = varied_layout(geoms, bw, bh)
            T = int(offs[-1])
            vals = torch.empty((K, T), dtype=torch.float32, device=dev)
            ow = torch.empty((K, T), dtype=torch.int32, device=dev)
            oh = torch.empty((K, T), dtype=torch.int32, device=dev)
            slots = torch.empty((K, T, bw * bh * ch), dtype=torch.uint8, device=dev) if want_pixels else None
        else:
            vals, ow, oh, slots = out
        pd = Params(bw, bh, mode, filt, 0.0, 0)
        self.use_torch_stream()
        self._check(self._L.pxz_shrink_varied_ladder_frames_device(
            self._h, C.cast(image_descs(geoms), C.c_void_p), len(geoms), ch, C.byref(pd),
            _p(fac) if fac is not None and fac.size else None, K, C.c_void_p(base),
            C.c_void_p(vals.data_ptr()), C.c_void_p(ow.data_ptr()), C.c_void_p(oh.data_ptr()),
            C.c_void_p(slots.data_ptr()) if slots is not None else None))
        del keep
        if offs is None:
            offs = varied_layout(geoms, bw, bh)
        return offs, vals, ow, oh, slots

    def encode_varied_frames_device(self, sizes, channels, bw, bh, vals, ow, oh, slots, filter_byte=0, out=None):
        """pxz_encode_varied_frames_device: sizes = [(width, height), ...] of the images whose tiles (varied layout) are given.
        Returns (file_offsets int64[n+1], bytes uint8[capacity])."""
        import torch
        geoms = [(w, h, w * channels, 0) for (w, h) in sizes]
        n = len(geoms)
        if out is None:
            cap = 0
            for (w, h) in sizes:
                cols, rows = grid(w, h, bw, bh)
                cap += 26 + rows * 4 + cols * rows * (13 + 10 + bw * bh * (channels + 1) + 8)
            offs = torch.empty(n + 1, dtype=torch.int64, device=vals.device)
            buf = torch.empty(cap, dtype=torch.uint8, device=vals.device)
        else:
            offs, buf = out
        pd = Params(bw, bh, 0, 0, 1.0, 0)
        self.use_torch_stream()
        self._check(self._L.pxz_encode_varied_frames_device(
            self._h, C.cast(image_descs(geoms), C.c_void_p), n, channels, C.byref(pd), filter_byte,
            C.c_void_p(vals.data_ptr()), C.c_void_p(ow.data_ptr()), C.c_void_p(oh.data_ptr()), C.c_void_p(slots.data_ptr()),
            C.c_void_p(buf.data_ptr()), buf.numel(), C.c_void_p(offs.data_ptr())))
        return offs, buf

    def encode_varied_images(self, imgs, bw, bh, mode, filt, factor, filter_byte=0):
        """pxz_encode_varied_images: host images (numpy uint8 [H, W, C], one channel count) -> a list of .pixlzr files (bytes)."""
        imgs = [np.ascontiguousarray(i) if i.strides[1] != i.shape[2] or i.strides[2] != 1 else i for i in imgs]
        n = len(imgs)
        ch = imgs[0].shape[2] if n else 4
        geoms = [(i.shape[1], i.shape[0], i.strides[0], 0) for i in imgs]
        ptrs = (C.c_void_p * max(n, 1))(*[i.ctypes.data for i in imgs])
        descs = image_descs(geoms)
        pd = Params(bw, bh, mode, filt, factor, 0)
        offs = np.zeros(n + 1, np.uint64)
        buf = np.empty(sum(i.size for i in imgs) * 5 // 4 + 4096 * max(n, 1), np.uint8)
        for attempt in range(2):  # (a second call only when the first guess at the files' size was short)
            rc = self._L.pxz_encode_varied_images(self._h, C.cast(ptrs, C.c_void_p), C.cast(descs, C.c_void_p), n, ch,
                                                  C.byref(pd), filter_byte, _p(buf), buf.size, _p(offs))
            if rc != -7 or attempt == 1:
                break
            buf = np.empty(int(offs[-1]), np.uint8)
        self._check(rc)
        return [buf[int(offs[i]):int(offs[i + 1])].tobytes() for i in range(n)]

    def decode_varied_frames_device(self, files, file_offsets, sizes, channels, bw, bh, out=None, image_flags=None):
        """pxz_decode_varied_frames_device: files = uint8 CUDA tensor holding the .pixlzr files of differently sized images
        back to back, file_offsets int64[n+1] (CUDA), sizes = [(width, height), ...].  Returns (tile_offsets uint64[n+1],
        values[T], w[T], h[T], slots[T, bw*bh*C]) in the varied layout; image_flags (int32[n] CUDA, optional) gets 0 | 2."""
        import torch
        geoms = [(w, h, w * channels, 0) for (w, h) in sizes]
        offs = None
        if out is None:
            offs = varied_layout(geoms, bw, bh)
            T = int(offs[-1])
            dev = files.device
            vals = torch.zeros(T, dtype=torch.float32, device=dev)
            ow = torch.zeros(T, dtype=torch.int32, device=dev)
            oh = torch.zeros(T, dtype=torch.int32, device=dev)
            slots = torch.zeros((T, bw * bh * channels), dtype=torch.uint8, device=dev)
        else:
            vals, ow, oh, slots = out
        pd = Params(bw, bh, 0, 0, 0.0, 0)
        self.use_torch_stream()
        self._check(self._L.pxz_decode_varied_frames_device(
            self._h, C.cast(image_descs(geoms), C.c_void_p), len(geoms), channels, C.byref(pd), C.c_void_p(files.data_ptr()),
            C.c_void_p(file_offsets.data_ptr()), C.c_void_p(vals.data_ptr()), C.c_void_p(ow.data_ptr()), C.c_void_p(oh.data_ptr()),
            C.c_void_p(slots.data_ptr()), C.c_void_p(image_flags.data_ptr()) if image_flags is not None else None))
        if offs is None:
            offs = varied_layout(geoms, bw, bh)
        return offs, vals, ow, oh, slots

    def expand_varied_frames_device(self, descs, channels, bw, bh, filt, ow, oh, slots, out, image_flags=None):
        """pxz_expand_varied_frames_device: the stored tiles of a varied batch (w[T], h[T], slots[T, bw*bh*C]) -> the images,
        written into the uint8 CUDA buffer `out` at descs = [(width, height, pitch_bytes, offset_bytes), ...].  Returns out."""
        geoms = [tuple(d) for d in descs]
        pd = Params(bw, bh, 0, filt, 0.0, 0)
        self.use_torch_stream()
        self._check(self._L.pxz_expand_varied_frames_device(
            self._h, C.cast(image_descs(geoms), C.c_void_p), len(geoms), channels, C.byref(pd), C.c_void_p(ow.data_ptr()),
            C.c_void_p(oh.data_ptr()), C.c_void_p(slots.data_ptr()), C.c_void_p(out.data_ptr()),
            C.c_void_p(image_flags.data_ptr()) if image_flags is not None else None))
        return out

    def decode_varied_files(self, files, channels, bw, bh, filt, sizes=None, out=None, descs=None):
        """pxz_decode_varied_files: a list of .pixlzr files (bytes) of one channel count and block size -> a list of
        (height, width, channels) images.  sizes defaults to what the headers say (file_header); with out (a numpy uint8
        buffer) and descs = [(width, height, pitch_bytes, offset_bytes), ...] the images are written there instead.
        Returns (images | out, flags uint32[n]); raises PxzError (with .flags) when a file is refused or malformed."""
        n = len(files)
        bufs = [np.frombuffer(bytes(f), np.uint8) for f in files]
        if sizes is None and descs is None:
            sizes = [file_header(f)[:2] for f in files]
        own = descs is None
        if own:
            descs, at = [], 0
            for (w, h) in sizes:
                descs.append((w, h, w * channels, at))
                at += w * h * channels
            out = np.zeros(max(at, 1), np.uint8)
        ptrs = (C.c_void_p * max(n, 1))(*[b.ctypes.data if b.size else None for b in bufs])
        lens = (C.c_size_t * max(n, 1))(*[b.size for b in bufs])
        flags = np.zeros(max(n, 1), np.uint32)
        pd = Params(bw, bh, 0, filt, 0.0, 0)
        rc = self._L.pxz_decode_varied_files(self._h, C.cast(ptrs, C.c_void_p), C.cast(lens, C.c_void_p),
                                             C.cast(image_descs(descs), C.c_void_p), n, channels, C.byref(pd), _p(out), _p(flags))
        if own:
            result = [out[d[3]:d[3] + d[0] * d[1] * channels].reshape(d[1], d[0], channels) for d in descs]
        else:
            result = out
        if rc != 0:
            err = PxzError(rc, (self._L.pxz_last_error(self._h) or b"").decode())
            err.flags, err.images = flags[:n], result
            raise err
        return result, flags[:n]

    # ---- the archive calls: stored tiles to stored tiles ----
    def _tiles_to_tiles(self, entry, sizes, channels, src_block, bw, bh, mode, filt, factor, expand_filter, ow, oh, slots, want_pixels, out,
                        image_flags, ladder=None):
        """The re-shrink, the re-tile and their ladders: the library's `entry` with src_block = (src_bw, src_bh) where the block
        changes (else ()) and ladder = (factors, n_factors) where it has rungs (outputs [K, T] then, else [T]).  Allocates the
        outputs that `out` does not bring, marshals, returns what the four wrappers return."""
        import torch
        geoms = [(w, h, w * channels, 0) for (w, h) in sizes]
        rungs = ()
        if ladder is not None:
            fac = None if ladder[0] is None else np.ascontiguousarray(ladder[0], np.float32)
            K = ladder[1] if ladder[1] is not None else (0 if fac is None else fac.size)
            rungs = (_p(fac) if fac is not None and fac.size else None, K)
        offs = None
        if out is None:
            offs = varied_layout(geoms, bw, bh)
            shape = rungs[1:] + (int(offs[-1]),)
            dev = ow.device
            vals = torch.empty(shape, dtype=torch.float32, device=dev)
            nw = torch.empty(shape, dtype=torch.int32, device=dev)
            nh = torch.empty(shape, dtype=torch.int32, device=dev)
            nslots = torch.empty(shape + (bw * bh * channels,), dtype=torch.uint8, device=dev) if want_pixels else None
        else:
            vals, nw, nh, nslots = out
        pd = Params(bw, bh, mode, filt, factor, 0)
        self.use_torch_stream()
        self._check(getattr(self._L, entry)(
            self._h, C.cast(image_descs(geoms), C.c_void_p), len(geoms), channels, *src_block, C.byref(pd), expand_filter, *rungs,
            C.c_void_p(ow.data_ptr()), C.c_void_p(oh.data_ptr()), C.c_void_p(slots.data_ptr()), C.c_void_p(vals.data_ptr()),
            C.c_void_p(nw.data_ptr()), C.c_void_p(nh.data_ptr()), C.c_void_p(nslots.data_ptr()) if nslots is not None else None,
            C.c_void_p(image_flags.data_ptr()) if image_flags is not None else None))
        if offs is None:
            offs = varied_layout(geoms, bw, bh)
        return offs, vals, nw, nh, nslots

    # ---- re-shrink: stored tiles to stored tiles ----
    def reshrink_varied_frames_device(self, sizes, channels, bw, bh, mode, filt, factor, expand_filter, ow, oh, slots,
                                      want_pixels=True, out=None, image_flags=None):
        """pxz_reshrink_varied_frames_device: the stored tiles (w[T], h[T], slots[T, bw*bh*C], varied layout) of the images
        sizes = [(width, height), ...] expanded with expand_filter and shrunk again with (mode, filt, factor), without the
        images.  Returns (tile_offsets uint64[n+1], values[T], w[T], h[T], slots | None).  out: a 4-tuple of such tensors
        (slots may be None); its w, h and slots may be the inputs themselves (in place).  image_flags (int32[n] CUDA,
        optional) gets 0 | 1."""
        return self._tiles_to_tiles("pxz_reshrink_varied_frames_device", sizes, channels, (), bw, bh, mode, filt, factor, expand_filter, ow, oh,
                                    slots, want_pixels, out, image_flags)

    def transcode_varied_files(self, files, bw, bh, mode, filt, factor, expand_filter, filter_byte=0, out=None):
        """pxz_transcode_varied_files: a list of .pixlzr files (bytes) of one channel count and block size -> the list of the
        files re-shrunk with (bw, bh, mode, filt, factor) after to_image(expand_filter).  out: a numpy uint8 buffer to write
        into (the call raises PxzError -7 with .needed when it is too small; out of size 0 is the size query), else the
        buffer is sized by a first call."""
        n = len(files)
        bufs = [np.frombuffer(bytes(f), np.uint8) for f in files]
        ptrs = (C.c_void_p * max(n, 1))(*[b.ctypes.data if b.size else None for b in bufs])
        lens = (C.c_size_t * max(n, 1))(*[b.size for b in bufs])
        pd = Params(bw, bh, mode, filt, factor, 0)
        offs = np.zeros(n + 1, np.uint64)

        def call(buf):
            return self._L.pxz_transcode_varied_files(self._h, C.cast(ptrs, C.c_void_p), C.cast(lens, C.c_void_p), n, C.byref(pd),
                                                      expand_filter, filter_byte, _p(buf) if buf is not None and buf.size else None,
                                                      0 if buf is None else buf.size, _p(offs))
        if out is None:
            rc = call(None)
            if rc == -7:
                out = np.empty(int(offs[-1]), np.uint8)
                rc = call(out)
        else:
            rc = call(out)
        if rc != 0:
            err = PxzError(rc, (self._L.pxz_last_error(self._h) or b"").decode())
            err.needed = int(offs[-1])
            raise err
        return [out[int(offs[i]):int(offs[i + 1])].tobytes() for i in range(n)]

    # ---- re-tile: stored tiles at one block size to stored tiles at another ----
    def retile_varied_frames_device(self, sizes, channels, src_bw, src_bh, bw, bh, mode, filt, factor, expand_filter, ow, oh, slots,
                                    want_pixels=True, out=None, image_flags=None):
        """pxz_retile_varied_frames_device: the stored tiles (w[S], h[S], slots[S, src_bw*src_bh*C], varied layout at
        src_bw x src_bh) of the images sizes = [(width, height), ...] expanded with expand_filter and shrunk again with (mode,
        filt, factor) at the block bw x bh, without the images.  Returns (tile_offsets uint64[n+1], values[T], w[T], h[T],
        slots[T, bw*bh*C] | None) in the varied layout at bw x bh.  out: a 4-tuple of such tensors (slots may be None), none of
        them an input.  image_flags (int32[n] CUDA, optional) gets 0 | 1."""
        return self._tiles_to_tiles("pxz_retile_varied_frames_device", sizes, channels, (src_bw, src_bh), bw, bh, mode, filt, factor,
                                    expand_filter, ow, oh, slots, want_pixels, out, image_flags)

    # ---- re-tile ladder: stored tiles at one block size to stored tiles at another, at several factors ----
    def retile_varied_ladder_frames_device(self, sizes, channels, src_bw, src_bh, bw, bh, mode, filt, factors, expand_filter, ow, oh, slots,
                                           want_pixels=True, out=None, image_flags=None, n_factors=None):
        """pxz_retile_varied_ladder_frames_device: retile_varied_frames_device at every factor of `factors` (a host sequence,
        1..32 of them) in one launch.  Returns (tile_offsets uint64[n+1], values[K,T], w[K,T], h[K,T], slots[K,T,bw*bh*C] |
        None) in the varied layout at bw x bh; rung r equals retile_varied_frames_device(..., factors[r], ...).  out: a 4-tuple
        of such tensors (slots may be None), none of them an input.  factors None with n_factors passes a null pointer."""
        return self._tiles_to_tiles("pxz_retile_varied_ladder_frames_device", sizes, channels, (src_bw, src_bh), bw, bh, mode, filt, 0.0,
                                    expand_filter, ow, oh, slots, want_pixels, out, image_flags, ladder=(factors, n_factors))

    # ---- re-shrink ladder: stored tiles to stored tiles at several factors ----
    def reshrink_varied_ladder_frames_device(self, sizes, channels, bw, bh, mode, filt, factors, expand_filter, ow, oh, slots,
                                             want_pixels=True, out=None, image_flags=None, n_factors=None):
        """pxz_reshrink_varied_ladder_frames_device: reshrink_varied_frames_device at every factor of `factors` (a host
        sequence, 1..32 of them) in one launch.  Returns (tile_offsets uint64[n+1], values[K,T], w[K,T], h[K,T],
        slots[K,T,bw*bh*C] | None); rung r equals reshrink_varied_frames_device(..., factors[r], ...).  out: a 4-tuple of such
        tensors (slots may be None); ow, oh and slots may be rung 0 of its w, h and slots (in place).  factors None with
        n_factors passes a null pointer."""
        return self._tiles_to_tiles("pxz_reshrink_varied_ladder_frames_device", sizes, channels, (), bw, bh, mode, filt, 0.0, expand_filter,
                                    ow, oh, slots, want_pixels, out, image_flags, ladder=(factors, n_factors))

    def transcode_varied_ladder_files(self, files, bw, bh, mode, filt, factors, expand_filter, filter_byte=0, out=None, sizes_only=False):
        """pxz_transcode_varied_ladder_files: transcode_varied_files at every factor of `factors` -> a list per rung of the
        list of new files.  sizes_only: the size query alone -- returns the rate table, int64[K, n] file lengths, and keeps no
        file.  out: a numpy uint8 buffer to write into (PxzError -7 with .needed and .offsets when it is too small), else
        the buffer is sized by a first call."""
        n = len(files)
        bufs = [np.frombuffer(bytes(f), np.uint8) for f in files]
        ptrs = (C.c_void_p * max(n, 1))(*[b.ctypes.data if b.size else None for b in bufs])
        lens = (C.c_size_t * max(n, 1))(*[b.size for b in bufs])
        fac = np.ascontiguousarray(factors, np.float32)
        K = fac.size
        pd = Params(bw, bh, mode, filt, 0.0, 0)
        offs = np.zeros(K * n + 1, np.uint64)

        def call(buf):
            return self._L.pxz_transcode_varied_ladder_files(self._h, C.cast(ptrs, C.c_void_p), C.cast(lens, C.c_void_p), n, C.byref(pd),
                                                             expand_filter, _p(fac) if K else None, K, filter_byte,
                                                             _p(buf) if buf is not None and buf.size else None,
                                                             0 if buf is None else buf.size, _p(offs))
        if out is None:
            rc = call(None)
            if rc == -7 and sizes_only:
                return np.diff(offs.astype(np.int64)).reshape(K, n)
            if rc == -7:
                out = np.empty(int(offs[-1]), np.uint8)
                rc = call(out)
        else:
            rc = call(out)
        if rc != 0:
            err = PxzError(rc, (self._L.pxz_last_error(self._h) or b"").decode())
            err.needed, err.offsets = int(offs[-1]), offs.copy()
            raise err
        return [[out[int(offs[r * n + i]):int(offs[r * n + i + 1])].tobytes() for i in range(n)] for r in range(K)]

    # ---- windows of files ----
    def decode_windows_device(self, files, file_offsets, sizes, windows, channels, bw, bh, out=None, window_flags=None):
        """pxz_decode_windows_device: files / file_offsets / sizes as decode_varied_frames_device, windows = [(image, x, y,
        width, height, pitch_bytes, offset_bytes), ...].  Only the tiles the windows cover are read: returns (tile_offsets
        uint64[k+1], values[T], w[T], h[T], slots[T, bw*bh*C]) in the window_layout order; window_flags (int32[k] CUDA,
        optional) gets 0 | 2.  out: a 4-tuple of such tensors."""
        import torch
        geoms = [(w, h, 0, 0) for (w, h) in sizes]
        offs = None
        if out is None:
            offs = window_layout(sizes, windows, bw, bh)
            T = int(offs[-1])
            dev = files.device
            vals = torch.zeros(T, dtype=torch.float32, device=dev)
            ow = torch.zeros(T, dtype=torch.int32, device=dev)
            oh = torch.zeros(T, dtype=torch.int32, device=dev)
            slots = torch.zeros((T, bw * bh * channels), dtype=torch.uint8, device=dev)
        else:
            vals, ow, oh, slots = out
        pd = Params(bw, bh, 0, 0, 0.0, 0)
        self.use_torch_stream()
        self._check(self._L.pxz_decode_windows_device(
            self._h, C.cast(image_descs(geoms), C.c_void_p), len(geoms), C.cast(window_descs(windows), C.c_void_p), len(windows),
            channels, C.byref(pd), C.c_void_p(files.data_ptr()), C.c_void_p(file_offsets.data_ptr()), C.c_void_p(vals.data_ptr()),
            C.c_void_p(ow.data_ptr()), C.c_void_p(oh.data_ptr()), C.c_void_p(slots.data_ptr()),
            C.c_void_p(window_flags.data_ptr()) if window_flags is not None else None))
        if offs is None:
            offs = window_layout(sizes, windows, bw, bh)
        return offs, vals, ow, oh, slots

    def expand_windows_device(self, sizes, windows, channels, bw, bh, filt, ow, oh, slots, out, window_flags=None):
        """pxz_expand_windows_device: the covered tiles of the windows (w[T], h[T], slots[T, bw*bh*C], window_layout order)
        -> the windows' pixels, written into the uint8 CUDA buffer `out` at each window's offset_bytes with its pitch_bytes
        between rows.  window_flags (int32[k] CUDA, optional) gets 0 | 1.  Returns out."""
        geoms = [(w, h, 0, 0) for (w, h) in sizes]
        pd = Params(bw, bh, 0, filt, 0.0, 0)
        self.use_torch_stream()
        self._check(self._L.pxz_expand_windows_device(
            self._h, C.cast(image_descs(geoms), C.c_void_p), len(geoms), C.cast(window_descs(windows), C.c_void_p), len(windows),
            channels, C.byref(pd), C.c_void_p(ow.data_ptr()), C.c_void_p(oh.data_ptr()), C.c_void_p(slots.data_ptr()),
            C.c_void_p(out.data_ptr()), C.c_void_p(window_flags.data_ptr()) if window_flags is not None else None))
        return out

    def decode_windows_files(self, files, windows, channels, bw, bh, filt, sizes=None, out=None):
        """pxz_decode_windows_files: a list of .pixlzr files (bytes) of one channel count and block size, and windows =
        [(image, x, y, width, height), ...] -> a list of (height, width, channels) crops.  sizes defaults to what the headers
        say (file_header).  With out (a numpy uint8 buffer) the windows carry pitch_bytes and offset_bytes too and are written
        there instead.  Returns (crops | out, flags uint32[k]); raises PxzError (with .flags, .crops) when a file is refused or
        a window comes back flagged."""
        n, k = len(files), len(windows)
        bufs = [np.frombuffer(bytes(f), np.uint8) for f in files]
        if sizes is None:
            sizes = [file_header(f)[:2] for f in files]
        own = out is None
        if own:
            full, at = [], 0
            for (i, x, y, w, h) in windows:
                full.append((i, x, y, w, h, w * channels, at))
                at += w * h * channels
            windows = full
            out = np.zeros(max(at, 1), np.uint8)
        ptrs = (C.c_void_p * max(n, 1))(*[b.ctypes.data if b.size else None for b in bufs])
        lens = (C.c_size_t * max(n, 1))(*[b.size for b in bufs])
        flags = np.zeros(max(k, 1), np.uint32)
        pd = Params(bw, bh, 0, filt, 0.0, 0)
        geoms = [(w, h, 0, 0) for (w, h) in sizes]
        rc = self._L.pxz_decode_windows_files(self._h, C.cast(ptrs, C.c_void_p), C.cast(lens, C.c_void_p),
                                              C.cast(image_descs(geoms), C.c_void_p), n, C.cast(window_descs(windows), C.c_void_p), k,
                                              channels, C.byref(pd), _p(out), out.size, _p(flags))
        if own:
            result = [out[w[6]:w[6] + w[3] * w[4] * channels].reshape(w[4], w[3], channels) for w in windows]
        else:
            result = out
        if rc != 0:
            err = PxzError(rc, (self._L.pxz_last_error(self._h) or b"").decode())
            err.flags, err.crops = flags[:k], result
            raise err
        return result, flags[:k]

    # ---- patch: new pixels into windows of files ----
    def patch_windows_device(self, sizes, windows, channels, bw, bh, mode, filt, factor, expand_filter, patch, ow, oh, slots,
                             want_pixels=True, out=None, window_flags=None):
        """pxz_patch_windows_device: the covered tiles of the windows (w[T], h[T], slots[T, bw*bh*C], window_layout order, as
        decode_windows_device leaves them) with the windows' new pixels written over them -- window k's width x height pixels
        stand in the uint8 CUDA buffer `patch` at its offset_bytes with its pitch_bytes between rows -- shrunk again with (mode,
        filt, factor) after the expand with expand_filter.  Returns (values[T], w[T], h[T], slots | None).  out: a 4-tuple of
        such tensors (slots may be None); its w, h and slots may be the inputs themselves (in place).  window_flags (int32[k]
        CUDA, optional) gets 0 | 1."""
        import torch
        geoms = [(w, h, 0, 0) for (w, h) in sizes]
        if out is None:
            T = ow.numel()
            dev = ow.device
            vals = torch.empty(T, dtype=torch.float32, device=dev)
            nw = torch.empty(T, dtype=torch.int32, device=dev)
            nh = torch.empty(T, dtype=torch.int32, device=dev)
            nslots = torch.empty((T, bw * bh * channels), dtype=torch.uint8, device=dev) if want_pixels else None
        else:
            vals, nw, nh, nslots = out
        pd = Params(bw, bh, mode, filt, factor, 0)
        self.use_torch_stream()
        self._check(self._L.pxz_patch_windows_device(
            self._h, C.cast(image_descs(geoms), C.c_void_p), len(geoms), C.cast(window_descs(windows), C.c_void_p), len(windows),
            channels, C.byref(pd), expand_filter, C.c_void_p(patch.data_ptr()), C.c_void_p(ow.data_ptr()), C.c_void_p(oh.data_ptr()),
            C.c_void_p(slots.data_ptr()), C.c_void_p(vals.data_ptr()), C.c_void_p(nw.data_ptr()), C.c_void_p(nh.data_ptr()),
            C.c_void_p(nslots.data_ptr()) if nslots is not None else None,
            C.c_void_p(window_flags.data_ptr()) if window_flags is not None else None))
        return vals, nw, nh, nslots

    def splice_windows_device(self, files, file_offsets, sizes, windows, channels, bw, bh, vals, ow, oh, slots, reader_flags=None,
                              patch_flags=None, out=None, image_flags=None):
        """pxz_splice_windows_device: the old files (files / file_offsets as decode_windows_device took them -- the call must
        follow that reader on this handle) and the new covered tiles (values[T], w[T], h[T], slots, window_layout order) -> the
        new files.  out: (file_offsets int64[n+1], bytes uint8[capacity]) CUDA tensors (bytes may be None: the size query); by
        default the buffer holds the old files and every covered record at its largest.  Returns (file_offsets, bytes)."""
        import torch
        geoms = [(w, h, 0, 0) for (w, h) in sizes]
        n = len(geoms)
        if out is None:
            T = vals.numel()
            cap = files.numel() + T * (13 + 14 + bw * bh * (channels + 1) + 8)
            offs = torch.empty(n + 1, dtype=torch.int64, device=vals.device)
            buf = torch.empty(cap, dtype=torch.uint8, device=vals.device)
        else:
            offs, buf = out
        opt = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
        pd = Params(bw, bh, 0, 0, 0.0, 0)
        self.use_torch_stream()
        self._check(self._L.pxz_splice_windows_device(
            self._h, C.cast(image_descs(geoms), C.c_void_p), n, C.cast(window_descs(windows), C.c_void_p), len(windows), channels,
            C.byref(pd), C.c_void_p(files.data_ptr()), C.c_void_p(file_offsets.data_ptr()), C.c_void_p(vals.data_ptr()),
            C.c_void_p(ow.data_ptr()), C.c_void_p(oh.data_ptr()), C.c_void_p(slots.data_ptr()), opt(reader_flags), opt(patch_flags),
            opt(buf), 0 if buf is None else buf.numel(), C.c_void_p(offs.data_ptr()), opt(image_flags)))
        return offs, buf

    def patch_windows_files(self, files, windows, patches, bw, bh, mode, filt, factor, expand_filter, out=None):
        """pxz_patch_windows_files: a list of .pixlzr files (bytes) of one channel count and block size, windows = [(image, x, y,
        width, height), ...] and patches = their new pixels (numpy uint8 [height, width, C]) -> the list of the patched files.
        out: a numpy uint8 buffer to write into (the call raises PxzError -7 with .needed when it is too small; out of size 0 is
        the size query), else the buffer is sized by a first call.  Raises PxzError naming the window when one is flagged."""
        n, k = len(files), len(windows)
        bufs = [np.frombuffer(bytes(f), np.uint8) for f in files]
        ptrs = (C.c_void_p * max(n, 1))(*[b.ctypes.data if b.size else None for b in bufs])
        lens = (C.c_size_t * max(n, 1))(*[b.size for b in bufs])
        pats = [p if p.strides[2] == 1 and p.strides[1] == p.shape[2] else np.ascontiguousarray(p) for p in patches]
        pptrs = (C.c_void_p * max(k, 1))(*[p.ctypes.data for p in pats])
        full = [(i, x, y, w, h, pats[j].strides[0], 0) for j, (i, x, y, w, h) in enumerate(windows)]
        pd = Params(bw, bh, mode, filt, factor, 0)
        offs = np.zeros(n + 1, np.uint64)

        def call(buf):
            return self._L.pxz_patch_windows_files(self._h, C.cast(ptrs, C.c_void_p), C.cast(lens, C.c_void_p), n,
                                                   C.cast(window_descs(full), C.c_void_p), k, C.cast(pptrs, C.c_void_p), C.byref(pd),
                                                   expand_filter, _p(buf) if buf is not None and buf.size else None,
                                                   0 if buf is None else buf.size, _p(offs))
        if out is None:
            rc = call(None)
            if rc == -7:
                out = np.empty(int(offs[-1]), np.uint8)
                rc = call(out)
        else:
            rc = call(out)
        if rc != 0:
            err = PxzError(rc, (self._L.pxz_last_error(self._h) or b"").decode())
            err.needed, err.offsets = int(offs[-1]), offs.copy()
            raise err
        return [out[int(offs[i]):int(offs[i + 1])].tobytes() for i in range(n)]

    # ---- decode at reduced scale ----
    def expand_varied_scaled_frames_device(self, descs, channels, bw, bh, filt, scales, ow, oh, slots, out, image_flags=None):
        """pxz_expand_varied_scaled_frames_device: expand_varied_frames_device with image i written at 1/2^scales[i].  descs =
        [(file width, file height, pitch_bytes, offset_bytes), ...]: pitch and offset describe the SCALED image.  Returns out."""
        geoms = [tuple(d) for d in descs]
        pd = Params(bw, bh, 0, filt, 0.0, 0)
        self.use_torch_stream()
        self._check(self._L.pxz_expand_varied_scaled_frames_device(
            self._h, C.cast(image_descs(geoms), C.c_void_p), len(geoms), channels, C.byref(pd), C.cast(_u32s(scales), C.c_void_p),
            C.c_void_p(ow.data_ptr()), C.c_void_p(oh.data_ptr()), C.c_void_p(slots.data_ptr()), C.c_void_p(out.data_ptr()),
            C.c_void_p(image_flags.data_ptr()) if image_flags is not None else None))
        return out

    def expand_windows_scaled_device(self, sizes, windows, channels, bw, bh, filt, scales, ow, oh, slots, out, window_flags=None):
        """pxz_expand_windows_scaled_device: expand_windows_device with window k written at 1/2^scales[k].  The windows are the
        full-resolution rectangles of window_layout; pitch and offset describe the SCALED crop.  Returns out."""
        geoms = [(w, h, 0, 0) for (w, h) in sizes]
        pd = Params(bw, bh, 0, filt, 0.0, 0)
        self.use_torch_stream()
        self._check(self._L.pxz_expand_windows_scaled_device(
            self._h, C.cast(image_descs(geoms), C.c_void_p), len(geoms), C.cast(window_descs(windows), C.c_void_p), len(windows),
            channels, C.byref(pd), C.cast(_u32s(scales), C.c_void_p), C.c_void_p(ow.data_ptr()), C.c_void_p(oh.data_ptr()),
            C.c_void_p(slots.data_ptr()), C.c_void_p(out.data_ptr()),
            C.c_void_p(window_flags.data_ptr()) if window_flags is not None else None))
        return out

    def decode_varied_files_scaled(self, files, channels, bw, bh, filt, scales, sizes=None, out=None, descs=None):
        """pxz_decode_varied_files_scaled: decode_varied_files with image i decoded at 1/2^scales[i] -> a list of (ceil(height/s),
        ceil(width/s), channels) images.  sizes (the FILES') defaults to what the headers say; with out and descs = [(file width,
        file height, pitch_bytes, offset_bytes), ...] the scaled images are written there instead.  Returns (images | out, flags);
        raises PxzError (with .flags) when a file is refused or malformed."""
        n = len(files)
        bufs = [np.frombuffer(bytes(f), np.uint8) for f in files]
        if sizes is None and descs is None:
            sizes = [file_header(f)[:2] for f in files]
        own = descs is None
        if own:
            descs, shapes, at = [], [], 0
            for (w, h), k in zip(sizes, scales):
                sw, sh = -(-w // (1 << k)), -(-h // (1 << k))
                descs.append((w, h, sw * channels, at))
                shapes.append((sw, sh))
                at += sw * sh * channels
            out = np.zeros(max(at, 1), np.uint8)
        ptrs = (C.c_void_p * max(n, 1))(*[b.ctypes.data if b.size else None for b in bufs])
        lens = (C.c_size_t * max(n, 1))(*[b.size for b in bufs])
        flags = np.zeros(max(n, 1), np.uint32)
        pd = Params(bw, bh, 0, filt, 0.0, 0)
        rc = self._L.pxz_decode_varied_files_scaled(self._h, C.cast(ptrs, C.c_void_p), C.cast(lens, C.c_void_p),
                                                    C.cast(image_descs(descs), C.c_void_p), n, channels, C.byref(pd),
                                                    C.cast(_u32s(scales), C.c_void_p), _p(out), _p(flags))
        if own:
            result = [out[d[3]:d[3] + sw * sh * channels].reshape(sh, sw, channels) for d, (sw, sh) in zip(descs, shapes)]
        else:
            result = out
        if rc != 0:
            err = PxzError(rc, (self._L.pxz_last_error(self._h) or b"").decode())
            err.flags, err.images = flags[:n], result
            raise err
        return result, flags[:n]

    def decode_windows_files_scaled(self, files, windows, channels, bw, bh, filt, scales, sizes=None, out=None):
        """pxz_decode_windows_files_scaled: decode_windows_files with window k decoded at 1/2^scales[k]; windows = [(image, x, y,
        width, height), ...] in full-resolution pixels -> a list of scaled crops.  With out (a numpy uint8 buffer) the windows
        carry the pitch_bytes and offset_bytes of their scaled crops too.  Returns (crops | out, flags uint32[k]); raises PxzError
        (with .flags, .crops) when a file is refused or a window comes back flagged."""
        n, k = len(files), len(windows)
        bufs = [np.frombuffer(bytes(f), np.uint8) for f in files]
        if sizes is None:
            sizes = [file_header(f)[:2] for f in files]
        own = out is None
        shapes = [scaled_window_size(w, s) for w, s in zip(windows, scales)]
        if own:
            full, at = [], 0
            for (i, x, y, w, h), (sw, sh) in zip(windows, shapes):
                full.append((i, x, y, w, h, sw * channels, at))
                at += sw * sh * channels
            windows = full
            out = np.zeros(max(at, 1), np.uint8)
        ptrs = (C.c_void_p * max(n, 1))(*[b.ctypes.data if b.size else None for b in bufs])
        lens = (C.c_size_t * max(n, 1))(*[b.size for b in bufs])
        flags = np.zeros(max(k, 1), np.uint32)
        pd = Params(bw, bh, 0, filt, 0.0, 0)
        geoms = [(w, h, 0, 0) for (w, h) in sizes]
        rc = self._L.pxz_decode_windows_files_scaled(self._h, C.cast(ptrs, C.c_void_p), C.cast(lens, C.c_void_p),
                                                     C.cast(image_descs(geoms), C.c_void_p), n, C.cast(window_descs(windows), C.c_void_p), k,
                                                     channels, C.byref(pd), C.cast(_u32s(scales), C.c_void_p), _p(out), out.size, _p(flags))
        if own:
            result = [out[w[6]:w[6] + sw * sh * channels].reshape(sh, sw, channels) for w, (sw, sh) in zip(windows, shapes)]
        else:
            result = out
        if rc != 0:
            err = PxzError(rc, (self._L.pxz_last_error(self._h) or b"").decode())
            err.flags, err.crops = flags[:k], result
            raise err
        return result, flags[:k]

    # ---- rate and distortion ----
    def distortion_frames_device(self, frames, bw, bh, filt, ow, oh, slots, want_tiles=True, out=None):
        """pxz_distortion_frames_device: per tile and channel the sum of (source - expanded)^2 of stored tiles against the
        frames [N,H,W,C] they were shrunk from, `expanded` being what expand_frames_device(..., filt, ...) writes.  ow, oh:
        [N,T] or [K,N,T] as shrink_frames_device / shrink_ladder_frames_device leave them, slots [..., bw*bh*C].  Returns
        (tile_sse int64 [K,N,T,C] | None, frame_sse int64 [K,N,C]).  Real sums stay below 2^63; the entries of a tile whose
        stored size is zero or exceeds its place are all-ones and read as -1 (decode_status() bit 0 is set; the frame's
        totals leave such tiles out).  out: a (tile_sse | None, frame_sse) pair of such tensors."""
        import torch
        fd, (N, H, W, Cc) = self._frames_desc(frames)
        cols, rows = grid(W, H, bw, bh)
        T = cols * rows
        K = ow.numel() // (N * T) if N * T else 0
        assert ow.numel() == K * N * T and oh.numel() == ow.numel() and ow.is_contiguous() and oh.is_contiguous() and slots.is_contiguous()
        if out is None:
            tile_sse = torch.empty((K, N, T, Cc), dtype=torch.int64, device=frames.device) if want_tiles else None
            frame_sse = torch.empty((K, N, Cc), dtype=torch.int64, device=frames.device)
        else:
            tile_sse, frame_sse = out
        pd = Params(bw, bh, 0, filt, 0.0, 0)
        self.use_torch_stream()
        self._check(self._L.pxz_distortion_frames_device(
            self._h, C.byref(fd), C.byref(pd), K, C.c_void_p(frames.data_ptr()), C.c_void_p(ow.data_ptr()), C.c_void_p(oh.data_ptr()),
            C.c_void_p(slots.data_ptr()), C.c_void_p(tile_sse.data_ptr()) if tile_sse is not None else None,
            C.c_void_p(frame_sse.data_ptr())))
        return tile_sse, frame_sse

    def distortion_varied_frames_device(self, images, bw, bh, filt, ow, oh, slots, descs=None, channels=None, want_tiles=True,
                                        out=None, image_flags=None):
        """pxz_distortion_varied_frames_device: the same for the stored tiles (varied layout: w[T], h[T], slots[T, bw*bh*C]) of a
        list of differently sized CUDA images, or of one uint8 CUDA buffer with descs = [(width, height, pitch_bytes,
        offset_bytes), ...] and channels.  Returns (tile_sse int64 [T,C] | None, image_sse int64 [n,C]); all-ones entries read
        as -1 as above, and image_flags (int32[n] CUDA, optional) gets 1 for an image that holds such a tile."""
        import torch
        base, geoms, ch, keep = self._varied_batch(images, descs)
        ch = channels if channels is not None else ch
        if out is None:
            dev = torch.device("cuda", self.device_id)
            tile_sse = torch.empty((ow.numel(), ch), dtype=torch.int64, device=dev) if want_tiles else None
            image_sse = torch.empty((len(geoms), ch), dtype=torch.int64, device=dev)
        else:
            tile_sse, image_sse = out
        pd = Params(bw, bh, 0, filt, 0.0, 0)
        self.use_torch_stream()
        self._check(self._L.pxz_distortion_varied_frames_device(
            self._h, C.cast(image_descs(geoms), C.c_void_p), len(geoms), ch, C.byref(pd), C.c_void_p(base), C.c_void_p(ow.data_ptr()),
            C.c_void_p(oh.data_ptr()), C.c_void_p(slots.data_ptr()), C.c_void_p(tile_sse.data_ptr()) if tile_sse is not None else None,
            C.c_void_p(image_sse.data_ptr()), C.c_void_p(image_flags.data_ptr()) if image_flags is not None else None))
        del keep
        return tile_sse, image_sse

    def rate_distortion_image(self, img, bw, bh, mode, filter_down, filter_up, factors):
        """pxz_rate_distortion_image: a host image (numpy uint8 [H,W,C]) at every factor of `factors` (1..16) ->
        (file_bytes uint64[K], sse uint64[K,C]): the length of the .pixlzr file of each factor and the squared error per
        channel of the image that file expands to with filter_up.  psnr(sse[r].sum(), H*W*C) is the rung's PSNR."""
        if img.strides[2] != 1 or img.strides[1] != img.shape[2]:
            img = np.ascontiguousarray(img)
        H, W, Cc = img.shape
        fac = np.ascontiguousarray(factors, np.float32)
        K = fac.size
        file_bytes = np.zeros(max(K, 1), np.uint64)
        sse = np.zeros((max(K, 1), Cc), np.uint64)
        self._check(self._L.pxz_rate_distortion_image(self._h, C.c_void_p(img.ctypes.data), W, H, Cc, img.strides[0], bw, bh, mode,
                                                      filter_down, filter_up, _p(fac) if K else None, K, _p(file_bytes), _p(sse)))
        return file_bytes[:K], sse[:K]

    def rate_distortion_varied_images(self, imgs, bw, bh, mode, filter_down, filter_up, factors):
        """pxz_rate_distortion_varied_images: host images (numpy uint8 [H,W,C], one channel count) at every factor of `factors`
        (1..32) -> (file_bytes uint64[K,n], sse uint64[K,n,C]): what rate_distortion_image gives per image and factor."""
        imgs = [np.ascontiguousarray(i) if i.strides[1] != i.shape[2] or i.strides[2] != 1 else i for i in imgs]
        n = len(imgs)
        ch = imgs[0].shape[2] if n else 4
        geoms = [(i.shape[1], i.shape[0], i.strides[0], 0) for i in imgs]
        ptrs = (C.c_void_p * max(n, 1))(*[i.ctypes.data for i in imgs])
        fac = np.ascontiguousarray(factors, np.float32)
        K = fac.size
        file_bytes = np.zeros((max(K, 1), max(n, 1)), np.uint64)
        sse = np.zeros((max(K, 1), max(n, 1), ch), np.uint64)
        self._check(self._L.pxz_rate_distortion_varied_images(
            self._h, C.cast(ptrs, C.c_void_p), C.cast(image_descs(geoms), C.c_void_p), n, ch, bw, bh, mode, filter_down, filter_up,
            _p(fac) if K else None, K, _p(file_bytes), _p(sse)))
        return file_bytes[:K, :n], sse[:K, :n]

    # ---- fit to a budget ----
    def fit_varied_ladder_device(self, file_offsets, image_sse, criterion, targets, n_images=None, n_factors=None, channels=None,
                                 out=None):
        """pxz_fit_varied_ladder_device: fit_select on the device.  file_offsets int64[K*n + 1] (encode_varied_frames_device
        over the images repeated K times) and image_sse int64[K, n, C] (distortion_varied_frames_device over the same) are
        CUDA tensors, targets n host integers -> (choice int32[n], fit_flags int32[n]) CUDA tensors, or out = such a pair.
        n_images, n_factors and channels override what image_sse's shape says; None for targets or a tensor passes a null
        pointer."""
        import torch
        K = n_factors if n_factors is not None else image_sse.shape[0]
        n = n_images if n_images is not None else image_sse.shape[1]
        ch = channels if channels is not None else image_sse.shape[2]
        tg = None if targets is None else np.array([int(t) for t in targets], np.uint64)
        if out is None:
            dev = torch.device("cuda", self.device_id)
            out = (torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev))
        choice, flags = out
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
        self.use_torch_stream()
        self._check(self._L.pxz_fit_varied_ladder_device(self._h, n, K, ch, criterion, _p(tg), ptr(file_offsets), ptr(image_sse),
                                                         ptr(choice), ptr(flags)))
        return choice, flags

    def gather_varied_rungs_device(self, sizes, channels, bw, bh, n_factors, choice, vals, ow, oh, slots, out=None, image_flags=None,
                                   want_pixels=True):
        """pxz_gather_varied_rungs_device: sizes = [(width, height), ...] of the images (or full (width, height, pitch_bytes,
        offset_bytes[, reserved]) tuples), choice int32[n] CUDA, and the rung-major tensors of
        shrink_varied_ladder_frames_device (values[K,T], w[K,T], h[K,T], slots[K,T,bw*bh*C]) -> (values[T], w[T], h[T],
        slots[T, bw*bh*C] | None) in the varied layout of the images: tile t of image i from rung choice[i].  out: such a
        4-tuple; image_flags (int32[n] CUDA, optional) gets 2 for an image whose choice was n_factors or more, else 0."""
        import torch
        geoms = [tuple(s) if len(s) > 2 else (s[0], s[1], s[0] * channels, 0) for s in sizes]
        if out is None:
            T = int(varied_layout(geoms, bw, bh)[-1])
            dev = vals.device
            out = (torch.empty(T, dtype=torch.float32, device=dev), torch.empty(T, dtype=torch.int32, device=dev),
                   torch.empty(T, dtype=torch.int32, device=dev),
                   torch.empty((T, bw * bh * channels), dtype=torch.uint8, device=dev) if want_pixels else None)
        o_vals, o_w, o_h, o_slots = out
        pd = Params(bw, bh, 0, 0, 0.0, 0)
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
        self.use_torch_stream()
        self._check(self._L.pxz_gather_varied_rungs_device(
            self._h, C.cast(image_descs(geoms), C.c_void_p), len(geoms), channels, C.byref(pd), n_factors, ptr(choice), ptr(vals),
            ptr(ow), ptr(oh), ptr(slots), ptr(o_vals), ptr(o_w), ptr(o_h), ptr(o_slots), ptr(image_flags)))
        return o_vals, o_w, o_h, o_slots

    def encode_varied_images_fit(self, imgs, bw, bh, mode, filter_down, filter_up, factors, criterion, targets, filter_byte=0,
                                 want_table=False):
        """pxz_encode_varied_images_fit: host images (numpy uint8 [H, W, C], one channel count) -> one .pixlzr file per image,
        each at the factor of `factors` (1..32) that fit_select picks under targets[i] (n host integers).  Returns (files: a
        list of bytes, choice uint32[n], fit_flags uint32[n]) and, with want_table, (file_bytes uint64[K,n], sse
        uint64[K,n,C]) as rate_distortion_varied_images returns them."""
        imgs = [np.ascontiguousarray(i) if i.strides[1] != i.shape[2] or i.strides[2] != 1 else i for i in imgs]
        n = len(imgs)
        ch = imgs[0].shape[2] if n else 4
        geoms = [(i.shape[1], i.shape[0], i.strides[0], 0) for i in imgs]
        ptrs = (C.c_void_p * max(n, 1))(*[i.ctypes.data for i in imgs])
        descs = image_descs(geoms)
        fac = np.ascontiguousarray(factors, np.float32)
        K = fac.size
        tg = np.array([int(t) for t in targets], np.uint64)
        offs = np.zeros(n + 1, np.uint64)
        choice, flags = np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.uint32)
        table_bytes = np.zeros((max(K, 1), max(n, 1)), np.uint64) if want_table else None
        table_sse = np.zeros((max(K, 1), max(n, 1), ch), np.uint64) if want_table else None
        buf = np.empty(sum(i.size for i in imgs) * 5 // 4 + 4096 * max(n, 1), np.uint8)
        for attempt in range(2):  # (a second call only when the first guess at the files' size was short)
            rc = self._L.pxz_encode_varied_images_fit(
                self._h, C.cast(ptrs, C.c_void_p), C.cast(descs, C.c_void_p), n, ch, bw, bh, mode, filter_down, filter_up,
                _p(fac) if K else None, K, criterion, _p(tg) if tg.size else None, filter_byte, _p(buf), buf.size, _p(offs), _p(choice),
                _p(flags), _p(table_bytes), _p(table_sse))
            if rc != -7 or attempt == 1:
                break
            buf = np.empty(int(offs[-1]), np.uint8)
        self._check(rc)
        files = [buf[int(offs[i]):int(offs[i + 1])].tobytes() for i in range(n)]
        if want_table:
            return files, choice[:n], flags[:n], table_bytes[:K, :n], table_sse[:K, :n]
        return files, choice[:n], flags[:n]

    # ---- fit an archive to a budget ----
    def _archive_distortion(self, entry, sizes, channels, src_block, bw, bh, expand_filter, filter_up, ref_w, ref_h, ref_slots, ow, oh, slots,
                            want_tiles, out, image_flags, n_sets):
        """both archive distortions: the library's `entry` with src_block = (src_bw, src_bh) where the block changes (else ())"""
        import torch
        geoms = [tuple(s) if len(s) > 2 else (s[0], s[1], s[0] * channels, 0) for s in sizes]
        n = len(geoms)
        T = int(varied_layout([g[:4] for g in geoms], bw, bh)[-1]) if n and out is None else 0
        K = n_sets if n_sets is not None else (ow.numel() // T if T else ow.shape[0])
        if out is None:
            dev = torch.device("cuda", self.device_id)
            tile_sse = torch.empty((K, T, channels), dtype=torch.int64, device=dev) if want_tiles else None
            image_sse = torch.empty((K, n, channels), dtype=torch.int64, device=dev)
        else:
            tile_sse, image_sse = out
        pd = Params(bw, bh, 0, filter_up, 0.0, 0)
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
        self.use_torch_stream()
        self._check(getattr(self._L, entry)(
            self._h, C.cast(image_descs(geoms), C.c_void_p) if n else None, n, channels, *src_block, C.byref(pd), expand_filter, K, ptr(ref_w),
            ptr(ref_h), ptr(ref_slots), ptr(ow), ptr(oh), ptr(slots), ptr(tile_sse), ptr(image_sse), ptr(image_flags)))
        return tile_sse, image_sse

    def reshrink_distortion_varied_device(self, sizes, channels, bw, bh, expand_filter, filter_up, ref_w, ref_h, ref_slots, ow, oh,
                                          slots, want_tiles=True, out=None, image_flags=None, n_sets=None):
        """pxz_reshrink_distortion_varied_device: sizes = [(width, height), ...] of the images; the archive's stored tiles
        (ref_w[T], ref_h[T], ref_slots[T, bw*bh*C], varied layout) against n_sets stored versions of them (ow[K,T], oh[K,T],
        slots[K,T,bw*bh*C], as reshrink_varied_ladder_frames_device leaves its rungs): per tile, set and channel the sum of
        (expand(reference, expand_filter) - expand(set, filter_up))^2.  Returns (tile_sse int64[K,T,C] | None, image_sse
        int64[K,n,C]); all-ones entries read as -1; image_flags (int32[n] CUDA, optional) gets 0 | 1.  out: such a pair.
        n_sets overrides what ow's shape says; None for a tensor passes a null pointer."""
        return self._archive_distortion("pxz_reshrink_distortion_varied_device", sizes, channels, (), bw, bh, expand_filter, filter_up, ref_w,
                                        ref_h, ref_slots, ow, oh, slots, want_tiles, out, image_flags, n_sets)

    def retile_distortion_varied_device(self, sizes, channels, src_bw, src_bh, bw, bh, expand_filter, filter_up, ref_w, ref_h,
                                        ref_slots, ow, oh, slots, want_tiles=True, out=None, image_flags=None, n_sets=None):
        """pxz_retile_distortion_varied_device: reshrink_distortion_varied_device for a block size that changes: the archive's
        stored tiles in the layout of src_bw x src_bh blocks (ref_w[Ts], ref_h[Ts], ref_slots[Ts, src_bw*src_bh*C]) against n_sets
        stored versions of the tiles of the bw x bh grid (ow[K,T], oh[K,T], slots[K,T,bw*bh*C], as
        retile_varied_ladder_frames_device leaves its rungs).  Returns, out, image_flags and n_sets as there, T being the tiles
        of the bw x bh grid."""
        return self._archive_distortion("pxz_retile_distortion_varied_device", sizes, channels, (src_bw, src_bh), bw, bh, expand_filter,
                                        filter_up, ref_w, ref_h, ref_slots, ow, oh, slots, want_tiles, out, image_flags, n_sets)

    def rate_distortion_retile_files(self, files, bw, bh, mode, filter_down, expand_filter, filter_up, factors):
        """pxz_rate_distortion_retile_files: rate_distortion_varied_files with bw x bh the NEW block size (the files' own comes
        from their headers): the length of each file re-tiled at every factor and its squared error against what the file
        decodes to now."""
        return self.rate_distortion_varied_files(files, bw, bh, mode, filter_down, expand_filter, filter_up, factors,
                                                 _entry="pxz_rate_distortion_retile_files")

    def retile_varied_files_fit(self, files, bw, bh, mode, filter_down, expand_filter, filter_up, factors, criterion, targets,
                                filter_byte=0, want_table=False, out=None):
        """pxz_retile_varied_files_fit: transcode_varied_files_fit with bw x bh the NEW block size; returns and out as there."""
        return self.transcode_varied_files_fit(files, bw, bh, mode, filter_down, expand_filter, filter_up, factors, criterion, targets,
                                               filter_byte=filter_byte, want_table=want_table, out=out, _entry="pxz_retile_varied_files_fit")

    def retile_varied_files_fit_tiles(self, files, bw, bh, mode, filter_down, expand_filter, filter_up, factors, criterion, targets,
                                      group_first=None, filter_byte=0, out=None):
        """pxz_retile_varied_files_fit_tiles: transcode_varied_files_fit_tiles with bw x bh the NEW block size (tile_choice: the
        tiles of the new grid); returns and out as there."""
        return self.transcode_varied_files_fit_tiles(files, bw, bh, mode, filter_down, expand_filter, filter_up, factors, criterion, targets,
                                                     group_first=group_first, filter_byte=filter_byte, out=out,
                                                     _entry="pxz_retile_varied_files_fit_tiles")

    def rate_distortion_varied_files(self, files, bw, bh, mode, filter_down, expand_filter, filter_up, factors,
                                     _entry="pxz_rate_distortion_varied_files"):
        """pxz_rate_distortion_varied_files: a list of .pixlzr files (bytes) of one channel count and of block size bw x bh at
        every factor of `factors` (1..32) -> (file_bytes uint64[K,n], sse uint64[K,n,C]): the length of each re-shrunk file
        and its squared error against what the file decodes to now.  (_entry: the entry point that is called -- the forms that
        take another block size share this marshalling.)"""
        n = len(files)
        bufs = [np.frombuffer(bytes(f), np.uint8) for f in files]
        ptrs = (C.c_void_p * max(n, 1))(*[b.ctypes.data if b.size else None for b in bufs])
        lens = (C.c_size_t * max(n, 1))(*[b.size for b in bufs])
        ch = file_header(files[0])[4] if n and len(files[0]) >= 26 else 4
        fac = np.ascontiguousarray(factors, np.float32)
        K = fac.size
        pd = Params(bw, bh, mode, filter_down, 0.0, 0)
        file_bytes = np.zeros((max(K, 1), max(n, 1)), np.uint64)
        sse = np.zeros((max(K, 1), max(n, 1), ch), np.uint64)
        self._check(getattr(self._L, _entry)(
            self._h, C.cast(ptrs, C.c_void_p), C.cast(lens, C.c_void_p), n, C.byref(pd), expand_filter, filter_up,
            _p(fac) if K else None, K, _p(file_bytes), _p(sse)))
        return file_bytes[:K, :n], sse[:K, :n]

    def transcode_varied_files_fit(self, files, bw, bh, mode, filter_down, expand_filter, filter_up, factors, criterion, targets,
                                   filter_byte=0, want_table=False, out=None, _entry="pxz_transcode_varied_files_fit"):
        """pxz_transcode_varied_files_fit: a list of .pixlzr files (bytes) -> the list of the files re-shrunk, each at the
        factor of `factors` that fit_select picks under targets[i], the error measured against what the file decodes to now.
        Returns (files, choice uint32[n], fit_flags uint32[n]) and, with want_table, (file_bytes uint64[K,n], sse
        uint64[K,n,C]).  out: a numpy uint8 buffer to write into (PxzError -7 with .needed, .choice, .fit_flags and .table when
        it is too small; size 0 is the size query), else the buffer is sized by a first call."""
        n = len(files)
        bufs = [np.frombuffer(bytes(f), np.uint8) for f in files]
        ptrs = (C.c_void_p * max(n, 1))(*[b.ctypes.data if b.size else None for b in bufs])
        lens = (C.c_size_t * max(n, 1))(*[b.size for b in bufs])
        ch = file_header(files[0])[4] if n and len(files[0]) >= 26 else 4
        fac = np.ascontiguousarray(factors, np.float32)
        K = fac.size
        tg = np.array([int(t) for t in targets], np.uint64)
        pd = Params(bw, bh, mode, filter_down, 0.0, 0)
        offs = np.zeros(n + 1, np.uint64)
        choice, flags = np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.uint32)
        table_bytes = np.zeros((max(K, 1), max(n, 1)), np.uint64)
        table_sse = np.zeros((max(K, 1), max(n, 1), ch), np.uint64)

        def call(buf):
            return getattr(self._L, _entry)(
                self._h, C.cast(ptrs, C.c_void_p), C.cast(lens, C.c_void_p), n, C.byref(pd), expand_filter, filter_up,
                _p(fac) if K else None, K, criterion, _p(tg) if tg.size else None, filter_byte,
                _p(buf) if buf is not None and buf.size else None, 0 if buf is None else buf.size, _p(offs), _p(choice), _p(flags),
                _p(table_bytes), _p(table_sse))
        if out is None:
            out = np.empty(sum(b.size for b in bufs) + 4096 * max(n, 1), np.uint8)
            rc = call(out)
            if rc == -7:
                out = np.empty(int(offs[-1]), np.uint8)
                rc = call(out)
        else:
            rc = call(out)
        if rc != 0:
            err = PxzError(rc, (self._L.pxz_last_error(self._h) or b"").decode())
            err.needed, err.choice, err.fit_flags = int(offs[-1]), choice[:n].copy(), flags[:n].copy()
            err.table = (table_bytes[:K, :n].copy(), table_sse[:K, :n].copy())
            raise err
        res = [out[int(offs[i]):int(offs[i + 1])].tobytes() for i in range(n)]
        if want_table:
            return res, choice[:n], flags[:n], table_bytes[:K, :n], table_sse[:K, :n]
        return res, choice[:n], flags[:n]

    # ---- fit to a budget per tile ----
    def record_bytes_varied_device(self, sizes, channels, bw, bh, vals, ow, oh, slots, want_offsets=True, out=None):
        """pxz_record_bytes_varied_device: sizes = [(width, height), ...] of the images whose tiles (varied layout; for a ladder's
        result the sizes repeated K times and the tensors flattened) are given -> (record_bytes int32[T], file_offsets
        int64[n+1] | None): the bytes of every tile's record in its file, and what encode_varied_frames_device gives for its
        offsets.  out: such a pair (the offsets may be None); None for a tensor passes a null pointer."""
        import torch
        geoms = [tuple(s) if len(s) > 2 else (s[0], s[1], s[0] * channels, 0) for s in sizes]
        n = len(geoms)
        if out is None:
            T = int(varied_layout(geoms, bw, bh)[-1])
            out = (torch.empty(T, dtype=torch.int32, device=vals.device),
                   torch.empty(n + 1, dtype=torch.int64, device=vals.device) if want_offsets else None)
        rec, offs = out
        pd = Params(bw, bh, 0, 0, 1.0, 0)
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
        self.use_torch_stream()
        self._check(self._L.pxz_record_bytes_varied_device(
            self._h, C.cast(image_descs(geoms), C.c_void_p) if n else None, n, channels, C.byref(pd), ptr(vals), ptr(ow), ptr(oh), ptr(slots),
            ptr(rec), ptr(offs)))
        return rec, offs

    def fit_varied_tiles_device(self, sizes, channels, bw, bh, record_bytes, tile_sse, criterion, targets, group_first=None, n_groups=None,
                                n_factors=None, out=None):
        """pxz_fit_varied_tiles_device: fit_tiles_select on the device.  sizes = [(width, height), ...] of the images,
        record_bytes int32[K, T] (record_bytes_varied_device over the images repeated K times) and tile_sse int64[K, T, C] (the
        distortion calls' per-tile sums over the same) are CUDA tensors; group_first (G + 1 host image indices, None: every
        image its own group) and targets (G host integers) -> (tile_choice int32[T], lambda int64[G], bytes int64[G], sse
        int64[G], flags int32[G]) CUDA tensors, or out = such a 5-tuple.  n_groups and n_factors override what the arguments
        say; None for targets or a tensor passes a null pointer."""
        import torch
        geoms = [tuple(s) if len(s) > 2 else (s[0], s[1], s[0] * channels, 0) for s in sizes]
        n = len(geoms)
        gf = None if group_first is None else np.array([int(x) for x in group_first], np.uint32)
        G = n_groups if n_groups is not None else (n if gf is None else len(gf) - 1)
        K = n_factors if n_factors is not None else record_bytes.shape[0]
        tg = None if targets is None else np.array([int(t) for t in targets], np.uint64)
        if out is None:
            T = int(varied_layout(geoms, bw, bh)[-1])
            dev = torch.device("cuda", self.device_id)
            out = (torch.empty(T, dtype=torch.int32, device=dev),) + tuple(torch.empty(G, dtype=torch.int64, device=dev) for _ in range(3)) + (
                torch.empty(G, dtype=torch.int32, device=dev),)
        pd = Params(bw, bh, 0, 0, 0.0, 0)
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
        self.use_torch_stream()
        self._check(self._L.pxz_fit_varied_tiles_device(
            self._h, C.cast(image_descs(geoms), C.c_void_p) if n else None, n, channels, C.byref(pd), _p(gf), G, K, criterion, _p(tg),
            ptr(record_bytes), ptr(tile_sse), *[ptr(t) for t in out]))
        return out

    def gather_varied_tile_rungs_device(self, sizes, channels, bw, bh, n_factors, tile_choice, vals, ow, oh, slots, out=None,
                                        image_flags=None, want_pixels=True):
        """pxz_gather_varied_tile_rungs_device: gather_varied_rungs_device with a choice per tile -- tile_choice int32[T] CUDA in
        flat tile order; output tile t comes from rung tile_choice[t].  image_flags (int32[n] CUDA, optional) gets 2 for an
        image that holds a tile whose choice was n_factors or more, else 0."""
        import torch
        geoms = [tuple(s) if len(s) > 2 else (s[0], s[1], s[0] * channels, 0) for s in sizes]
        if out is None:
            T = int(varied_layout(geoms, bw, bh)[-1])
            dev = vals.device
            out = (torch.empty(T, dtype=torch.float32, device=dev), torch.empty(T, dtype=torch.int32, device=dev),
                   torch.empty(T, dtype=torch.int32, device=dev),
                   torch.empty((T, bw * bh * channels), dtype=torch.uint8, device=dev) if want_pixels else None)
        o_vals, o_w, o_h, o_slots = out
        pd = Params(bw, bh, 0, 0, 0.0, 0)
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
        self.use_torch_stream()
        self._check(self._L.pxz_gather_varied_tile_rungs_device(
            self._h, C.cast(image_descs(geoms), C.c_void_p), len(geoms), channels, C.byref(pd), n_factors, ptr(tile_choice), ptr(vals),
            ptr(ow), ptr(oh), ptr(slots), ptr(o_vals), ptr(o_w), ptr(o_h), ptr(o_slots), ptr(image_flags)))
        return o_vals, o_w, o_h, o_slots

    def _fit_tiles_outputs(self, n, G, T):
        return (np.zeros(n + 1, np.uint64), np.zeros(max(T, 1), np.uint32), np.zeros(max(G, 1), np.uint64), np.zeros(max(G, 1), np.uint64),
                np.zeros(max(G, 1), np.uint64), np.zeros(max(G, 1), np.uint32))

    def _fit_tiles_result(self, call, first_size, n, G, T, res, out):
        """the two-call protocol of the tile-fit forms: out None -> a first guess, then the exact size"""
        offs, choice, lam, gb, gs, fl = res
        if out is None:
            out = np.empty(first_size, np.uint8)
            rc = call(out)
            if rc == -7:
                out = np.empty(int(offs[-1]), np.uint8)
                rc = call(out)
        else:
            rc = call(out)
        if rc != 0:
            err = PxzError(rc, (self._L.pxz_last_error(self._h) or b"").decode())
            err.needed, err.tile_choice, err.groups = int(offs[-1]), choice[:T].copy(), (lam[:G].copy(), gb[:G].copy(), gs[:G].copy(), fl[:G].copy())
            raise err
        files = [out[int(offs[i]):int(offs[i + 1])].tobytes() for i in range(n)]
        return files, choice[:T], lam[:G], gb[:G], gs[:G], fl[:G]

    def encode_varied_images_fit_tiles(self, imgs, bw, bh, mode, filter_down, filter_up, factors, criterion, targets, group_first=None,
                                       filter_byte=0, out=None):
        """pxz_encode_varied_images_fit_tiles: host images (numpy uint8 [H, W, C], one channel count) -> one .pixlzr file per
        image whose tiles come from the rungs of `factors` (1..32) that fit_tiles_select picks under targets[g] for the groups
        of group_first (G + 1 image indices; None: every image its own group).  Returns (files: a list of bytes, tile_choice
        uint32[T] in flat tile order, lambda uint64[G], bytes uint64[G], sse uint64[G], flags uint32[G]).  out: a numpy uint8
        buffer to write into (PxzError -7 with .needed, .tile_choice and .groups when it is too small; size 0 is the size
        query), else the buffer is sized by a first call."""
        imgs = [np.ascontiguousarray(i) if i.strides[1] != i.shape[2] or i.strides[2] != 1 else i for i in imgs]
        n = len(imgs)
        ch = imgs[0].shape[2] if n else 4
        geoms = [(i.shape[1], i.shape[0], i.strides[0], 0) for i in imgs]
        ptrs = (C.c_void_p * max(n, 1))(*[i.ctypes.data for i in imgs])
        descs = image_descs(geoms)
        fac = np.ascontiguousarray(factors, np.float32)
        K = fac.size
        gf = None if group_first is None else np.array([int(x) for x in group_first], np.uint32)
        G = n if gf is None else len(gf) - 1
        tg = np.array([int(t) for t in targets], np.uint64)
        T = int(varied_layout(geoms, bw, bh)[-1]) if n else 0
        res = self._fit_tiles_outputs(n, G, T)

        def call(buf):
            return self._L.pxz_encode_varied_images_fit_tiles(
                self._h, C.cast(ptrs, C.c_void_p), C.cast(descs, C.c_void_p), n, ch, bw, bh, mode, filter_down, filter_up,
                _p(fac) if K else None, K, criterion, _p(gf), G, _p(tg) if tg.size else None, filter_byte,
                _p(buf) if buf is not None and buf.size else None, 0 if buf is None else buf.size, *[_p(a) for a in res])
        return self._fit_tiles_result(call, sum(i.size for i in imgs) * 5 // 4 + 4096 * max(n, 1), n, G, T, res, out)

    def transcode_varied_files_fit_tiles(self, files, bw, bh, mode, filter_down, expand_filter, filter_up, factors, criterion, targets,
                                         group_first=None, filter_byte=0, out=None, _entry="pxz_transcode_varied_files_fit_tiles"):
        """pxz_transcode_varied_files_fit_tiles: the same for a list of .pixlzr files (bytes) of one channel count and of block
        size bw x bh, the error measured against what each file decodes to now (expand_filter).  Returns and out as
        encode_varied_images_fit_tiles."""
        n = len(files)
        bufs = [np.frombuffer(bytes(f), np.uint8) for f in files]
        ptrs = (C.c_void_p * max(n, 1))(*[b.ctypes.data if b.size else None for b in bufs])
        lens = (C.c_size_t * max(n, 1))(*[b.size for b in bufs])
        fac = np.ascontiguousarray(factors, np.float32)
        K = fac.size
        gf = None if group_first is None else np.array([int(x) for x in group_first], np.uint32)
        G = n if gf is None else len(gf) - 1
        tg = np.array([int(t) for t in targets], np.uint64)
        pd = Params(bw, bh, mode, filter_down, 0.0, 0)
        try:
            geoms = [file_header(f)[:2] for f in files]
            T = int(varied_layout([(w, h, 0, 0) for (w, h) in geoms], bw, bh)[-1])
        except PxzError:  # (a malformed file: the call itself says which)
            T = 0
        res = self._fit_tiles_outputs(n, G, T)

        def call(buf):
            return getattr(self._L, _entry)(
                self._h, C.cast(ptrs, C.c_void_p), C.cast(lens, C.c_void_p), n, C.byref(pd), expand_filter, filter_up,
                _p(fac) if K else None, K, criterion, _p(gf), G, _p(tg) if tg.size else None, filter_byte,
                _p(buf) if buf is not None and buf.size else None, 0 if buf is None else buf.size, res[0].ctypes.data,
                _p(res[1]) if T else None, *[_p(a) for a in res[2:]])
        return self._fit_tiles_result(call, sum(b.size for b in bufs) + 4096 * max(n, 1), n, G, T, res, out)

    # ---- decode side: Pixlzr::expand + to_image ----
    def expand_image(self, width, height, channels, bw, bh, filt, tile_w, tile_h, slots):
        """Host buffers: stored tiles (slots[t] holds tile_w[t]*tile_h[t]*channels tightly packed bytes in a slot of
        bw*bh*channels) -> (height, width, channels) image."""
        tile_w = np.ascontiguousarray(tile_w, np.uint32)
        tile_h = np.ascontiguousarray(tile_h, np.uint32)
        slots = np.ascontiguousarray(slots, np.uint8)
        assert slots.shape[1] == bw * bh * channels
        out = np.zeros((height, width, channels), np.uint8)
        self._check(self._L.pxz_expand_image(self._h, width, height, channels, width * channels, bw, bh, filt,
                                             _p(tile_w), _p(tile_h), _p(slots), _p(out)))
        return out

    def expand_frames_device(self, shape, bw, bh, filt, ow, oh, slots, out=None):
        """Device tensors as left by shrink_frames_device (w[N,T], h[N,T], slots[N,T,bw*bh*C]) -> frames [N,H,W,C]."""
        import torch
        N, H, W, Cc = shape
        if out is None:
            out = torch.empty((N, H, W, Cc), dtype=torch.uint8, device=slots.device)
        fd, _ = self._frames_desc(out)
        pd = Params(bw, bh, 0, filt, 0.0, 0)
        self.use_torch_stream()
        self._check(self._L.pxz_expand_frames_device(self._h, C.byref(fd), C.byref(pd), C.c_void_p(ow.data_ptr()),
                                                     C.c_void_p(oh.data_ptr()), C.c_void_p(slots.data_ptr()),
                                                     C.c_void_p(out.data_ptr())))
        return out

    @staticmethod
    def _rgba_out(frames, out):
        """-> (out, row pitch, frame stride in bytes): a packed tensor of its own, or the caller's [N,H,W,4] view as it lies"""
        import torch
        N, H, W, _ = frames.shape
        if out is None:
            return torch.empty((N, H, W, 4), dtype=torch.uint8, device=frames.device), W * 4, W * 4 * H
        assert out.is_cuda and out.dtype == torch.uint8 and out.device == frames.device and tuple(out.shape) == (N, H, W, 4)
        assert out.stride(3) == 1 and out.stride(2) == 4 and out.stride(1) >= W * 4
        assert N == 1 or out.stride(0) >= out.stride(1) * (H - 1) + W * 4
        return out, out.stride(1), out.stride(0)

    def process_frames_device(self, frames, bw, bh, filter_down=4, filter_up=0, out=None):
        """process_custom with |x - avg| / identity (process/mod.rs:71-121): frames [N,H,W,C] -> RGBA [N,H,W,4].
        out: a [N,H,W,4] uint8 view to write into (any row pitch and frame stride; bytes between the rows are left alone)."""
        fd, (N, H, W, Cc) = self._frames_desc(frames)
        out, pitch, stride = self._rgba_out(frames, out)
        pd = Params(bw, bh, 0, filter_down, 1.0, 0)
        self.use_torch_stream()
        self._check(self._L.pxz_process_frames_device(self._h, C.byref(fd), C.byref(pd), filter_up,
                                                      C.c_void_p(frames.data_ptr()), C.c_void_p(out.data_ptr()),
                                                      pitch, stride))
        return out

    def tree_process_frames_device(self, frames, bw, bh, threshold, min_bw=4, min_bh=4, filter_down=4, filter_up=0, out=None):
        """tree::process_custom with |x - avg| / identity (process/tree.rs:23-109): frames [N,H,W,C] -> RGBA [N,H,W,4].
        out: as in process_frames_device."""
        fd, (N, H, W, Cc) = self._frames_desc(frames)
        out, pitch, stride = self._rgba_out(frames, out)
        pd = Params(bw, bh, 0, filter_down, 1.0, 0)
        self.use_torch_stream()
        self._check(self._L.pxz_tree_process_frames_device(self._h, C.byref(fd), C.byref(pd), filter_up, C.c_float(threshold),
                                                           min_bw, min_bh, C.c_void_p(frames.data_ptr()),
                                                           C.c_void_p(out.data_ptr()), pitch, stride))
        return out

    def decode_status(self):
        """bit 0: invalid stored tile size seen by expand; bit 1: malformed file/record seen by decode."""
        flags = C.c_uint32(0)
        self._check(self._L.pxz_decode_status(self._h, C.byref(flags)))
        return flags.value

    def decode_frames_device(self, files, file_offsets, shape, bw, bh, out=None):
        """files: uint8 CUDA tensor holding N .pixlzr files back to back, file_offsets int64[N+1] (CUDA).
        Returns (values[N,T], w[N,T], h[N,T], slots[N,T,bw*bh*C]) for frames of `shape` = (N,H,W,C)."""
        import torch
        N, H, W, Cc = shape
        cols, rows = grid(W, H, bw, bh)
        T = cols * rows
        dev = files.device
        if out is None:
            vals = torch.zeros((N, T), dtype=torch.float32, device=dev)
            ow = torch.zeros((N, T), dtype=torch.int32, device=dev)
            oh = torch.zeros((N, T), dtype=torch.int32, device=dev)
            slots = torch.zeros((N, T, bw * bh * Cc), dtype=torch.uint8, device=dev)
        else:
            vals, ow, oh, slots = out
        fd = Frames(W, H, Cc, W * Cc, N, 0, W * Cc * H)
        pd = Params(bw, bh, 0, 0, 0.0, 0)
        self.use_torch_stream()
        self._check(self._L.pxz_decode_frames_device(self._h, C.byref(fd), C.byref(pd), C.c_void_p(files.data_ptr()),
                                                     C.c_void_p(file_offsets.data_ptr()), C.c_void_p(vals.data_ptr()),
                                                     C.c_void_p(ow.data_ptr()), C.c_void_p(oh.data_ptr()),
                                                     C.c_void_p(slots.data_ptr())))
        return vals, ow, oh, slots

    def lod_frames_device(self, frames, bw, bh, mode, factor=1.0):
        import torch
        fd, (N, H, W, Cc) = self._frames_desc(frames)
        cols, rows = grid(W, H, bw, bh)
        T = cols * rows
        l0 = torch.empty((N, T), dtype=torch.float32, device=frames.device)
        l1 = torch.empty((N, T), dtype=torch.float32, device=frames.device)
        pd = Params(bw, bh, mode, FILTER_NEAREST, factor, 0)
        self.use_torch_stream()
        self._check(self._L.pxz_lod_frames_device(self._h, C.byref(fd), C.byref(pd), C.c_void_p(frames.data_ptr()),
                                                  C.c_void_p(l0.data_ptr()), C.c_void_p(l1.data_ptr())))
        return l0, l1

    def pack_tiles_device(self, ow, oh, slots, channels, out=None):
        """Compacts the valid bytes of the slots (any leading batch dims) into one stream.
        Returns (offsets int64[n_tiles+1], packed uint8[capacity]); offsets[-1] is the stream length."""
        import torch
        n = ow.numel()
        slot_bytes = slots.shape[-1]
        if out is None:
            offsets = torch.empty(n + 1, dtype=torch.int64, device=ow.device)
            packed = torch.empty(n * slot_bytes, dtype=torch.uint8, device=ow.device)
        else:
            offsets, packed = out
        self.use_torch_stream()
        self._check(self._L.pxz_pack_tiles_device(
            self._h, n, channels, slot_bytes, C.c_void_p(ow.data_ptr()), C.c_void_p(oh.data_ptr()),
            C.c_void_p(slots.data_ptr()), C.c_void_p(offsets.data_ptr()), C.c_void_p(packed.data_ptr()),
            packed.numel()))
        return offsets, packed

    def encode_frames_device(self, shape, bw, bh, vals, ow, oh, slots, filter_byte=0, out=None):
        """GPU bitstream: tiles of a batch -> the .pixlzr files, back to back.  shape = (N, H, W, C) of the frames.
        Returns (file_offsets int64[N+1], bytes uint8[capacity])."""
        import torch
        N, H, W, Cc = shape
        fd = Frames(W, H, Cc, W * Cc, N, 0, W * Cc * H)
        pd = Params(bw, bh, 0, 0, 1.0, 0)
        if out is None:
            cols, rows = grid(W, H, bw, bh)
            cap = N * (26 + rows * 4) + N * cols * rows * (13 + 10 + bw * bh * (Cc + 1) + 8)
            offs = torch.empty(N + 1, dtype=torch.int64, device=vals.device)
            buf = torch.empty(cap, dtype=torch.uint8, device=vals.device)
        else:
            offs, buf = out
        self.use_torch_stream()
        self._check(self._L.pxz_encode_frames_device(
            self._h, C.byref(fd), C.byref(pd), filter_byte, C.c_void_p(vals.data_ptr()), C.c_void_p(ow.data_ptr()),
            C.c_void_p(oh.data_ptr()), C.c_void_p(slots.data_ptr()), C.c_void_p(buf.data_ptr()), buf.numel(),
            C.c_void_p(offs.data_ptr())))
        return offs, buf

    def synth_frames_device(self, n_frames, height, width, channels=4, first_frame=0, dist=DIST_OPAQUE, out=None):
        import torch
        if out is None:
            out = torch.empty((n_frames, height, width, channels), dtype=torch.uint8,
                              device=torch.device("cuda", self.device_id))
        fd, _ = self._frames_desc(out)
        self.use_torch_stream()
        self._check(self._L.pxz_synth_frames_device(self._h, C.byref(fd), C.c_void_p(out.data_ptr()), first_frame, dist))
        return out
