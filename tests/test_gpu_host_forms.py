"""The steps the host forms share (the header scan, the reader's flags, the writer's room, the rung table) give one answer
whichever form takes them: files that disagree and a truncated file are refused with one code and one text by every form that
reads files, the four writers report the room they need in one way and write the same bytes into exactly that room, and the
fit forms' tables equal the rate-distortion calls'.  The expected texts are taken from the first form and compared with the
others, never written down here: this file asserts that there is one answer, the other suites that it is the right one.
Every output buffer is poisoned before each call."""
import ctypes as C
import re

import numpy as np
import pytest

from test_gpu_varied import make_image

pytestmark = pytest.mark.gpu

INVALID_ARG, BUFFER_TOO_SMALL = -1, -7
POISON = 0xA5
BW = BH = 16
MODE, FILT, EXPAND, UP = 0, 4, 1, 1  # shrink_by (no tile is too small for it), Lanczos3 down, triangle up
FACTORS = [1.0, 0.5]
FIT_BYTES = 0
SIZES = [(40, 24), (17, 33), (33, 17)]  # width x height: no multiple of the block, a one-pixel edge column and edge row


@pytest.fixture(scope="module")
def gpu(product):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    h = product.Handle(0)
    yield h
    h.close()


@pytest.fixture(scope="module")
def images():
    rng = np.random.default_rng(20261019)
    return {c: [make_image(rng, w, h, c, alpha=False) for (w, h) in SIZES] for c in (3, 4)}


@pytest.fixture(scope="module")
def archives(gpu, images):
    """channels -> the images' .pixlzr files in 16x16 blocks; "8x8": the RGBA images in 8x8 blocks"""
    files = {c: gpu.encode_varied_images(images[c], BW, BH, MODE, FILT, 1.0) for c in (3, 4)}
    files["8x8"] = gpu.encode_varied_images(images[4], 8, 8, MODE, FILT, 1.0)
    return files


def last_error(gpu):
    return (gpu._L.pxz_last_error(gpu._h) or b"").decode()


def _ptr(a):
    return None if a is None else a.ctypes.data


class Call:
    """One host form with poisoned outputs: run(out_bytes) -> (code, text), the outputs kept on the object.  out_bytes None
    passes a null `out` and capacity 0."""

    def __init__(self, gpu, product, name, srcs, n_files):
        self.gpu, self.product, self.name, self.n = gpu, product, name, len(srcs)
        self.offs = np.full(n_files + 1, 0x5A5A5A5A5A5A5A5A, np.uint64)
        self.choice, self.flags = np.zeros(self.n, np.uint32), np.zeros(self.n, np.uint32)
        self.pd = product.binding.Params(BW, BH, MODE, FILT, 1.0, 0)
        self.fac = np.ascontiguousarray(FACTORS, np.float32)
        self.targets = np.full(self.n, 1 << 40, np.uint64)  # every rung fits: rung 0 is chosen
        self.keep = srcs  # (the arrays behind the pointers)
        self.ptrs = (C.c_void_p * self.n)(*[s.ctypes.data for s in srcs])
        self.out = None

    def from_files(self):
        self.lens = (C.c_size_t * self.n)(*[s.size for s in self.keep])
        return self

    def from_images(self):
        self.ch = self.keep[0].shape[2]
        self.descs = self.product.binding.image_descs([(i.shape[1], i.shape[0], i.strides[0], 0) for i in self.keep])
        return self

    def run(self, out_bytes):
        L, h, K = self.gpu._L, self.gpu._h, self.fac.size
        self.out = None if out_bytes is None else np.full(out_bytes + 64, POISON, np.uint8)  # (64: a guard behind the room)
        self.offs[:] = 0x5A5A5A5A5A5A5A5A
        out, cap, offs = _ptr(self.out), out_bytes or 0, _ptr(self.offs)
        ptrs = C.cast(self.ptrs, C.c_void_p)
        if self.name == "transcode_varied_files":
            rc = L.pxz_transcode_varied_files(h, ptrs, C.cast(self.lens, C.c_void_p), self.n, C.byref(self.pd), EXPAND, 0, out, cap, offs)
        elif self.name == "transcode_varied_ladder_files":
            rc = L.pxz_transcode_varied_ladder_files(h, ptrs, C.cast(self.lens, C.c_void_p), self.n, C.byref(self.pd), EXPAND, _ptr(self.fac), K,
                                                     0, out, cap, offs)
        elif self.name == "transcode_varied_files_fit":
            rc = L.pxz_transcode_varied_files_fit(h, ptrs, C.cast(self.lens, C.c_void_p), self.n, C.byref(self.pd), EXPAND, UP, _ptr(self.fac), K,
                                                  FIT_BYTES, _ptr(self.targets), 0, out, cap, offs, _ptr(self.choice), _ptr(self.flags), None,
                                                  None)
        elif self.name == "encode_varied_images":
            rc = L.pxz_encode_varied_images(h, ptrs, C.cast(self.descs, C.c_void_p), self.n, self.ch, C.byref(self.pd), 0, out, cap, offs)
        elif self.name == "encode_varied_images_fit":
            rc = L.pxz_encode_varied_images_fit(h, ptrs, C.cast(self.descs, C.c_void_p), self.n, self.ch, BW, BH, MODE, FILT, UP, _ptr(self.fac),
                                                K, FIT_BYTES, _ptr(self.targets), 0, out, cap, offs, _ptr(self.choice), _ptr(self.flags), None,
                                                None)
        else:
            raise AssertionError(self.name)
        return rc, last_error(self.gpu) if rc else ""

    def out_untouched(self):
        return self.out is None or bool((self.out == POISON).all())


def rate_distortion_files(gpu, product, bufs):
    """pxz_rate_distortion_varied_files with poisoned tables (its `out`) -> (code, text, tables untouched)"""
    n, K = len(bufs), len(FACTORS)
    ptrs = (C.c_void_p * n)(*[b.ctypes.data for b in bufs])
    lens = (C.c_size_t * n)(*[b.size for b in bufs])
    pd = product.binding.Params(BW, BH, MODE, FILT, 0.0, 0)
    fac = np.ascontiguousarray(FACTORS, np.float32)
    file_bytes, sse = np.full((K, n), POISON, np.uint64), np.full((K, n, 4), POISON, np.uint64)
    rc = gpu._L.pxz_rate_distortion_varied_files(gpu._h, C.cast(ptrs, C.c_void_p), C.cast(lens, C.c_void_p), n, C.byref(pd), EXPAND, UP, _ptr(fac), K,
                                                 _ptr(file_bytes), _ptr(sse))
    return rc, last_error(gpu) if rc else "", bool((file_bytes == POISON).all() and (sse == POISON).all())


def refusals(gpu, product, files):
    """the four forms that read files, on `files` -> [(name, code, text, out untouched)]"""
    bufs = [np.frombuffer(bytes(f), np.uint8) for f in files]
    got = []
    for name, n_files in (("transcode_varied_files", len(files)), ("transcode_varied_ladder_files", len(FACTORS) * len(files)),
                          ("transcode_varied_files_fit", len(files))):
        call = Call(gpu, product, name, bufs, n_files).from_files()
        rc, text = call.run(1 << 16)
        got.append((name, rc, text, call.out_untouched()))
        if name == "transcode_varied_ladder_files":
            got.append(("rate_distortion_varied_files",) + rate_distortion_files(gpu, product, bufs))
    return got


def assert_one_refusal(got, code, index):
    for name, rc, text, untouched in got:
        print(name, rc, repr(text))
    _, rc0, text0, _ = got[0]
    assert rc0 == code and text0.startswith("image %u:" % index), got[0]
    for name, rc, text, untouched in got:
        assert (rc, text) == (rc0, text0), (name, "answers otherwise than", got[0][0])
        assert untouched, (name, "wrote to out")


# ---- 1. files that disagree -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("odd", ["8x8", 3])
def test_files_that_disagree_are_refused_alike(gpu, product, archives, odd):
    files = list(archives[4])
    files[1] = archives[odd][1]
    assert_one_refusal(refusals(gpu, product, files), INVALID_ARG, 1)


# ---- 2. a truncated file --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("channels", [3, 4])
def test_a_truncated_file_is_refused_alike(gpu, product, archives, channels):
    files = list(archives[channels])
    files[-1] = files[-1][:-5]
    got = refusals(gpu, product, files)
    assert_one_refusal(got, INVALID_ARG, len(files) - 1)
    assert got[0][2].endswith("nothing was written")


# ---- 3. room ----------------------------------------------------------------------------------------------------------------

def writers(gpu, product, images, files):
    bufs = [np.frombuffer(bytes(f), np.uint8) for f in files]
    n = len(images)
    return [Call(gpu, product, "encode_varied_images", images, n).from_images(),
            Call(gpu, product, "transcode_varied_files", bufs, n).from_files(),
            Call(gpu, product, "encode_varied_images_fit", images, n).from_images(),
            Call(gpu, product, "transcode_varied_files_fit", bufs, n).from_files()]


@pytest.mark.parametrize("channels", [3, 4])
def test_the_writers_report_and_use_their_room_alike(gpu, product, images, archives, channels):
    shape = None
    for call in writers(gpu, product, images[channels], archives[channels]):
        rc, text = call.run(1 << 16)  # ample room
        assert rc == 0, (call.name, text)
        offs = call.offs.copy()
        total = int(offs[-1])
        assert offs[0] == 0 and (np.diff(offs.astype(np.int64)) > 0).all() and total < (1 << 16), (call.name, offs)
        ample = call.out[:total].copy()
        assert (call.out[total:] == POISON).all(), (call.name, "wrote behind the files")
        for room in (None, total - 1):
            rc, text = call.run(room)
            print(call.name, room, rc, repr(text))
            assert rc == BUFFER_TOO_SMALL, (call.name, room, rc)
            assert [int(v) for v in re.findall(r"\d+", text)] == [total, room or 0], (call.name, text)
            shape = shape or re.sub(r"\d+", "#", text)
            assert re.sub(r"\d+", "#", text) == shape, (call.name, "words it otherwise than the first writer")
            assert (call.offs == offs).all(), (call.name, room, "file_offsets is not filled")
            assert call.out_untouched(), (call.name, room, "wrote to out")
        rc, text = call.run(total)  # exactly the room
        assert rc == 0, (call.name, text)
        assert (call.offs == offs).all() and (call.out[:total] == ample).all(), (call.name, "other files in exactly their room")
        assert (call.out[total:] == POISON).all(), (call.name, "wrote behind its room")


# ---- 4. the rung table ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("channels", [3, 4])
def test_the_fit_forms_tables_are_the_rate_distortion_calls(gpu, images, archives, channels):
    n = len(SIZES)
    targets = [1 << 40] * n
    fb, sse = gpu.rate_distortion_varied_images(images[channels], BW, BH, MODE, FILT, UP, FACTORS)
    _, _, _, t_fb, t_sse = gpu.encode_varied_images_fit(images[channels], BW, BH, MODE, FILT, UP, FACTORS, FIT_BYTES, targets, want_table=True)
    assert fb.shape == (len(FACTORS), n) and (fb > 0).all()
    assert (t_fb == fb).all() and (t_sse == sse).all(), "images: the fit form's table is not rate_distortion_varied_images'"
    fb, sse = gpu.rate_distortion_varied_files(archives[channels], BW, BH, MODE, FILT, EXPAND, UP, FACTORS)
    _, _, _, t_fb, t_sse = gpu.transcode_varied_files_fit(archives[channels], BW, BH, MODE, FILT, EXPAND, UP, FACTORS, FIT_BYTES, targets,
                                                          want_table=True)
    assert fb.shape == (len(FACTORS), n) and (fb > 0).all()
    assert (t_fb == fb).all() and (t_sse == sse).all(), "files: the fit form's table is not rate_distortion_varied_files'"
