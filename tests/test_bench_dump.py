"""bench.py --dump-outputs on CPU tensors: what it writes is the shrink's output (oracle), in float, with the unspecified
rest of every slot left out, the same whatever that rest holds."""
import os

import numpy as np
import torch

import bench


def _outputs(oracle, frames, junk):
    res = [oracle.shrink_image(oracle.synth_frame(200, 130, 4, f, oracle.DIST_ALPHA), 32, 32, 1, 4, 16.0) for f in frames]
    vals, w, h, slots = (np.stack([r[i] for r in res]) for i in range(4))
    nbytes = w.astype(np.int64) * h * 4
    slots = np.where(np.arange(slots.shape[-1]) < nbytes[..., None], slots, junk).astype(np.uint8)
    return (torch.from_numpy(vals), torch.from_numpy(w.astype(np.int32)), torch.from_numpy(h.astype(np.int32)),
            torch.from_numpy(slots)), nbytes


def test_dump_outputs_match_the_oracle(oracle, tmp_path):
    out, nbytes = _outputs(oracle, (0, 1), junk=0xA5)
    bench.dump_outputs(str(tmp_path / "a"), out, 4)
    bench.dump_outputs(str(tmp_path / "b"), _outputs(oracle, (0, 1), junk=0x3C)[0], 4)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["height.npy", "pixel_sum.npy", "pixels.npy", "pixels_tile.npy", "values.npy", "width.npy"]
    got = {n[:-4]: np.load(tmp_path / "a" / n) for n in names}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    for n in names:
        assert np.array_equal(got[n[:-4]], np.load(tmp_path / "b" / n)), n
    vals, w, h, slots = (t.numpy() for t in out)
    assert np.array_equal(got["values"].view(np.uint32), vals.view(np.uint32))
    assert np.array_equal(got["width"], w) and np.array_equal(got["height"], h)
    valid = np.where(np.arange(slots.shape[-1]) < nbytes[..., None], slots, 0)
    assert np.array_equal(got["pixel_sum"], valid.sum(-1, dtype=np.int64))
    idx = got["pixels_tile"].astype(np.int64)
    assert len(idx) == w.size and np.array_equal(got["pixels"], valid.reshape(w.size, -1)[idx])
