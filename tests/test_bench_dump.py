"""CPU: bench.py --dump-outputs writes what the timed fit() left for its caller -- float32 / float64 arrays, at most
64 MB, a seeded scene sample that is the same from run to run -- checked on a stand-in batch of host tensors."""
import os
import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")


def _batch(S, K=4, B=5, H=64, W=64, it=9):
    g = torch.Generator().manual_seed(S)
    return types.SimpleNamespace(
        S=S, device=torch.device("cpu"),
        sed_current=torch.rand(S, K, B, generator=g), morph_current=torch.rand(S, K, H, W, generator=g),
        centers=torch.randint(0, H, (S, K, 2), generator=g, dtype=torch.int32),
        shifts=torch.rand(S, K, 2, generator=g, dtype=torch.float64),
        mse_buf=torch.rand(S, it + 3, generator=g, dtype=torch.float64),
        it=torch.full((S,), it, dtype=torch.int32), flags=torch.zeros(S, K, dtype=torch.int32))


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_small_batch_is_complete(tmp_path):
    import bench
    b = _batch(6)
    info = bench.dump_outputs(b, str(tmp_path))
    out = _load(str(tmp_path))
    assert set(out) == {"scenes", "sed", "morph", "centers", "shifts", "loss", "iterations", "flags"}
    assert info["scenes"] == info["of_scenes"] == 6
    assert all(a.dtype in (np.float32, np.float64) for a in out.values())
    np.testing.assert_array_equal(out["scenes"], np.arange(6))
    np.testing.assert_array_equal(out["morph"], b.morph_current.numpy())
    np.testing.assert_array_equal(out["loss"], b.mse_buf[:, 8].numpy())       # the last step's loss (it = 9)
    np.testing.assert_array_equal(out["centers"], b.centers.numpy())


def test_dump_large_batch_is_a_fixed_sample_under_64_mb(tmp_path):
    import bench
    b = _batch(1200)                              # 1200 x 64 KB of morphologies: over the limit
    info1 = bench.dump_outputs(b, str(tmp_path / "a"))
    info2 = bench.dump_outputs(b, str(tmp_path / "b"))
    assert 0 < info1["scenes"] < 1200 and info1 == dict(info2, dir=info1["dir"])
    on_disk = sum(os.path.getsize(os.path.join(info1["dir"], f)) for f in os.listdir(info1["dir"]))
    assert on_disk <= 64 << 20
    a, c = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    for k in a:
        np.testing.assert_array_equal(a[k], c[k])
    idx = a["scenes"].astype(np.int64)
    assert np.all(np.diff(idx) > 0)
    np.testing.assert_array_equal(a["morph"], b.morph_current.numpy()[idx])
    np.testing.assert_array_equal(a["sed"], b.sed_current.numpy()[idx])
