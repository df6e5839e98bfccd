"""bench.py --dump-outputs: the merged cloud is written exactly, in float32 / float64, within 64 MB (no GPU needed)."""
import os

import numpy as np
import torch

import bench
from conftest import random_cloud


def _as_tensor(pts):
    return torch.from_numpy(np.ascontiguousarray(pts).view(np.int32).reshape(-1, 4).copy())


def test_dump_outputs_round_trips_the_merged_cloud_bit_for_bit(tmp_path):
    pts = random_cloud(5000, seed=7)
    info = bench.dump_outputs(str(tmp_path), _as_tensor(pts))
    assert info["files"] == ["merged_rgba.npy", "merged_xyz.npy"] and info["merged_points"] == 5000
    xyz = np.load(tmp_path / "merged_xyz.npy")
    rgba = np.load(tmp_path / "merged_rgba.npy")
    assert xyz.dtype == np.float32 and xyz.shape == (5000, 3)
    assert rgba.dtype == np.float64 and rgba.shape == (5000,)
    for k, ax in enumerate("xyz"):
        assert np.array_equal(xyz[:, k].view(np.uint32), pts[ax].view(np.uint32))
    assert np.array_equal(rgba.astype(np.uint32), pts["rgba"])


def test_dump_outputs_samples_large_clouds_the_same_way_every_time(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_POINTS", 300)
    pts = random_cloud(4000, seed=8)
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(str(a), _as_tensor(pts))
    info = bench.dump_outputs(str(b), _as_tensor(pts))
    assert info["sampled_points"] == 300 and "merged_index.npy" in info["files"]
    for f in info["files"]:
        assert np.load(a / f).tobytes() == np.load(b / f).tobytes()
    idx = np.load(b / "merged_index.npy").astype(np.int64)
    assert np.all(np.diff(idx) > 0)
    assert np.array_equal(np.load(b / "merged_xyz.npy")[:, 2].view(np.uint32), pts["z"][idx].view(np.uint32))
    # a later, unsampled dump into the same folder leaves no stale index behind
    bench.dump_outputs(str(b), _as_tensor(pts[:100]))
    assert not os.path.exists(b / "merged_index.npy")


def test_dump_outputs_stays_within_64_mb():
    per_point = 3 * 4 + 8 + 8  # xyz float32, rgba float64, index float64
    assert bench.DUMP_MAX_POINTS * per_point <= 64 * 2**20
