"""`pose --cluster_cloud file.ply --cluster_tolerance t`: the two PLYs and the record table, decoded, against
Context.clusterCloud on the same points; the printed lines; the refusals."""
import os

import numpy as np
import pytest

from test_cli_orthophoto import GOLDEN, _pts_of, _run
from test_cluster_reference import random_scene
from test_plane_segmentation import _read_ply

FLAGS = ("--cluster_cloud file.ply", "--cluster_tolerance t", "--cluster_min_size n", "--cluster_max_size n")


def small_ply(tmp_path, n=1500):
    """the first n points of the random scene with random colours as a binary PLY of the layout the tool reads and writes"""
    z = np.load(os.path.join(GOLDEN, "cloud_ply.npz"))
    v = np.zeros(n, z["vertices"].dtype)
    xyz = random_scene()[:n]
    v["x"], v["y"], v["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    rgb = np.random.default_rng(2).integers(0, 256, (n, 3), dtype=np.uint8)
    v["r"], v["g"], v["b"] = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    header = z["header"].tobytes().replace(b"element vertex 55940", b"element vertex %d" % n)
    src = str(tmp_path / "cloud.ply")
    with open(src, "wb") as f:
        f.write(header + v.tobytes() + z["tail"].tobytes())
    return src, v


# ---- without a GPU ------------------------------------------------------------------------------------------------------
def test_cli_cluster_cloud_refusals(tmp_path):
    src, _ = small_ply(tmp_path, 10)
    for argv, text in (([], "missing argument"), ([str(tmp_path / "none.ply"), "--cluster_tolerance", "1"], "could not read"),
                       ([src], "--cluster_cloud needs --cluster_tolerance"), ([src, "--cluster_min_size", "3"], "--cluster_cloud needs --cluster_tolerance"),
                       ([src, "--cluster_tolerance", "0"], "--cluster_tolerance must be finite and > 0"),
                       ([src, "--cluster_tolerance", "nan"], "--cluster_tolerance must be finite and > 0"),
                       ([src, "--cluster_tolerance", "1", "--cluster_min_size", "0"], "--cluster_min_size must be >= 1"),
                       ([src, "--cluster_tolerance", "1", "--cluster_min_size", "5", "--cluster_max_size", "4"], "--cluster_max_size must be >="),
                       ([src, "--cluster_tolerance"], "missing value after --cluster_tolerance")):
        res = _run(["--cluster_cloud"] + argv, timeout=60)
        out = res.stdout + res.stderr
        assert res.returncode != 0 and text in out and "unknown flag" not in out, (argv, out)
    assert sorted(os.listdir(str(tmp_path))) == ["cloud.ply"]
    usage = _run(["--help"], timeout=60).stdout
    assert all(f in usage for f in FLAGS) and all(t in usage for t in ("clusters_<file>", "unclustered_<file>", "clusters_<file>.txt"))
    # elsewhere the --cluster_* flags are parsed and ignored
    res = _run(["--downsample", str(tmp_path / "none.ply"), "--cluster_tolerance", "-1", "--cluster_min_size", "0", "--cluster_max_size", "-5"], timeout=60)
    out = res.stdout + res.stderr
    assert "unknown flag" not in out and "--cluster" not in out and "could not read" in out


# ---- on the GPU ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("flags,kw", [([], {}), (["--cluster_min_size", "3", "--cluster_max_size", "40"], dict(min_size=3, max_size=40))])
def test_cli_cluster_cloud_equals_the_api(tmp_path, flags, kw):
    import online_3d_reconstruction_amd as o3dr
    src, v = small_ply(tmp_path)
    pts = _pts_of(v)
    res = _run(["--cluster_cloud", src, "--cluster_tolerance", "0.5"] + flags)
    assert res.returncode == 0, res.stdout + res.stderr
    with o3dr.Context(0) as ctx:
        label, rec, indices, info = ctx.clusterCloud(pts, 0.5, return_clusters=True, return_indices=True, return_info=True, **kw)
    K = info.n_clusters
    assert K > 10 and (info.n_rejected_points > 0) == bool(kw)
    c = _read_ply(str(tmp_path / "clusters_cloud.ply"))
    u = _read_ply(str(tmp_path / "unclustered_cloud.ply"))
    assert len(c) == info.n_clustered_points and len(u) == info.n_rejected_points
    want = pts[indices]                                   # cluster by cluster, each in ascending index
    number = np.repeat(np.arange(K, dtype=np.uint32), rec["size"])
    rgba = ((number + np.uint32(1)) * np.uint32(2654435761) >> np.uint32(8)) | np.uint32(0x404040)
    for ax in "xyz":
        assert np.array_equal(c[ax].view(np.uint32), want[ax].view(np.uint32))
        assert np.array_equal(u[ax].view(np.uint32), pts[label < 0][ax].view(np.uint32))  # input order
    assert np.array_equal(c["red"], (rgba >> 16) & 255) and np.array_equal(c["green"], (rgba >> 8) & 255) and np.array_equal(c["blue"], rgba & 255)
    rest = pts[label < 0]["rgba"]
    assert np.array_equal(u["red"], (rest >> 16) & 255) and np.array_equal(u["blue"], rest & 255)
    lines = open(str(tmp_path / "clusters_cloud.ply.txt")).read().splitlines()
    assert len(lines) == K
    for k, r in enumerate(rec):
        floats = " ".join(f"{float(x):.9g}" for x in list(r["lo"]) + list(r["hi"]))
        assert lines[k] == f"{k} {r['first']} {r['size']} {floats} " + " ".join(f"{float(x):.17g}" for x in r["centroid"]), k
    out = res.stdout
    assert f"points in {len(pts)}, linked pairs {info.n_pairs}" in out
    assert (f"components {info.n_components} (largest {info.largest}), clusters {K}, too small {info.n_too_small}, "
            f"too large {info.n_too_large}") in out
    assert f"clustered points {info.n_clustered_points}, other points {info.n_rejected_points}" in out and "cluster time" in out
    assert all(("cluster " + lines[k]) in out for k in range(10)) and ("cluster " + lines[10]) not in out
