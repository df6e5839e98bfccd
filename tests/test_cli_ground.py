"""`pose --ground_filter file.ply`: the two PLYs and the DTM picture, decoded, against Context.groundFilter on the same file
and the stated 16-bit quantisation of the heights (raster_reference.height_png16); the printed lines; the refusals."""
import os

import numpy as np
import pytest

import raster_reference as rr
from test_cli_orthophoto import _golden_ply, _png, _pts_of, _run
from test_plane_segmentation import _read_ply

FLAGS = ("--ground_filter file.ply", "--ground_max_window r", "--ground_window_base b", "--ground_linear", "--ground_slope s",
         "--ground_initial_distance m", "--ground_max_distance m", "--ground_fill_radius r")


# ---- without a GPU ------------------------------------------------------------------------------------------------------
def test_cli_ground_filter_refusals(tmp_path):
    src, _ = _golden_ply(tmp_path)
    for argv, text in (([], "missing argument"), (["--voxel_size", "0.05"], "missing argument"),
                       ([str(tmp_path / "none.ply")], "could not read"),
                       ([src, "--ground_max_window", "0"], "--ground_max_window must be in 1..128"),
                       ([src, "--ground_max_window", "129"], "--ground_max_window must be in 1..128"),
                       ([src, "--ground_window_base", "1"], "--ground_window_base must be >= 2"),
                       ([src, "--ground_window_base", "0", "--ground_linear"], "--ground_window_base must be >= 2, or >= 1 with --ground_linear"),
                       ([src, "--ground_window_base", "17", "--ground_linear"], "no window fits"),
                       ([src, "--ground_slope", "-1"], "--ground_slope must be finite and >= 0"),
                       ([src, "--ground_initial_distance", "nan"], "--ground_initial_distance must be finite and >= 0"),
                       ([src, "--ground_max_distance", "inf"], "--ground_max_distance must be finite and >= 0"),
                       ([src, "--ground_fill_radius", "33"], "--ground_fill_radius must be in 0..32"),
                       ([src, "--ground_fill_radius", "-1"], "--ground_fill_radius must be in 0..32"),
                       ([src, "--ground_slope"], "missing value after --ground_slope")):
        res = _run(["--ground_filter"] + argv, timeout=60)
        out = res.stdout + res.stderr
        assert res.returncode != 0 and text in out and "unknown flag" not in out, (argv, out)
    assert sorted(os.listdir(str(tmp_path))) == ["cloud.ply"]
    usage = _run(["--help"], timeout=60).stdout
    assert all(f in usage for f in FLAGS) and "terrain_<file>" in usage and "objects_<file>" in usage and "dtm_<file>.png" in usage
    # elsewhere the --ground_* flags are parsed and ignored
    res = _run(["--downsample", str(tmp_path / "none.ply"), "--ground_max_window", "999", "--ground_window_base", "0", "--ground_linear",
                "--ground_slope", "-1", "--ground_initial_distance", "-1", "--ground_max_distance", "-1", "--ground_fill_radius", "99"], timeout=60)
    out = res.stdout + res.stderr
    assert "unknown flag" not in out and "--ground" not in out and "could not read" in out


# ---- on the GPU ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gctx():
    import online_3d_reconstruction_amd as o3dr
    with o3dr.Context(0) as c:
        yield c


def _check_files(tmp_path, pts, res, ground, dtm, info, radii, thr):
    t = _read_ply(str(tmp_path / "terrain_cloud.ply"))
    o = _read_ply(str(tmp_path / "objects_cloud.ply"))
    on = ground != 0
    assert len(t) == int(on.sum()) > 0 and len(o) == int((~on).sum()) > 0
    for got, want in ((t, pts[on]), (o, pts[~on])):  # input order
        for ax in "xyz":
            assert np.array_equal(got[ax].view(np.uint32), want[ax].view(np.uint32))
        assert np.array_equal(got["red"], (want["rgba"] >> 16) & 255) and np.array_equal(got["blue"], want["rgba"] & 255)
    has = ~np.isnan(dtm)
    z_min, z_max = (dtm[has] + np.float32(0)).min(), (dtm[has] + np.float32(0)).max()
    d16, step = rr.height_png16(dtm, z_min, z_max)
    pic = _png(str(tmp_path / "dtm_cloud.ply.png"))
    assert pic.dtype == np.uint16 and np.array_equal(pic, d16[::-1])  # north up
    assert (pic == 0).sum() == info.n_dtm_empty and pic[pic > 0].min() == 1
    out = res.stdout
    assert f"points in {len(pts)} (outside the box 0)" in out
    assert f"box cx0 {info.cx0} cy0 {info.cy0} width {info.width} height {info.height}" in out
    for k, (r, th, rem) in enumerate(zip(radii, thr, info.n_removed)):
        assert f"iteration {k} radius {r} threshold {float(th):.9g} removed cells {rem}" in out, (k, out)
    assert f"iteration {len(radii)} " not in out
    assert f"cells occupied {info.n_occupied}, ground {info.n_ground_cells}, dtm filled {info.n_dtm_filled}, dtm empty {info.n_dtm_empty}" in out
    assert f"ground points {info.n_ground_points}, object points {len(pts) - info.n_ground_points}" in out
    assert f"dtm z_min {z_min:.9g} z_max {z_max:.9g} step {step:.17g}" in out and "ground filter time" in out


@pytest.mark.gpu
def test_cli_ground_filter_on_the_reference_cloud(tmp_path, gctx):
    import online_3d_reconstruction_amd as o3dr
    src, v = _golden_ply(tmp_path)
    pts = _pts_of(v)
    # the defaults
    res = _run(["--ground_filter", src, "--voxel_size", "0.05"])
    assert res.returncode == 0, res.stdout + res.stderr
    ground, dtm, info = gctx.groundFilter(pts, 0.05, return_dtm=True, return_info=True)
    assert info.n_iterations == 5 and info.n_dtm_filled == 0 and sum(info.n_removed) > 0
    _check_files(tmp_path, pts, res, ground, dtm, info, *o3dr.groundSchedule(0.05))
    # every flag
    kw = dict(max_window_radius=24, window_base=3, exponential=False, slope=0.4, initial_distance=0.05, max_distance=0.5, fill_radius=6)
    res = _run(["--ground_filter", src, "--voxel_size", "0.1", "--ground_max_window", "24", "--ground_window_base", "3", "--ground_linear",
                "--ground_slope", "0.4", "--ground_initial_distance", "0.05", "--ground_max_distance", "0.5", "--ground_fill_radius", "6"])
    assert res.returncode == 0, res.stdout + res.stderr
    ground, dtm, info = gctx.groundFilter(pts, 0.1, return_dtm=True, return_info=True, **kw)
    assert info.n_iterations == 8 and info.n_dtm_filled > 0 and info.n_ground_points > info.n_ground_cells
    radii, thr = o3dr.groundSchedule(0.1, **{k: x for k, x in kw.items() if k != "fill_radius"})
    _check_files(tmp_path, pts, res, ground, dtm, info, radii, thr)
