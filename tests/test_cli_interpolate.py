"""`pose --ground_filter file.ply --ground_interpolate [--ground_smooth n]`: the DTM picture is hole-free and decodes to
Context.groundFilter(interpolate=True)'s DTM, one more line is printed; without the flag the tool writes and prints what
it did before (the picture byte for byte, the lines but for the time)."""
import os

import numpy as np
import pytest

import raster_reference as rr
from test_cli_orthophoto import _golden_ply, _png, _pts_of, _run

FLAGS = ("--ground_interpolate", "--ground_smooth n")


def _lines(res):
    return [ln for ln in res.stdout.splitlines() if not ln.startswith("ground filter time")]


def _decoded(dtm):
    has = ~np.isnan(dtm)
    z_min, z_max = (dtm[has] + np.float32(0)).min(), (dtm[has] + np.float32(0)).max()
    d16, step = rr.height_png16(dtm, z_min, z_max)
    return d16[::-1], z_min, z_max, step  # north up


# ---- without a GPU ------------------------------------------------------------------------------------------------------
def test_cli_ground_interpolate_refusals(tmp_path):
    src, _ = _golden_ply(tmp_path)
    for argv, text in (([src, "--ground_interpolate", "--ground_fill_radius", "3"], "--ground_interpolate needs --ground_fill_radius 0"),
                       ([src, "--ground_interpolate", "--ground_smooth", "9"], "--ground_smooth must be in 0..8"),
                       ([src, "--ground_interpolate", "--ground_smooth", "-1"], "--ground_smooth must be in 0..8"),
                       ([src, "--ground_interpolate", "--ground_smooth"], "missing value after --ground_smooth")):
        res = _run(["--ground_filter"] + argv, timeout=60)
        out = res.stdout + res.stderr
        assert res.returncode != 0 and text in out and "unknown flag" not in out, (argv, out)
    assert sorted(os.listdir(str(tmp_path))) == ["cloud.ply"]
    usage = _run(["--help"], timeout=60).stdout
    assert all(f in usage for f in FLAGS)
    # elsewhere the flags are parsed and ignored
    res = _run(["--downsample", str(tmp_path / "none.ply"), "--ground_interpolate", "--ground_smooth", "99"], timeout=60)
    out = res.stdout + res.stderr
    assert "unknown flag" not in out and "--ground" not in out and "could not read" in out


# ---- on the GPU ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_cli_ground_filter_with_and_without_ground_interpolate(tmp_path):
    import online_3d_reconstruction_amd as o3dr
    src, v = _golden_ply(tmp_path)
    pts = _pts_of(v)
    png = str(tmp_path / "dtm_cloud.ply.png")
    with o3dr.Context(0) as ctx:
        ground, dtm0, ginfo = ctx.groundFilter(pts, 0.05, return_dtm=True, return_info=True)
        _, dtm2, _, dinfo = ctx.groundFilter(pts, 0.05, return_dtm=True, return_info=True, interpolate=True)
        _, dtm5 = ctx.groundFilter(pts, 0.05, return_dtm=True, interpolate=True, smooth=5)
    assert ginfo.n_dtm_empty > 0 and dinfo.n_empty == 0 and dinfo.n_data == ginfo.n_ground_cells

    # without the flag: the picture with its holes, no new line; --ground_smooth alone changes nothing
    plain = _run(["--ground_filter", src, "--voxel_size", "0.05"])
    assert plain.returncode == 0, plain.stdout + plain.stderr
    plain_png = open(png, "rb").read()
    pic = _png(png)
    want, z_min, z_max, step = _decoded(dtm0)
    assert pic.dtype == np.uint16 and np.array_equal(pic, want) and (pic == 0).sum() == ginfo.n_dtm_empty
    assert "interpolated" not in plain.stdout
    assert f"dtm z_min {z_min:.9g} z_max {z_max:.9g} step {step:.17g}" in plain.stdout
    os.remove(png)
    again = _run(["--ground_filter", src, "--voxel_size", "0.05", "--ground_smooth", "5"])
    assert again.returncode == 0 and open(png, "rb").read() == plain_png and _lines(again) == _lines(plain)

    # with it: no 0 pixel, the API's interpolated DTM, one more line, the rest of the output unchanged
    for argv, dtm in ((["--ground_interpolate"], dtm2), (["--ground_interpolate", "--ground_smooth", "5"], dtm5)):
        res = _run(["--ground_filter", src, "--voxel_size", "0.05"] + argv)
        assert res.returncode == 0, res.stdout + res.stderr
        pic = _png(png)
        want, z_min, z_max, step = _decoded(dtm)
        assert pic.dtype == np.uint16 and not (pic == 0).any() and np.array_equal(pic, want)
        new = f"dtm interpolated: {dinfo.n_data} data cells, {dinfo.n_filled} filled, {dinfo.n_levels} levels"
        zline = f"dtm z_min {z_min:.9g} z_max {z_max:.9g} step {step:.17g}"
        assert new in res.stdout and zline in res.stdout
        assert [ln for ln in _lines(res) if ln != new and not ln.startswith("dtm z_min")] == [ln for ln in _lines(plain) if not ln.startswith("dtm z_min")]
        # the two clouds do not change
        for name in ("terrain_cloud.ply", "objects_cloud.ply"):
            assert os.path.getsize(str(tmp_path / name)) > 0
    assert not np.array_equal(dtm2.view(np.uint32), dtm5.view(np.uint32))
