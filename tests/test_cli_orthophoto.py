"""`pose --orthophoto file.ply` and `--orthophoto_out prefix` of a reconstruction run: the three PNGs, decoded, against
Context.rasterizeMap (rows flipped: the pictures are north up) and the stated 16-bit quantisation of the heights; the
printed counts; the refusals."""
import os
import subprocess

import numpy as np
import pytest

import raster_reference as rr
from conftest import GOLDEN
from test_cli_pose import POSE_BIN, _write_dataset

LIGHT = (-1.0, 1.0, 1.0)


def _run(argv, timeout=300):
    return subprocess.run([POSE_BIN] + argv, capture_output=True, text=True, timeout=timeout)


def _png(path):
    from PIL import Image
    return np.array(Image.open(path))


def _golden_ply(tmp_path):
    z = np.load(os.path.join(GOLDEN, "cloud_ply.npz"))
    src = str(tmp_path / "cloud.ply")
    with open(src, "wb") as f:
        f.write(z["header"].tobytes() + z["vertices"].tobytes() + z["tail"].tobytes())
    return src, z["vertices"]


# ---- without a GPU ------------------------------------------------------------------------------------------------------
def test_cli_orthophoto_refusals(tmp_path):
    src, _ = _golden_ply(tmp_path)
    for argv, text in (([], "missing argument"), (["--voxel_size", "0.05"], "missing argument"),
                       ([str(tmp_path / "none.ply")], "could not read"),
                       ([src, "--ortho_fill_radius", "33"], "--ortho_fill_radius must be in 0..32"),
                       ([src, "--ortho_fill_radius", "-1"], "--ortho_fill_radius must be in 0..32"),
                       ([src, "--ortho_light", "0", "0", "0"], "--ortho_light"), ([src, "--ortho_light", "1", "2"], "missing argument"),
                       ([src, "--ortho_select", "middle"], "--ortho_select must be first, top or bottom")):
        res = _run(["--orthophoto"] + argv, timeout=60)
        out = res.stdout + res.stderr
        assert res.returncode != 0 and text in out and "unknown flag" not in out, (argv, out)
    assert not [f for f in os.listdir(str(tmp_path)) if f.endswith(".png")]
    base = ["1248", "1249", "--orthophoto_out", str(tmp_path / "m_"), "--data_dir", str(tmp_path) + "/"]
    for extra in (["--gpus", "2"], ["--partitioned_merge"], ["--reference_fanout"]):
        res = _run(base + extra, timeout=60)
        assert res.returncode != 0 and "--orthophoto_out is not available with " + extra[0] in res.stdout + res.stderr
    usage = _run(["--help"], timeout=60).stdout
    assert "--orthophoto file.ply" in usage and "--orthophoto_out prefix" in usage and "--ortho_light lx ly lz" in usage
    # elsewhere the --ortho_* flags are parsed and ignored
    res = _run(["--downsample", str(tmp_path / "none.ply"), "--ortho_fill_radius", "99", "--ortho_select", "x", "--ortho_light", "0", "0", "0"],
               timeout=60)
    assert "unknown flag" not in res.stdout + res.stderr and "--ortho" not in res.stdout + res.stderr and "could not read" in res.stdout + res.stderr


# ---- on the GPU ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def octx():
    import online_3d_reconstruction_amd as o3dr
    with o3dr.Context(0) as c:
        yield c


def _api_pictures(ctx, pts, cell, **kw):
    """what the tool must write for this cloud: (ortho RGB, height uint16, shade or None, RasterInfo, step)"""
    got = ctx.rasterizeMap(pts, cell, return_info=True, **kw)
    info = got[-1]
    h16, step = rr.height_png16(got[0], info.z_min, info.z_max)
    shade = got[2][::-1] if "light" in kw else None
    return got[1][::-1, :, ::-1], h16[::-1], shade, info, step


def _pts_of(v):
    from online_3d_reconstruction_amd import POINT
    p = np.zeros(len(v), POINT)
    p["x"], p["y"], p["z"] = v["x"], v["y"], v["z"]
    p["rgba"] = (np.uint32(255) << 24) | (v["r"].astype(np.uint32) << 16) | (v["g"].astype(np.uint32) << 8) | v["b"].astype(np.uint32)
    return p


@pytest.mark.gpu
def test_cli_orthophoto_on_the_reference_cloud(tmp_path, octx):
    src, v = _golden_ply(tmp_path)
    pts = _pts_of(v)
    names = [str(tmp_path / (k + "_cloud.ply.png")) for k in ("ortho", "height", "shade")]
    # plain: no fill, no light -> no shade file
    res = _run(["--orthophoto", src, "--voxel_size", "0.05"])
    assert res.returncode == 0, res.stdout + res.stderr
    rgb, h16, _, info, step = _api_pictures(octx, pts, 0.05)
    assert np.array_equal(_png(names[0]), rgb) and np.array_equal(_png(names[1]), h16) and not os.path.exists(names[2])
    assert "points in 55940 (outside the box 0)" in res.stdout and "box cx0 9 cy0 -297 width 355 height 376" in res.stdout
    assert "cells occupied 55940 (shadowed points 0), filled 0, empty 77540" in res.stdout and "raster time" in res.stdout
    assert f"z_min {info.z_min:.9g} z_max {info.z_max:.9g} step {step:.17g}" in res.stdout
    assert h16.max() >= 65534 and h16[h16 > 0].min() == 1 and (h16 == 0).sum() == 77540
    # north up and not mirrored: the picture's first row is the greatest cy
    cy = np.floor(pts["y"] * (np.float32(1.0) / np.float32(0.05))).astype(np.int64)
    top = pts[cy == cy.max()]
    cx = np.floor(top["x"] * (np.float32(1.0) / np.float32(0.05))).astype(np.int64) - 9
    assert np.array_equal(_png(names[0])[0, cx, 0], (top["rgba"] >> 16) & 255)
    # every flag
    for select in ("top", "bottom"):
        res = _run(["--orthophoto", src, "--voxel_size", "0.1", "--ortho_select", select, "--ortho_fill_radius", "4", "--ortho_light", "-1",
                    "1", "1"])
        assert res.returncode == 0, res.stdout + res.stderr
        rgb, h16, shade, info, step = _api_pictures(octx, pts, 0.1, select=select, fill_radius=4, light=LIGHT)
        assert np.array_equal(_png(names[0]), rgb) and np.array_equal(_png(names[1]), h16) and np.array_equal(_png(names[2]), shade)
        assert _png(names[2]).dtype == np.uint8 and _png(names[1]).dtype == np.uint16
        assert f"cells occupied {info.n_occupied} (shadowed points {info.n_shadowed}), filled {info.n_filled}, empty {info.n_empty}" in res.stdout
        assert info.n_shadowed > 0 and info.n_filled > 0


@pytest.mark.gpu
def test_cli_reconstruction_run_writes_the_tools_files(tmp_path):
    """--orthophoto_out in a short run on the bundled frames: byte-identical to the tool on the run's cloud.ply"""
    tmp = str(tmp_path)
    _write_dataset(tmp)
    flags = ["--voxel_size", "0.05", "--ortho_fill_radius", "3", "--ortho_light", "-1", "1", "1", "--ortho_select", "top"]
    res = _run(["1248", "1249", "--jump_pixels", "15", "--only_MAVLink", "--sor", "0", "--data_dir", tmp + "/data_files/", "--image_dir",
                tmp + "/images/", "--disparity_dir", tmp + "/disparities/", "--output_dir", tmp + "/output/", "--orthophoto_out",
                tmp + "/output/map_"] + flags)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "cells occupied" in res.stdout and "raster time" in res.stdout
    tool = _run(["--orthophoto", tmp + "/output/cloud.ply"] + flags)
    assert tool.returncode == 0, tool.stdout + tool.stderr
    for k in ("ortho", "height", "shade"):
        a = open(f"{tmp}/output/map_{k}.png", "rb").read()
        b = open(f"{tmp}/output/{k}_cloud.ply.png", "rb").read()
        assert len(a) > 1000 and a == b, k
    pick = lambda out: [l for l in out.splitlines() if l.startswith(("box ", "cells ", "z_min "))]  # noqa: E731
    assert pick(res.stdout) == pick(tool.stdout) and len(pick(tool.stdout)) == 3
