"""`pose --contours file.ply --contour_interval m [--contour_base b] [--voxel_size m] [--contour_surface dtm|dsm]
[--contour_min_segments n]`: contours_<file>.geojson holds Context.contourRaster's lines of the same surface, coordinate for
coordinate (%.17g round-trips a double): of rasterizeMap(select="top")'s heights for dsm, of groundFilter(interpolate=True)'s
terrain model for dtm."""
import json
import os

import numpy as np
import pytest

from test_cli_orthophoto import _golden_ply, _pts_of, _run

FLAGS = ("--contours file.ply", "--contour_interval m", "--contour_base b", "--contour_surface dtm|dsm", "--contour_min_segments n")
CELL = 0.1


# ---- without a GPU ------------------------------------------------------------------------------------------------------
def test_cli_contours_refusals(tmp_path):
    src, _ = _golden_ply(tmp_path)
    for argv, text in (([], "missing argument"), ([src], "--contours needs --contour_interval m"),
                       ([str(tmp_path / "none.ply"), "--contour_interval", "1"], "could not read"),
                       ([src, "--contour_interval", "0"], "--contour_interval must be finite and > 0"),
                       ([src, "--contour_interval", "-2"], "--contour_interval must be finite and > 0"),
                       ([src, "--contour_interval", "nan"], "--contour_interval must be finite and > 0"),
                       ([src, "--contour_interval", "1", "--contour_base", "inf"], "--contour_base must be finite"),
                       ([src, "--contour_interval", "1", "--contour_surface", "dem"], "--contour_surface must be dtm or dsm"),
                       ([src, "--contour_interval", "1", "--contour_min_segments", "0"], "--contour_min_segments must be >= 1"),
                       ([src, "--contour_interval"], "missing value after --contour_interval")):
        res = _run(["--contours"] + argv, timeout=60)
        out = res.stdout + res.stderr
        assert res.returncode != 0 and text in out and "unknown flag" not in out, (argv, out)
    assert sorted(os.listdir(str(tmp_path))) == ["cloud.ply"]
    usage = _run(["--help"], timeout=60).stdout
    assert all(f in usage for f in FLAGS)
    # elsewhere the flags are parsed and ignored
    res = _run(["--downsample", str(tmp_path / "none.ply"), "--contour_interval", "-1", "--contour_base", "nan", "--contour_surface", "x",
                "--contour_min_segments", "-5"], timeout=60)
    out = res.stdout + res.stderr
    assert "unknown flag" not in out and "--contour" not in out and "could not read" in out


# ---- on the GPU ---------------------------------------------------------------------------------------------------------
def _same_lines(features, lines, vertices, min_segments=1):
    import online_3d_reconstruction_amd as o3dr
    poly = o3dr.contourPolylines(lines, vertices)
    keep = [i for i, l in enumerate(lines) if l["n_segments"] >= min_segments]
    assert len(features) == len(keep) > 0
    for f, i in zip(features, keep):
        l = lines[i]
        assert f["type"] == "Feature" and f["geometry"]["type"] == "LineString"
        assert f["properties"] == {"line": i, "level": int(l["k"]), "elevation": float(l["level"]), "closed": int(l["closed"]),
                                   "segments": int(l["n_segments"])}
        got = np.array(f["geometry"]["coordinates"], np.float64)
        assert got.shape == poly[i].shape and got.tobytes() == poly[i].tobytes(), i


@pytest.mark.gpu
@pytest.mark.parametrize("surface", ["dsm", "dtm"])
def test_cli_contours_hold_the_apis_lines(tmp_path, surface):
    import online_3d_reconstruction_amd as o3dr
    src, v = _golden_ply(tmp_path)
    pts = _pts_of(v)
    interval, base = 0.25, 0.05
    with o3dr.Context(0) as ctx:
        bounds = ctx.rasterExtent(pts, CELL)
        if surface == "dsm":
            Z = ctx.rasterizeMap(pts, CELL, bounds, select="top")[0]
        else:
            Z = ctx.groundFilter(pts, CELL, bounds, return_dtm=True, interpolate=True)[1]
        seg, lines, vertices, info = ctx.contourRaster(Z, interval, base, CELL, bounds[:2], return_lines=True, return_vertices=True,
                                                       return_info=True)
    assert np.isnan(Z).any() == (surface == "dsm") and info.n_lines > 10
    out = str(tmp_path / "contours_cloud.ply.geojson")
    argv = ["--contours", src, "--contour_interval", str(interval), "--contour_base", str(base), "--voxel_size", str(CELL)]
    res = _run(argv + (["--contour_surface", "dsm"] if surface == "dsm" else []))
    assert res.returncode == 0, res.stdout + res.stderr
    doc = json.load(open(out))
    assert doc["type"] == "FeatureCollection"
    _same_lines(doc["features"], lines, vertices)
    assert f"points in {len(pts)}, surface {surface}" in res.stdout and "contour time" in res.stdout
    assert "box cx0 {} cy0 {} width {} height {}".format(*bounds) in res.stdout
    assert f"levels k {info.k_lo} .. {info.k_hi} (interval {interval:.17g} base {base:.17g})" in res.stdout
    assert (f"quads {info.n_quads} (crossed {info.n_quads_crossed}), segments {info.n_segments}, lines {info.n_lines} (closed {info.n_closed}, "
            f"longest {info.n_longest} segments), vertices {info.n_vertices}") in res.stdout
    # --contour_min_segments drops the shorter lines and keeps the numbers
    m = int(np.median(lines["n_segments"])) + 1
    os.remove(out)
    res = _run(argv + ["--contour_surface", surface, "--contour_min_segments", str(m)])
    assert res.returncode == 0, res.stdout + res.stderr
    _same_lines(json.load(open(out))["features"], lines, vertices, m)
