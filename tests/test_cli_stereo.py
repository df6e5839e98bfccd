"""The stereo modes of the C++ host layer (`online_3d_reconstruction_amd/bin/pose`): the `--stereo_disparity left.png
right.png` tool and `--gpu_disparity --right_image_dir` in a reconstruction run.  The tool's PNG must decode to exactly the
API's image, and a run that makes its disparities on the GPU must write the cloud.ply a run fed the tool's PNGs through
--disparity_dir writes, byte for byte."""
import os
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest

from conftest import load_frame
from test_cli_pose import POSE_BIN, _write_dataset

SHIFT = 80  # the right image is the left one moved by this many columns: above the reconstruction's min_disparity of 64
FLAGS = ["--stereo_n_disparities", "32", "--stereo_min_disparity", "64", "--stereo_paths", "4"]


def _run(cmd, timeout=300):
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)
    return res.returncode, res.stdout + res.stderr


def _decode_grey_png(path):
    """an 8-bit greyscale PNG whose rows all use filter 0, with the standard library alone"""
    raw = open(path, "rb").read()
    assert raw[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, w, h = 8, b"", 0, 0
    while pos < len(raw):
        n, kind = struct.unpack(">I4s", raw[pos:pos + 8])
        data = raw[pos + 8:pos + 8 + n]
        assert zlib.crc32(kind + data) == struct.unpack(">I", raw[pos + 8 + n:pos + 12 + n])[0], kind
        if kind == b"IHDR":
            w, h, depth, ctype, comp, flt, inter = struct.unpack(">IIBBBBB", data)
            assert (depth, ctype, comp, flt, inter) == (8, 0, 0, 0, 0)
        elif kind == b"IDAT":
            idat += data
        pos += 12 + n
    rows = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, w + 1)  # (checks the Adler-32 as well)
    assert not rows[:, 0].any()
    return np.ascontiguousarray(rows[:, 1:])


def _shifted(bgr):
    right = np.empty_like(bgr)
    right[:, :-SHIFT] = bgr[:, SHIFT:]
    right[:, -SHIFT:] = bgr[:, -1:]
    return right


def _save_bgr(path, bgr):
    from PIL import Image
    Image.fromarray(np.ascontiguousarray(bgr[:, :, ::-1]), "RGB").save(path)


@pytest.mark.gpu
def test_stereo_tool_equals_the_api(tmp_path, ctx):
    bgr = np.ascontiguousarray(load_frame("1248")[1][300:530, 500:803])  # 230 x 303: more than one 65535-byte stored block
    right = _shifted(bgr)
    lp, rp = str(tmp_path / "left.png"), str(tmp_path / "right.png")
    _save_bgr(lp, bgr)
    _save_bgr(rp, right)
    for flags, kw in ((["--stereo_n_disparities", "96"], dict(n_disparities=96)),
                      (["--stereo_n_disparities", "32", "--stereo_min_disparity", "64", "--stereo_p1", "5", "--stereo_p2", "60", "--stereo_paths", "4",
                        "--stereo_uniqueness", "0", "--stereo_lr_max_diff", "-1"],
                       dict(n_disparities=32, min_disparity=64, p1=5, p2=60, n_paths=4, uniqueness=0, lr_max_diff=-1))):
        rc, out = _run([POSE_BIN, "--stereo_disparity", lp, rp] + flags)
        assert rc == 0, out
        want = ctx.stereoDisparity(bgr, right, **kw)
        got = _decode_grey_png(lp + ".disparity.png")
        assert (want == SHIFT).mean() > 0.5 and np.array_equal(got, want)
        assert f"accepted {int((want != 0).sum())} of {want.size} pixels" in out, out
    rc, out = _run([POSE_BIN, "--stereo_disparity", lp, str(tmp_path / "missing.png")])
    assert rc != 0 and "could not read" in out
    rc, out = _run([POSE_BIN, "--stereo_disparity", lp])
    assert rc != 0 and "needs left.png and right.png" in out
    rc, out = _run([POSE_BIN, "--stereo_disparity", lp, rp, "--stereo_n_disparities", "48"])
    assert rc != 0 and "n_disparities" in out


@pytest.mark.gpu
def test_gpu_disparity_run_equals_a_disparity_dir_run(tmp_path):
    tmp = str(tmp_path)
    _write_dataset(tmp)
    for d in ("right", "disp2", "output2"):
        os.makedirs(f"{tmp}/{d}")
    for name in ("1248", "1249"):
        _save_bgr(f"{tmp}/right/{name}.png", _shifted(load_frame(name)[1]))
        rc, out = _run([POSE_BIN, "--stereo_disparity", f"{tmp}/images/{name}.png", f"{tmp}/right/{name}.png"] + FLAGS)
        assert rc == 0, out
        shutil.copy(f"{tmp}/images/{name}.png.disparity.png", f"{tmp}/disp2/{name}.png")
    base = [POSE_BIN, "1248", "1249", "--jump_pixels", "15", "--voxel_size", "0.05", "--only_MAVLink", "--data_dir", tmp + "/data_files/",
            "--image_dir", tmp + "/images/"]
    rc, out = _run(base + ["--output_dir", tmp + "/output/", "--gpu_disparity", "--right_image_dir", tmp + "/right/"] + FLAGS)
    assert rc == 0 and "2 disparity images from o3dr_stereo_disparity" in out and out.count("Accepted!") == 2, out
    rc, out2 = _run(base + ["--output_dir", tmp + "/output2/", "--disparity_dir", tmp + "/disp2/"])
    assert rc == 0 and out2.count("Accepted!") == 2, out2
    a, b = open(tmp + "/output/cloud.ply", "rb").read(), open(tmp + "/output2/cloud.ply", "rb").read()
    assert a == b and len(a) > 10000
    rc, out3 = _run(base + ["--output_dir", tmp + "/output2/", "--disparity_dir", tmp + "/disparities/"])
    assert rc == 0 and open(tmp + "/output2/cloud.ply", "rb").read() != a  # the computed images really took part


def test_gpu_disparity_refuses_what_it_does_not_serve(tmp_path):
    """(the refusals come from the flag parser, before any device is opened)"""
    tmp = str(tmp_path)
    base = [POSE_BIN, "1248", "1249", "--data_dir", tmp + "/", "--gpu_disparity", "--right_image_dir", tmp + "/right/"]
    for extra in (["--gpus", "2"], ["--partitioned_merge"], ["--reference_fanout"], ["--use_segment_labels"]):
        rc, out = _run(base + extra)
        assert rc != 0 and "--gpu_disparity is not available" in out, out
    rc, out = _run([POSE_BIN, "1248", "1249", "--data_dir", tmp + "/", "--gpu_disparity"])
    assert rc != 0 and "--gpu_disparity needs --right_image_dir" in out, out
