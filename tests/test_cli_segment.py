"""The segmentation modes of the C++ host layer (`online_3d_reconstruction_amd/bin/pose`): the `--segment_image image.png`
tool and `--gpu_segment_labels` under `--use_segment_labels`.  The tool's 16-bit PNG, read back through `--print_label_png`,
must hold exactly the API's labels, and a run that makes its labels on the GPU must write the cloud.ply a run fed the tool's
PNGs through --segment_labels_dir writes, byte for byte."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import segment_reference as R
from conftest import load_frame
from test_cli_pose import POSE_BIN, _write_dataset


def _run(cmd, timeout=300):
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)
    return res.returncode, res.stdout + res.stderr


def _save_bgr(path, bgr):
    from PIL import Image
    Image.fromarray(np.ascontiguousarray(bgr[:, :, ::-1]), "RGB").save(path)


def _labels_of_png(path):
    res = subprocess.run([POSE_BIN, "--print_label_png", path], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stdout + res.stderr
    lines = res.stdout.strip().splitlines()
    lab = np.array([l.split() for l in lines[1:]], np.int64)
    assert lines[0].split() == [str(lab.shape[0]), str(lab.shape[1])]
    return lab


@pytest.mark.gpu
def test_segment_tool_equals_the_api(tmp_path, ctx):
    img = R.region_image()[0]
    path = str(tmp_path / "img.png")
    _save_bgr(path, img)
    rc, out = _run([POSE_BIN, "--segment_image", path])
    assert rc == 0, out
    want, (info,) = ctx.segmentImage(img, return_info=True)
    assert np.array_equal(_labels_of_png(path + ".labels.png"), want)
    assert f"{info.n_centres} centres, {info.n_components} components, {info.n_merged} merged, {info.n_labels} labels" in out, out
    flags = ["--segment_step", "8", "--segment_compactness", "10", "--segment_iterations", "3", "--segment_min_size", "5"]
    rc, out = _run([POSE_BIN, "--segment_image", path] + flags)
    assert rc == 0, out
    want2 = ctx.segmentImage(img, 8, 10, 3, 5)
    assert np.array_equal(_labels_of_png(path + ".labels.png"), want2) and not np.array_equal(want2, want)
    rc, out = _run([POSE_BIN, "--segment_image", path, "--segment_step", "3"])
    assert rc != 0 and "step" in out, out
    # more than 65536 labels: refused, nothing written
    big = R.checkerboard(260, 260)
    bpath = str(tmp_path / "board.png")
    _save_bgr(bpath, np.repeat(big[:, :, None], 3, axis=2))
    rc, out = _run([POSE_BIN, "--segment_image", bpath, "--segment_step", "5", "--segment_compactness", "0", "--segment_min_size", "0"])
    assert rc != 0 and "more than 65536 labels" in out and f"{260 * 260} labels" in out, out
    assert not os.path.exists(bpath + ".labels.png")


@pytest.mark.gpu
def test_gpu_segment_labels_run_equals_a_segment_labels_dir_run(tmp_path, ctx):
    tmp = str(tmp_path)
    _write_dataset(tmp)
    for d in ("labels", "output2"):
        os.makedirs(f"{tmp}/{d}")
    flags = ["--segment_step", "24", "--segment_compactness", "20", "--segment_iterations", "3"]
    for name in ("1248", "1249"):
        rc, out = _run([POSE_BIN, "--segment_image", f"{tmp}/images/{name}.png"] + flags)
        assert rc == 0, out
        shutil.copy(f"{tmp}/images/{name}.png.labels.png", f"{tmp}/labels/{name}.png")
        want = ctx.segmentImage(load_frame(name)[1], 24, 20, 3)
        assert want.max() > 255 and np.array_equal(_labels_of_png(f"{tmp}/labels/{name}.png"), want)
    base = [POSE_BIN, "1248", "1249", "--jump_pixels", "15", "--voxel_size", "0.05", "--only_MAVLink", "--data_dir", tmp + "/data_files/",
            "--image_dir", tmp + "/images/", "--disparity_dir", tmp + "/disparities/", "--use_segment_labels"]
    rc, out = _run(base + ["--output_dir", tmp + "/output/", "--gpu_segment_labels"] + flags)
    assert rc == 0 and "--gpu_segment_labels: 2 label images from o3dr_segment_image" in out, out
    assert out.count("Accepted!") == 2 and "plane-fitted disparity: 2 frames" in out, out
    rc, out2 = _run(base + ["--output_dir", tmp + "/output2/", "--segment_labels_dir", tmp + "/labels/"])
    assert rc == 0 and out2.count("Accepted!") == 2, out2
    a, b = open(tmp + "/output/cloud.ply", "rb").read(), open(tmp + "/output2/cloud.ply", "rb").read()
    assert a == b and len(a) > 10000


def test_segment_refusals(tmp_path):
    """(the refusals come from the flag parser, before any device is opened)"""
    tmp = str(tmp_path)
    base = [POSE_BIN, "1248", "1249", "--data_dir", tmp + "/"]
    rc, out = _run(base + ["--gpu_segment_labels"])
    assert rc != 0 and "--gpu_segment_labels makes the labels of --use_segment_labels" in out, out
    rc, out = _run(base + ["--use_segment_labels", "--gpu_segment_labels", "--segment_labels_dir", tmp + "/labels/"])
    assert rc != 0 and "--gpu_segment_labels cannot be combined with --segment_labels_dir" in out, out
    rc, out = _run([POSE_BIN, "--segment_image", str(tmp_path / "missing.png")])
    assert rc != 0 and "could not read" in out, out
    rc, out = _run([POSE_BIN, "--segment_image"])
    assert rc != 0 and "needs image.png" in out, out
