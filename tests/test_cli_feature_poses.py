"""`--feature_poses` of the C++ host layer (`online_3d_reconstruction_amd/bin/pose`): every cycle's frames go through
o3dr_orb_detect, o3dr_keypoints_3d and o3dr_pose_chain, with the earlier cycles' frames as the chain's history."""
import re
import subprocess

import pytest

from test_cli_pose import POSE_BIN, _read_ply, _write_dataset

STATUS = re.compile(r"^(\d+) pose chain: (ANCHOR|MATCHED|TOO_FEW|DEGENERATE|RMS) pairs (\d+)/(\d+) good (\d+) used (\d+) rms (\S+)\t(Accepted|Rejected)!$",
                    re.M)


def _run(cmd, timeout=300):
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)
    return res.returncode, res.stdout + res.stderr


def _base(tmp):
    return [POSE_BIN, "1248", "1249", "--jump_pixels", "15", "--voxel_size", "0.05", "--data_dir", tmp + "/data_files/",
            "--image_dir", tmp + "/images/", "--disparity_dir", tmp + "/disparities/", "--output_dir", tmp + "/output/",
            "--orb_n_features", "700"]


@pytest.mark.gpu
def test_feature_poses_runs(tmp_path):
    tmp = str(tmp_path)
    _write_dataset(tmp)
    ply = tmp + "/output/cloud.ply"
    rc, out = _run(_base(tmp))
    assert rc == 0 and "pose chain" not in out, out
    plain = open(ply, "rb").read()
    # no frame is nearby: every frame is an anchor with its recorded pose, the cloud is the plain run's
    rc, out = _run(_base(tmp) + ["--feature_poses", "--dist_nearby", "0"])
    assert rc == 0, out
    assert [(m[0], m[1], m[7]) for m in STATUS.findall(out)] == [("1248", "ANCHOR", "Accepted"), ("1249", "ANCHOR", "Accepted")], out
    assert "Adding Point Cloud number/points: 2 of 2 frames" in out
    assert open(ply, "rb").read() == plain
    # frames within 50 m: one status line per frame, and the cloud is made of the accepted ones
    lines = {}
    for extra in ([], ["--seq_len", "1"]):  # one cycle; one frame per cycle (the second call's history is the first frame)
        rc, out = _run(_base(tmp) + ["--feature_poses", "--dist_nearby", "50"] + extra)
        assert rc == 0, out
        st = STATUS.findall(out)
        assert [m[0] for m in st] == ["1248", "1249"], out
        assert st[0][1] == "ANCHOR" and st[1][1] != "ANCHOR" and (st[1][2], st[1][3]) == ("1", "1")
        assert all((m[1] in ("ANCHOR", "MATCHED")) == (m[7] == "Accepted") for m in st)
        kept = sum(int(n) for n in re.findall(r"Adding Point Cloud number/points: (\d+) of \d+ frames", out))
        assert kept == sum(m[7] == "Accepted" for m in st)
        assert len(_read_ply(ply)) > 0
        lines[len(extra)] = st
    assert lines[0] == lines[2]  # the chain does not depend on the split into cycles
    rc, out = _run(_base(tmp) + ["--feature_poses", "--dist_nearby", "50", "--chain_min_matches", "100000"])
    st = STATUS.findall(out)
    assert rc == 0 and (st[1][1], st[1][7]) == ("TOO_FEW", "Rejected") and "points: 1 of 2 frames" in out, out
    rc, out = _run(_base(tmp) + ["--feature_poses", "--range_width", "0"])
    assert rc != 0 and "range_width" in out


@pytest.mark.gpu
def test_feature_poses_refused_combinations(tmp_path):
    tmp = str(tmp_path)
    _write_dataset(tmp)
    for extra in (["--gpus", "2"], ["--partitioned_merge"], ["--reference_fanout"]):
        rc, out = _run(_base(tmp) + ["--feature_poses"] + extra)
        assert rc != 0 and "--feature_poses is not available" in out, out
