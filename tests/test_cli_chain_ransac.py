"""`--chain_ransac_threshold` of the C++ host layer under `--feature_poses`: o3dr_pose_chain_robust filters every pair's
correspondences and each frame's status line gains the number of slots the filter dropped.  Without the flag the status
lines keep today's format (the pattern of tests/test_cli_feature_poses.py)."""
import re

import pytest

from test_cli_feature_poses import STATUS, _base, _run
from test_cli_pose import _write_dataset

ROBUST = re.compile(r"^(\d+) pose chain: (ANCHOR|MATCHED|TOO_FEW|DEGENERATE|RMS) pairs (\d+)/(\d+) good (\d+) used (\d+) rms (\S+) dropped (\d+)"
                    r"\t(Accepted|Rejected)!$", re.M)


@pytest.mark.gpu
def test_chain_ransac_flags(tmp_path):
    tmp = str(tmp_path)
    _write_dataset(tmp)
    chain = _base(tmp) + ["--feature_poses", "--dist_nearby", "50"]
    rc, out = _run(chain)
    assert rc == 0 and "dropped" not in out, out
    plain = STATUS.findall(out)
    assert [m[0] for m in plain] == ["1248", "1249"] and int(plain[1][5]) > 0, out
    # the other chain flags alone change nothing: the filter is off unless a threshold is given
    rc, out = _run(chain + ["--chain_ransac_iterations", "64", "--chain_ransac_seed", "3"])
    assert rc == 0 and STATUS.findall(out) == plain and not ROBUST.findall(out), out
    dropped = {}
    for thr in ("100", "0.05"):
        rc, out = _run(chain + ["--chain_ransac_threshold", thr, "--chain_ransac_iterations", "128", "--chain_ransac_seed", "3"])
        assert rc == 0 and not STATUS.findall(out), out
        st = ROBUST.findall(out)
        assert [m[0] for m in st] == ["1248", "1249"] and (st[0][1], st[0][7]) == ("ANCHOR", "0"), out
        assert st[1][2:5] == plain[1][2:5]  # pairs and good rows: the matching is the same
        assert int(st[1][5]) + int(st[1][7]) == int(plain[1][5])  # used + dropped = the plain run's used
        dropped[thr] = int(st[1][7])
    # every hypothesis' score grows with the threshold, so the best one's does: a tighter threshold drops no fewer
    assert dropped["0.05"] > dropped["100"] >= 0
    rc, out = _run(chain + ["--chain_ransac_threshold", "0"])
    assert rc != 0 and "threshold" in out
    rc, out = _run(chain + ["--chain_ransac_threshold", "0.05", "--chain_ransac_iterations", "0"])
    assert rc != 0 and "iterations" in out
