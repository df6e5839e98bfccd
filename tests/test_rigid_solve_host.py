"""The shared Kabsch solve (online_3d_reconstruction_amd/csrc/o3dr_rigid_solve.h) on the CPU.  tests/rigid_solve_main.cpp is
built with g++ against the header alone (no HIP header; -ffp-contract=off like the library) and prints, for a fixed list of
records - a generic motion, a pure translation, coplanar pairs with a reflection to correct, rank 1, rank 0, two and three
equal singular values, a NaN moment, n = 3 -, the record it solved and the T and return value it got; it also checks the
column sort against std::sort on all 27 tie patterns.  Every printed T equals tests/rigid_core_reference.py bit for bit.
The second test holds that restatement against numpy's SVD (kabsch_ref) on random motions."""
import os
import struct
import subprocess

import numpy as np
import pytest

import rigid_core_reference as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["generic", "nan_moment", "n3", "translation", "coplanar_reflection", "collinear_rank1", "rank0", "two_equal_singular",
         "two_equal_singular_moved", "three_equal_singular", "three_equal_singular_moved"]
SOLVED = {"generic", "n3", "translation", "coplanar_reflection", "two_equal_singular", "two_equal_singular_moved",
          "three_equal_singular", "three_equal_singular_moved"}


def _doubles(words):
    return np.array([struct.unpack("<d", struct.pack("<Q", int(w, 16)))[0] for w in words], np.float64)


@pytest.fixture(scope="module")
def program_output(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("rigid_solve") / "rigid_solve_main")
    build = subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-I",
                            os.path.join(ROOT, "online_3d_reconstruction_amd", "csrc"), os.path.join(ROOT, "tests", "rigid_solve_main.cpp"),
                            "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    assert build.stderr.strip() == "", build.stderr  # -Wall -Wextra stay silent
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    return run.stdout.splitlines()


def test_solve_equals_the_reference_bit_for_bit(program_output):
    lines = [ln.split() for ln in program_output if ln.startswith("case ")]
    assert [ln[1] for ln in lines] == CASES
    for ln in lines:
        name = ln[1]
        assert ln[2] == "rec" and ln[22] == "ret" and ln[24] == "T" and len(ln) == 37, name
        rec, c0, ret, T = _doubles(ln[3:19]), _doubles(ln[19:22]), int(ln[23]), _doubles(ln[25:37])
        ok, Tref = rc.rigid_solve(rec, c0)
        assert ret == int(ok), name
        assert ret == int(name in SOLVED), name
        assert T.tobytes() == Tref.tobytes(), (name, T, Tref)
        if ret:  # a proper rotation that maps the record's mean src onto its mean tgt
            R = T.reshape(3, 4)[:, :3]
            assert abs(np.linalg.det(R) - 1.0) < 1e-12 and np.abs(R @ R.T - np.eye(3)).max() < 1e-12, name


def test_column_sort_equals_std_sort_and_the_generator(program_output):
    assert "order check: 0 of 27 patterns differ from std::sort" in program_output
    assert f"splitmix64 0 {rc.splitmix64(0):016x}" in program_output
    assert rc.splitmix64(0) == 0xE220A8397B1DCDAF


def test_reference_fit_against_numpy_svd():
    """The restated sums and solve against kabsch_ref (numpy's SVD, mean-centred): another SVD and summation order, so
    the suite's 1e-9.  Largest difference seen over these 40 motions: 2.7e-15 (printed below)."""
    from test_feature_matching import kabsch_ref
    rng = np.random.default_rng(11)
    worst = 0.0
    for k in range(40):
        n = int(rng.integers(3, 700))
        src = rng.uniform(-5, 5, (n, 3)).astype(np.float32)
        axis, ang = rng.normal(size=3), rng.uniform(-np.pi, np.pi)
        axis /= np.linalg.norm(axis)
        K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
        R = np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K
        tgt = (src.astype(np.float64) @ R.T + rng.uniform(-3, 3, 3) + rng.normal(0, 0.01, (n, 3))).astype(np.float32)
        used = rng.random(n) > 0.2
        used[:3] = True
        fold, threads = (rc.fold_strided, rc.RUN) if k % 2 else (rc.fold_chain, rc.CHAIN_THREADS)
        fit = rc.rigid_fit(src, tgt, used, fold, threads)
        assert fit["ok"] and fit["n_used"] == used.sum()
        ref = kabsch_ref(src[used], tgt[used])
        worst = max(worst, float(np.abs(fit["T"].reshape(3, 4) - ref[:3]).max()))
        rms = rc.residual_rms(fit["T"], src, tgt, used, fit["n_used"], fold, threads)
        e = src[used].astype(np.float64) @ ref[:3, :3].T + ref[:3, 3] - tgt[used]
        assert abs(rms - np.sqrt((e * e).sum() / used.sum())) < 1e-9
    print(f"largest |T - kabsch_ref| over 40 motions: {worst:.3g}")
    assert worst < 1e-9
