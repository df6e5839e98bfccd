"""The image-stack layout contract (online_3d_reconstruction_amd/csrc/o3dr_image_stack.h) on the CPU: a stand-alone program,
tests/image_stack_host.cpp, asserts the byte extent against the formula written out by hand, every shared rejection's text,
the overlap test, the frames-per-group rule and that an extent beyond int64 is reported rather than computed.  It is built
with AddressSanitizer and UBSan (any report is fatal) and run as a child process: the only test of the overflow rejection,
which no GPU test may exercise."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_image_stack_header_under_sanitizers(tmp_path):
    exe = str(tmp_path / "image_stack_host")
    build = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-I", os.path.join(ROOT, "online_3d_reconstruction_amd", "csrc"), os.path.join(ROOT, "tests", "image_stack_host.cpp"),
                            "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip() == "image stack: ok"
