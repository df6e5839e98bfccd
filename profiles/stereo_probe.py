"""Cost of stereo disparity (o3dr_stereo_disparity; DESIGN.md "Stereo disparity").

Synthetic 1280x720 B G R pairs in HBM (synth.py frames as the left images, the right ones moved by 40 columns), D = 256,
8 paths, defaults otherwise, device tensors in and out; 1 frame and 16 frames per call.  Measured after one warm-up call:
ms per call (HIP events on torch's current stream = the context's stream; the call synchronises), the median of --reps,
and the kernels' times from the library's own profile hooks in a further call.  Each kernel group's compulsory bytes are
set against the float4 copy rate of the MI355X (6.29 TB/s).  Prints one JSON line (and writes it with --out).

    python profiles/stereo_probe.py [--reps 7] [--out profiles/out/stereo_probe.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_TBPS = 6.29
D, PATHS, SEG = 256, 8, 256


def measure(ctx, L, torch, left, right, reps):
    stream = torch.cuda.current_stream()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    disp = ctx.stereoDisparity(left, right, D, n_paths=PATHS)  # warm-up: scratch allocated
    times = []
    for _ in range(reps):
        ev[0].record(stream)
        disp = ctx.stereoDisparity(left, right, D, n_paths=PATHS)
        ev[1].record(stream)
        torch.cuda.synchronize()
        times.append(ev[0].elapsed_time(ev[1]))
    ctx.profileReset()
    ctx.profileEnable(-1, True)
    ctx.stereoDisparity(left, right, D, n_paths=PATHS)
    ids = (L.K_STEREO_CENSUS, L.K_STEREO_PATHS, L.K_STEREO_WINNER)
    kernel_ms = {L.KERNEL_NAMES[k]: ctx.profileRead(k)[0] for k in ids}
    ctx.profileEnable(-1, False)
    F, rows, cols = left.shape[:3]
    n = rows * cols
    # compulsory bytes per frame.  census: both B G R images in, two 8-byte words per pixel out.  paths: S is stored by the
    # first direction and read, added and stored by the others (2 n D + (PATHS - 1) 4 n D), each direction reads the two
    # census images once.  winner: a wave reads the S columns of its 256 right pixels and the D - 1 after them, writes
    # 5 bytes per pixel; the finish pass reads those and writes the image.
    bytes_ = {"stereo_census": F * n * (6 + 16), "stereo_paths": F * n * (2 * D + (PATHS - 1) * 4 * D + PATHS * 16),
              "stereo_winner": F * (n * 2 * D * (SEG + D - 1) // SEG + n * 11)}
    share = {k: bytes_[k] / (COPY_TBPS * 1e9) / kernel_ms[k] for k in bytes_ if kernel_ms[k] > 0}
    return {"frames": F, "accepted_fraction": float((disp != 0).float().mean()), "ms_per_call": statistics.median(times),
            "ms_per_call_all": times, "kernel_ms": kernel_ms, "compulsory_bytes": bytes_, "fraction_of_copy_rate": share}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    import online_3d_reconstruction_amd as o3dr
    from online_3d_reconstruction_amd import _lib as L
    from online_3d_reconstruction_amd import synth

    F = args.frames
    left = torch.from_numpy(synth.make_frames(0, 8, invalid_frac=0.02)[1]).cuda().repeat((F + 7) // 8, 1, 1, 1)[:F].contiguous()
    right = torch.cat([left[:, :, 40:], left[:, :, -1:].expand(-1, -1, 40, -1)], 2).contiguous()
    with o3dr.Context(0, stream=torch.cuda.current_stream()) as ctx:
        res = {"device": ctx.device_info()[0], "rows": 720, "cols": 1280, "n_disparities": D, "n_paths": PATHS, "copy_TBps": COPY_TBPS,
               "single_frame": measure(ctx, L, torch, left[:1].contiguous(), right[:1].contiguous(), args.reps),
               "stack": measure(ctx, L, torch, left, right, args.reps)}
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
