"""Cost of the disparity filter (o3dr_disparity_filter; DESIGN.md "Disparity filter").

Synthetic 1280x720 uint8 disparity images in HBM: a smooth ramp of levels 60..120 (neighbours differ by at most 1), 2 % of
the pixels rejected (0), and planted speckles - 3 x 3 blocks 40 levels off their surroundings - covering 1 % of the pixels.
Median 3, max_speckle_size 100, max_diff 1, device tensors in and out; 1 frame and 16 frames per call.  Measured after one
warm-up call: ms per call (HIP events on torch's current stream = the context's stream; the call synchronises), the median
of --reps, and the kernels' times from the library's own profile hooks in a further call.  Each kernel group's compulsory
bytes are set against the float4 copy rate of the MI355X (6.29 TB/s).  Prints one JSON line (and writes it with --out).

    python profiles/disparity_filter_probe.py [--reps 7] [--out profiles/out/disparity_filter_probe.json]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_TBPS = 6.29
MEDIAN, SIZE, DIFF = 3, 100, 1
SPECKLE_SHARE, REJECTED_SHARE = 0.01, 0.02


def make_frames(F, rows=720, cols=1280, seed=0):
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:rows, 0:cols]
    out = np.empty((F, rows, cols), np.uint8)
    for f in range(F):
        img = (60 + (x + 2 * y + 37 * f) // 40 % 61).astype(np.uint8)
        img[rng.rand(rows, cols) < REJECTED_SHARE] = 0
        n_blobs = int(SPECKLE_SHARE * rows * cols / 9)
        by, bx = rng.randint(0, rows - 3, n_blobs), rng.randint(0, cols - 3, n_blobs)
        for dy in range(3):
            for dx in range(3):
                img[by + dy, bx + dx] = 180
        out[f] = img
    return out


def measure(ctx, L, torch, disp, reps):
    stream = torch.cuda.current_stream()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    out, info = ctx.filterDisparity(disp, MEDIAN, SIZE, DIFF, return_info=True)  # warm-up: scratch allocated
    times = []
    for _ in range(reps):
        ev[0].record(stream)
        out = ctx.filterDisparity(disp, MEDIAN, SIZE, DIFF)
        ev[1].record(stream)
        torch.cuda.synchronize()
        times.append(ev[0].elapsed_time(ev[1]))
    ctx.profileReset()
    ctx.profileEnable(-1, True)
    ctx.filterDisparity(disp, MEDIAN, SIZE, DIFF)
    ids = (L.K_DISP_MEDIAN, L.K_DISP_LABEL, L.K_DISP_SPECKLE)
    kernel_ms = {L.KERNEL_NAMES[k]: ctx.profileRead(k)[0] for k in ids}
    ctx.profileEnable(-1, False)
    F, rows, cols = disp.shape
    n = rows * cols
    # compulsory bytes per frame.  median: the image in, the image out.  label: the local pass reads the image and writes
    # label and count (1 + 8), the flatten pass reads both and writes the label (8 + 4); the border pass touches one pixel
    # in 64 and one in 16.  speckle: the image, the label and the count at the label in, the image out (1 + 4 + 4 + 1).
    bytes_ = {"disp_median": F * n * 2, "disp_label": F * n * (9 + 12), "disp_speckle": F * n * 10}
    share = {k: bytes_[k] / (COPY_TBPS * 1e9) / kernel_ms[k] for k in bytes_ if kernel_ms[k] > 0}
    return {"frames": F, "removed_fraction": sum(i.n_removed for i in info) / (F * n), "speckles": sum(i.n_speckles for i in info),
            "components": sum(i.n_components for i in info), "kept_fraction": float((out != 0).float().mean()),
            "ms_per_call": statistics.median(times), "ms_per_call_all": times, "kernel_ms": kernel_ms, "compulsory_bytes": bytes_,
            "fraction_of_copy_rate": share}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    import online_3d_reconstruction_amd as o3dr
    from online_3d_reconstruction_amd import _lib as L

    disp = torch.from_numpy(make_frames(args.frames)).cuda()
    with o3dr.Context(0, stream=torch.cuda.current_stream()) as ctx:
        res = {"device": ctx.device_info()[0], "rows": 720, "cols": 1280, "median": MEDIAN, "max_speckle_size": SIZE, "max_diff": DIFF,
               "planted_speckle_share": SPECKLE_SHARE, "rejected_share": REJECTED_SHARE, "copy_TBps": COPY_TBPS,
               "single_frame": measure(ctx, L, torch, disp[:1].contiguous(), args.reps),
               "stack": measure(ctx, L, torch, disp, args.reps)}
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
