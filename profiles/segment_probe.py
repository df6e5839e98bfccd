"""Cost of the image segmentation (o3dr_segment_image; DESIGN.md "Image segmentation").

Synthetic 1280x720 B G R images in HBM: blocks of a few colours (a real border every 40 to 60 pixels) under +-8 levels of
noise, so that superpixels split into components and some of them are merged.  Defaults (step 16, compactness 20, 5
iterations, min_size 64), device tensors in and out; 1 frame and 16 frames per call.  Measured after one warm-up call: ms per
call (HIP events on torch's current stream = the context's stream; the call synchronises), the median of --reps, and the two
kernel groups' times from the library's own profile hooks in a further call.  Each group's compulsory bytes are set against
the float4 copy rate of the MI355X (6.29 TB/s).  Prints one JSON line (and writes it with --out).

    python profiles/segment_probe.py [--reps 7] [--out profiles/out/segment_probe.json]
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
STEP, COMPACTNESS, ITERATIONS = 16, 20, 5


def make_frames(F, rows=720, cols=1280, seed=0):
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:rows, 0:cols]
    out = np.empty((F, rows, cols, 3), np.uint8)
    for f in range(F):
        cell = ((y // (40 + f)) * 7 + (x // (60 - f)) * 3) % 5
        base = rng.randint(0, 256, (5, 3))[cell]
        out[f] = np.clip(base + rng.randint(-8, 9, (rows, cols, 3)), 0, 255)
    return out


def measure(ctx, L, torch, img, reps):
    stream = torch.cuda.current_stream()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    labels, info = ctx.segmentImage(img, STEP, COMPACTNESS, ITERATIONS, return_info=True)  # warm-up: scratch allocated
    times = []
    for _ in range(reps):
        ev[0].record(stream)
        labels = ctx.segmentImage(img, STEP, COMPACTNESS, ITERATIONS)
        ev[1].record(stream)
        torch.cuda.synchronize()
        times.append(ev[0].elapsed_time(ev[1]))
    ctx.profileReset()
    ctx.profileEnable(-1, True)
    ctx.segmentImage(img, STEP, COMPACTNESS, ITERATIONS)
    ids = (L.K_SEG_ASSIGN, L.K_SEG_LABEL)
    kernel_ms = {L.KERNEL_NAMES[k]: ctx.profileRead(k)[0] for k in ids}
    ctx.profileEnable(-1, False)
    F, rows, cols = (int(v) for v in img.shape[:3])
    n = rows * cols
    # compulsory bytes per pixel.  assign: the image K + 1 times (3 bytes), the raw label and the key's start value out
    # (4 + 8).  label: the local pass reads the raw label and writes label and count (4 + 8), the flatten pass reads both and
    # writes the label (8 + 4), the key pass reads label and raw label (8), the link pass reads the label and writes the flag
    # (8), the chase and the flag pass read the label (4 + 4), the scan reads the flags twice and writes them once (12), the
    # relabel pass reads the label and writes the number (8); what happens at roots alone is not counted.
    bytes_ = {"seg_assign": F * n * (3 * (ITERATIONS + 1) + 12), "seg_label": F * n * (12 + 12 + 8 + 8 + 8 + 12 + 8)}
    share = {k: bytes_[k] / (COPY_TBPS * 1e9) / kernel_ms[k] for k in bytes_ if kernel_ms[k] > 0}
    return {"frames": F, "centres": sum(i.n_centres for i in info), "components": sum(i.n_components for i in info),
            "merged": sum(i.n_merged for i in info), "labels": sum(i.n_labels for i in info),
            "largest": max(i.largest for i in info), "smallest": min(i.smallest for i in info),
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

    img = torch.from_numpy(make_frames(args.frames)).cuda()
    with o3dr.Context(0, stream=torch.cuda.current_stream()) as ctx:
        res = {"device": ctx.device_info()[0], "rows": 720, "cols": 1280, "channels": 3, "step": STEP, "compactness": COMPACTNESS,
               "iterations": ITERATIONS, "min_size": STEP * STEP // 4, "copy_TBps": COPY_TBPS,
               "single_frame": measure(ctx, L, torch, img[:1].contiguous(), args.reps),
               "stack": measure(ctx, L, torch, img, args.reps)}
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
