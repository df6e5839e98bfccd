"""Cost of ORB feature extraction (o3dr_orb_detect; DESIGN.md "ORB features").

A stack of --frames synthetic 1280x720 B G R frames in HBM (synth.py), default parameters (1500 features, 5 levels at
1.3, threshold 20, edge 31), device tensors in and out.  Measured after one warm-up call: ms per call (HIP events on
torch's current stream = the context's stream; the call synchronises), the median of --reps, and the kernels' times from
the library's own profile hooks in a further call.  The same for a single frame.  Each kernel group's compulsory bytes
are set against the float4 copy rate of the MI355X (6.29 TB/s).  Prints one JSON line (and writes it with --out).

    python profiles/orb_probe.py [--frames 200] [--reps 7] [--out profiles/out/orb_probe.json]
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


def measure(ctx, L, torch, bgr, reps):
    stream = torch.cuda.current_stream()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    out = ctx.findFeatures(bgr)  # warm-up: scratch allocated, table uploaded
    times = []
    for _ in range(reps):
        ev[0].record(stream)
        out = ctx.findFeatures(bgr)
        ev[1].record(stream)
        torch.cuda.synchronize()
        times.append(ev[0].elapsed_time(ev[1]))
    ctx.profileReset()
    ctx.profileEnable(-1, True)
    ctx.findFeatures(bgr)
    ids = (L.K_ORB_PYRAMID, L.K_ORB_FAST, L.K_ORB_CANDIDATES, L.K_ORB_SELECT, L.K_ORB_DESCRIBE)
    kernel_ms = {L.KERNEL_NAMES[k]: ctx.profileRead(k)[0] for k in ids}
    ctx.profileEnable(-1, False)
    F, rows, cols = bgr.shape[:3]
    wh = np.zeros(10, np.int32)
    ctx._lib.o3dr_orb_level_sizes(rows, cols, None, wh.ctypes.data, None)
    pyr = int(sum(int(wh[2 * l]) * int(wh[2 * l + 1]) for l in range(5)))
    n_kp = int(out[3][-1])
    # compulsory bytes per frame: the pyramid reads B G R and each level once and writes each level; the FAST pass reads a
    # level and writes 1 + 2 bytes per pixel; the candidate passes read the score map twice; a keypoint's record is 72 bytes
    bytes_ = {"orb_pyramid": F * (3 * rows * cols + 2 * pyr - rows * cols), "orb_fast": F * 4 * pyr, "orb_candidates": F * 2 * pyr,
              "orb_describe": n_kp * 72}
    share = {k: bytes_[k] / (COPY_TBPS * 1e9) / kernel_ms[k] for k in bytes_ if kernel_ms[k] > 0}
    return {"frames": F, "keypoints": n_kp, "ms_per_call": statistics.median(times), "ms_per_call_all": times, "kernel_ms": kernel_ms,
            "compulsory_bytes": bytes_, "fraction_of_copy_rate": share}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    import online_3d_reconstruction_amd as o3dr
    from online_3d_reconstruction_amd import _lib as L
    from online_3d_reconstruction_amd import synth

    F = args.frames
    bgr = torch.from_numpy(synth.make_frames(0, 8, invalid_frac=0.02)[1]).cuda().repeat((F + 7) // 8, 1, 1, 1)[:F].contiguous()
    with o3dr.Context(0, stream=torch.cuda.current_stream()) as ctx:
        res = {"device": ctx.device_info()[0], "rows": 720, "cols": 1280, "copy_TBps": COPY_TBPS,
               "stack": measure(ctx, L, torch, bgr, args.reps), "single_frame": measure(ctx, L, torch, bgr[:1].contiguous(), args.reps)}
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
