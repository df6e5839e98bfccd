"""Cost of stereo rectification (o3dr_rectify_maps, o3dr_rectify_remap; DESIGN.md "Stereo rectification").

Synthetic 1280x720 B G R pairs in HBM (synth.py frames as the left images, the right ones moved by 40 columns), a mild
two-camera calibration (radial, tangential and rational terms, a small rotation each), device tensors in and out; both
cameras, 1 frame and 16 frames per call.  Measured after one warm-up call: ms per call (HIP events on torch's current
stream = the context's stream; the call synchronises), the median of --reps, and the kernels' times from the library's own
profile hooks in a further call.  Each kernel's compulsory bytes are set against the float4 copy rate of the MI355X
(6.29 TB/s): the map kernel writes 8 bytes per destination pixel and reads nothing; the remap reads the map once per
launch (8 bytes per destination pixel) and per frame reads about as many image bytes as the rows_out * cols_out * 3 it
writes.  Prints one JSON line (and writes it with --out).

    python profiles/rectify_probe.py [--reps 7] [--out profiles/out/rectify_probe.json]
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
ROWS, COLS = 720, 1280


def cameras():
    K = np.array([[1100.0, 0, 636.5], [0, 1095.0, 352.25], [0, 0, 1]])
    P1 = np.array([[1050.0, 0, 640, 0], [0, 1050, 360, 0], [0, 0, 1, 0]])
    P2 = P1.copy()
    P2[0, 3] = -126.0

    def rot(r):
        r = np.asarray(r, np.float64)
        th = np.linalg.norm(r)
        k = r / th
        Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)
    D = np.array([-0.28, 0.09, 0.0012, -0.0007, -0.011, 0.02, -0.01, 0.003])
    return [(K, D, rot((0.01, -0.015, 0.008)), P1), (K, 0.9 * D, rot((-0.012, 0.01, -0.006)), P2)]


def measure(ctx, L, torch, images, maps, reps):
    """images / maps: one entry per camera"""
    stream = torch.cuda.current_stream()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    out = [ctx.rectify(i, m) for i, m in zip(images, maps)]  # warm-up
    times = []
    for _ in range(reps):
        ev[0].record(stream)
        out = [ctx.rectify(i, m) for i, m in zip(images, maps)]
        ev[1].record(stream)
        torch.cuda.synchronize()
        times.append(ev[0].elapsed_time(ev[1]))
    ctx.profileReset()
    ctx.profileEnable(-1, True)
    out = [ctx.rectify(i, m) for i, m in zip(images, maps)]
    kernel_ms = ctx.profileRead(L.K_RECTIFY_REMAP)[0]
    ctx.profileEnable(-1, False)
    valid = [ctx.rectify(i[:1], m, return_valid=True)[1] for i, m in zip(images, maps)]
    F, n = int(images[0].shape[0]), ROWS * COLS
    bytes_ = len(images) * (n * 8 + F * n * 6)  # per camera: the map once, then 3 bytes read and 3 written per pixel and frame
    del out
    return {"frames": F, "cameras": len(images), "valid_fraction": [float(v.float().mean()) for v in valid],
            "ms_per_call_pair": statistics.median(times), "ms_per_call_pair_all": times, "kernel_ms": {"rectify_remap": kernel_ms},
            "compulsory_bytes": {"rectify_remap": bytes_},
            "fraction_of_copy_rate": {"rectify_remap": bytes_ / (COPY_TBPS * 1e9) / kernel_ms} if kernel_ms > 0 else {}}


def measure_maps(ctx, L, torch, cams, reps):
    stream = torch.cuda.current_stream()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    maps = [ctx.rectifyMaps(*c, (ROWS, COLS), device="cuda:0") for c in cams]  # warm-up
    times = []
    for _ in range(reps):
        ev[0].record(stream)
        maps = [ctx.rectifyMaps(*c, (ROWS, COLS), device="cuda:0") for c in cams]
        ev[1].record(stream)
        torch.cuda.synchronize()
        times.append(ev[0].elapsed_time(ev[1]))
    ctx.profileReset()
    ctx.profileEnable(-1, True)
    maps = [ctx.rectifyMaps(*c, (ROWS, COLS), device="cuda:0") for c in cams]
    kernel_ms = ctx.profileRead(L.K_RECTIFY_MAPS)[0]
    ctx.profileEnable(-1, False)
    bytes_ = len(cams) * ROWS * COLS * 8
    res = {"cameras": len(cams), "ms_per_call_pair": statistics.median(times), "ms_per_call_pair_all": times,
           "kernel_ms": {"rectify_maps": kernel_ms}, "compulsory_bytes": {"rectify_maps": bytes_},
           "fraction_of_copy_rate": {"rectify_maps": bytes_ / (COPY_TBPS * 1e9) / kernel_ms} if kernel_ms > 0 else {}}
    return maps, res


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
        maps, maps_res = measure_maps(ctx, L, torch, cameras(), args.reps)
        res = {"device": ctx.device_info()[0], "rows": ROWS, "cols": COLS, "channels": 3, "copy_TBps": COPY_TBPS, "maps": maps_res,
               "single_frame": measure(ctx, L, torch, [left[:1].contiguous(), right[:1].contiguous()], maps, args.reps),
               "stack": measure(ctx, L, torch, [left, right], maps, args.reps)}
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
