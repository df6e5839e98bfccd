"""Cost of the multi-view filter (o3dr_multiview_filter; DESIGN.md "Multi-view filter").

Synthetic 1280x720 uint8 disparity images in HBM: 16 views of the flat ground under the benchmark's lawn-mower track
(synth.make_poses, 0.98 m between frames, 22 m up: about a quarter of the image height a frame; the share of the tests
that land inside a neighbour is reported), each
exactly what its pose sees of the plane, rounded to levels, 2 % of the pixels rejected (0).  k = 4 neighbours, the defaults
otherwise, device tensor in and out.  Measured after one warm-up call: ms per call (HIP events on torch's current stream =
the context's stream; the call synchronises), the median of --reps, and the kernel's time from the library's own profile
hooks in a further call.  The compulsory bytes - every frame read once, the image and the two count images written -
are set against the float4 copy rate of the MI355X (6.29 TB/s).  Prints one JSON line (and writes it with --out).

    python profiles/multiview_probe.py [--reps 7] [--out profiles/out/multiview_probe.json]
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
K, REJECTED_SHARE = 4, 0.02


def make_frames(Q, poses, rows=720, cols=1280, seed=0):
    """what each pose sees of the world plane z = 0: d(x, y) = -(p0 x + p1 y + p3) / p2 with p = (T Q)^T (0, 0, 1, 0)"""
    rng = np.random.RandomState(seed)
    x = np.arange(cols, dtype=np.float64)[None, :]
    y = np.arange(rows, dtype=np.float64)[:, None]
    out = np.empty((len(poses), rows, cols), np.uint8)
    for f, T in enumerate(poses):
        p = (T.astype(np.float64) @ Q).T @ np.array([0.0, 0.0, 1.0, 0.0])
        d = np.rint(-(p[0] * x + p[1] * y + p[3]) / p[2])
        img = np.where((d >= 1) & (d <= 255), d, 0).astype(np.uint8)
        img[rng.rand(rows, cols) < REJECTED_SHARE] = 0
        out[f] = img
    return out


def measure(ctx, L, torch, disp, poses, nb, reps):
    stream = torch.cuda.current_stream()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    out, info = ctx.multiviewFilter(disp, poses, nb, return_info=True)  # warm-up: scratch allocated
    times = []
    for _ in range(reps):
        ev[0].record(stream)
        out, sup, vio = ctx.multiviewFilter(disp, poses, nb, return_support=True, return_violations=True)
        ev[1].record(stream)
        torch.cuda.synchronize()
        times.append(ev[0].elapsed_time(ev[1]))
    ctx.profileReset()
    ctx.profileEnable(-1, True)
    ctx.multiviewFilter(disp, poses, nb, return_support=True, return_violations=True)
    kernel_ms = ctx.profileRead(L.K_MULTIVIEW)[0]
    ctx.profileEnable(-1, False)
    F, rows, cols = disp.shape
    n = rows * cols
    bytes_ = F * n * 1 + F * n * (1 + 2)  # read F H W e, write F H W (e + 2), e = 1
    tests = sum(i.n_outside + i.n_hole + i.n_support + i.n_violation + i.n_occluded for i in info)
    ms = statistics.median(times)
    return {"frames": F, "neighbors": K, "pairs": int((nb >= 0).sum()), "tests": tests,
            "inside_fraction": 1.0 - sum(i.n_outside for i in info) / max(tests, 1),
            "kept_fraction": sum(i.n_kept for i in info) / max(sum(i.n_valid for i in info), 1),
            "ms_per_call": ms, "ms_per_frame": ms / F, "ms_per_call_all": times, "kernel_ms": kernel_ms, "compulsory_bytes": bytes_,
            "fraction_of_copy_rate": bytes_ / (COPY_TBPS * 1e9) / kernel_ms if kernel_ms > 0 else None,
            "tests_per_us": tests / (kernel_ms * 1e3) if kernel_ms > 0 else None}


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

    Q = synth.camera_Q()
    poses = synth.make_poses(0, args.frames)
    nb = o3dr.nearbyFrames(poses, K)
    disp = torch.from_numpy(make_frames(Q, poses)).cuda()
    with o3dr.Context(0, Q=Q, stream=torch.cuda.current_stream()) as ctx:
        res = {"device": ctx.device_info()[0], "rows": 720, "cols": 1280, "elem_bytes": 1, "rejected_share": REJECTED_SHARE,
               "copy_TBps": COPY_TBPS, "stack": measure(ctx, L, torch, disp, poses, nb, args.reps)}
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
