"""Cost of the map raster (o3dr_rasterize_map; DESIGN.md "Map raster").

BASELINE configs[1]'s frames (synthetic 1280x720, dense, voxel 0.05, outlier removal off): 200 frames into cloud_big,
merged into the map (o3dr_finalize).  Measured, the map in HBM, device tensors in and out, the box from one
o3dr_raster_extent call: the median of 7 calls after one warm-up call, bracketed by HIP events on the context's stream
(torch's current stream; the call synchronises), at fill_radius 0, 4 and 32, without and with the shaded relief.
Every row also carries the call's compulsory bytes per kernel, computed from n (points) and C (cells) below, and the time
they would take at the device copy rate measured here (a 256 MiB device-to-device copy, bytes read + written).
The kernels' own times come from a separate run of this script under rocprofv3 --kernel-trace --stats (tracing slows
the host): --kernel-stats <csv> folds that run's kernel_stats file into the JSON line as the average per launch.

    python profiles/raster_probe.py [--frames 200] [--out profiles/raster_probe.json] [--kernel-stats stats.csv]
    rocprofv3 --kernel-trace --stats --output-format csv -d out -- python profiles/raster_probe.py --radii 4
"""
import argparse
import csv
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def compulsory_bytes(n, cells, sourced, R, shade):
    """bytes every pass must move: n points of 16 bytes, C cells; `sourced` cells gather one point"""
    b = {
        "k_cloud_finite": 16 * n,
        "k_cell_range": 16 * n,
        "fill (memset of the cells' words)": 8 * cells,
        "k_raster_winner": 16 * n + 16 * n,  # the cloud, and one 8-byte atomic (read + write) per point
        "k_raster_resolve": 8 * cells + 16 * sourced + (4 + 3) * cells,  # words in, points gathered, height + colour out
    }
    if R > 0:
        b["k_raster_fill_col"] = 8 * cells + cells
        b["k_raster_resolve"] += cells
    if shade:
        b["k_raster_shade"] = 4 * cells + cells
    return b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--radii", default="0,4,32", help="the fill radii to run (one radius under the profiler keeps its averages clean)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-stats", default=None)
    args = ap.parse_args()
    import torch

    import online_3d_reconstruction_amd as o3dr
    from online_3d_reconstruction_amd import synth

    F = args.frames
    disp, bgr = synth.make_frames(0, F)
    poses = synth.make_poses(0, F)
    stream = torch.cuda.current_stream()
    vs = 0.05
    ctx = o3dr.Context(0, Q=synth.camera_Q(), params=o3dr.Params(jump_pixels=1, voxel_size=vs, sor_enable=False))
    ctx.set_stream(stream)
    ctx.accumulateFrames(torch.from_numpy(disp).cuda(), torch.from_numpy(bgr).cuda(), torch.from_numpy(poses).cuda())
    mp = ctx.finalize(device=torch.device("cuda", 0))
    mp = mp if torch.is_tensor(mp) else torch.from_numpy(np.ascontiguousarray(mp).view(np.int32).reshape(-1, 4)).cuda()
    mp = mp.contiguous()
    n = int(mp.shape[0])

    def timed(fn, calls):
        fn()  # warm-up (scratch grows once)
        ms, out = [], None
        for _ in range(calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            out = fn()
            e1.record(stream)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return float(np.median(ms)), out

    a = torch.empty(256 << 20, dtype=torch.uint8, device="cuda")
    b = torch.empty_like(a)
    copy_ms, _ = timed(lambda: b.copy_(a), args.calls)
    copy_rate = 2 * a.numel() / (copy_ms * 1e-3)  # bytes read + written per second
    ext_ms, box = timed(lambda: ctx.rasterExtent(mp, vs), args.calls)
    cells = box[2] * box[3]
    res = {"device": ctx.device_info()[0], "map_points": n, "cell_size": vs, "box": list(box), "cells": cells,
           "device_copy_GBps": round(copy_rate / 1e9, 1), "extent_call_ms": round(ext_ms, 3), "calls": args.calls}
    rows = []
    for R in [int(r) for r in args.radii.split(",")]:
        for shade in (False, True):
            ms, out = timed(lambda: ctx.rasterizeMap(mp, vs, bounds=box, fill_radius=R, light=(-1.0, 1.0, 1.0) if shade else None,
                                                     return_info=True), args.calls)
            info = out[-1]
            byt = compulsory_bytes(n, cells, info.n_occupied + info.n_filled, R, shade)
            total = sum(byt.values())
            rows.append({"fill_radius": R, "shade": shade, "call_ms": round(ms, 3), "compulsory_bytes": byt,
                         "compulsory_bytes_total": total, "ms_at_copy_rate": round(total / copy_rate * 1e3, 4),
                         "n_occupied": info.n_occupied, "n_shadowed": info.n_shadowed, "n_filled": info.n_filled, "n_empty": info.n_empty})
    res["map"] = rows
    if args.kernel_stats:
        with open(args.kernel_stats) as f:
            stats = {r["Name"].split("(")[0].replace("o3dr::", "").replace("void ", ""): r for r in csv.DictReader(f)}
        keep = ("k_raster", "k_cell_range", "k_cloud_finite", "k_fold4_u32", "fill")
        res["kernel_stats_note"] = "rocprofv3 --kernel-trace --stats of `raster_probe.py --radii 4` (both shade settings, warm-up included)"
        res["kernel_avg_us"] = {k: {"calls": int(r["Calls"]), "avg_us": round(float(r["AverageNs"]) / 1e3, 2),
                                    "min_us": round(float(r["MinNs"]) / 1e3, 2), "max_us": round(float(r["MaxNs"]) / 1e3, 2)}
                                for k, r in stats.items() if any(s in k for s in keep)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
