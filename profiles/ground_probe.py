"""Cost of the ground filter (o3dr_ground_filter; DESIGN.md "Ground filter").

Two workloads, inputs in HBM, device tensors in and out, the box from one o3dr_raster_extent call:
  map        BASELINE configs[1]'s frames (synthetic 1280x720, dense, voxel 0.05, outlier removal off): 200 frames into
             cloud_big, merged into the map (o3dr_finalize), filtered at the map's voxel size with the default schedule;
  synthetic  a 4096 x 4096 raster at full occupancy (one point per cell), the default schedule, and one-iteration
             schedules at radius 1 and at radius 128: their ratio says how the cost of an iteration grows with the window.
Measured: the median of 7 calls after one warm-up call, bracketed by HIP events on the context's stream (torch's current
stream; the call synchronises), and per kernel group - the winner, the iterations, the fill, the point pass - the
library's own event brackets (o3dr_profile_enable) averaged over the same calls.  Every row carries the groups'
compulsory bytes, from n (points), C (cells) and K (iterations), and the time they would take at the device copy rate
measured here (a 256 MiB device-to-device copy, bytes read + written).

    python profiles/ground_probe.py [--frames 200] [--side 4096] [--out profiles/ground_probe.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def compulsory_bytes(n, cells, iters, ground_cells, fill_radius):
    """bytes every group must move: n points of 16 bytes, C cells, K iterations"""
    b = {
        # the words' memset, the cloud and one 8-byte atomic (read + write) per point, the words in, Z and the state out
        "winner": 8 * cells + 32 * n + (8 + 4 + 1) * cells + 16 * min(n, cells),
        # per iteration: Z and the state in, the state out, two fp32 intermediates written and read once each
        "iterations": iters * (4 + 1 + 1 + 2 * (4 + 4)) * cells,
        # the states in, the words out and in, the ground points gathered, the DTM out (and the column offsets out and in)
        "fill": (1 + 8 + 8 + 4) * cells + 16 * ground_cells + (2 * cells if fill_radius else 0),
        # the cloud in, the state and the DTM gathered, mask and height out
        "points": (16 + 1 + 4 + 1 + 4) * n,
    }
    return b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--side", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    import online_3d_reconstruction_amd as o3dr
    from online_3d_reconstruction_amd import _lib as L, synth

    stream = torch.cuda.current_stream()
    vs = 0.05
    ctx = o3dr.Context(0, Q=synth.camera_Q(), params=o3dr.Params(jump_pixels=1, voxel_size=vs, sor_enable=False))
    ctx.set_stream(stream)
    groups = {"winner": L.K_GROUND_WINNER, "iterations": L.K_GROUND_ITER, "fill": L.K_GROUND_FILL, "points": L.K_GROUND_POINTS}
    for k in groups.values():
        ctx.profileEnable(k)

    def timed(fn, calls):
        fn()  # warm-up (scratch grows once)
        ctx.profileReset()
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
    del a, b
    res = {"device": ctx.device_info()[0], "device_copy_GBps": round(copy_rate / 1e9, 1), "calls": args.calls}

    def row(name, pts, cell, box, **kw):
        n = int(pts.shape[0])
        ms, out = timed(lambda: ctx.groundFilter(pts, cell, bounds=box, return_height=True, return_dtm=True, return_info=True, **kw), args.calls)
        info = out[-1]
        group_ms = {g: round(ctx.profileRead(k)[0] / args.calls, 4) for g, k in groups.items()}
        byt = compulsory_bytes(n, box[2] * box[3], info.n_iterations, info.n_ground_cells, kw.get("fill_radius", 0))
        return {"workload": name, "points": n, "cell_size": cell, "box": list(box), "cells": box[2] * box[3], "params": kw,
                "radii": [int(r) for r in o3dr.groundSchedule(cell, **{k: v for k, v in kw.items() if k != "fill_radius"})[0]],
                "call_ms": round(ms, 3), "group_ms": group_ms, "compulsory_bytes": byt,
                "ms_at_copy_rate": {g: round(v / copy_rate * 1e3, 4) for g, v in byt.items()},
                "n_ground_cells": info.n_ground_cells, "n_removed": list(info.n_removed), "n_ground_points": info.n_ground_points,
                "n_dtm_filled": info.n_dtm_filled}

    rows = []
    if args.frames > 0:
        disp, bgr = synth.make_frames(0, args.frames)
        poses = synth.make_poses(0, args.frames)
        ctx.accumulateFrames(torch.from_numpy(disp).cuda(), torch.from_numpy(bgr).cuda(), torch.from_numpy(poses).cuda())
        mp = ctx.finalize(device=torch.device("cuda", 0))
        mp = mp if torch.is_tensor(mp) else torch.from_numpy(np.ascontiguousarray(mp).view(np.int32).reshape(-1, 4)).cuda()
        mp = mp.contiguous()
        box = ctx.rasterExtent(mp, vs)
        rows.append(row("map", mp, vs, box))
        rows.append(row("map, fill_radius 8", mp, vs, box, fill_radius=8))
        ctx.cloudBigReset()
        del mp
    if args.side > 0:
        S = args.side
        g = torch.arange(S, device="cuda", dtype=torch.float32)
        x = ((g + 0.5) * vs).repeat(S)
        y = ((g + 0.5) * vs).repeat_interleave(S)
        z = 0.5 * torch.sin(x * 0.3) * torch.cos(y * 0.2) + 0.01 * torch.rand(S * S, device="cuda")
        z = torch.where(((x * 0.7).floor() % 9 == 0) & ((y * 0.7).floor() % 7 == 0), z + 3.0, z)  # blocks 1.4 m wide on a 12.9 x 10 m grid
        pts = torch.stack([x, y, z, torch.zeros_like(x)], 1).view(torch.int32).contiguous()
        del x, y, z, g
        torch.cuda.synchronize()  # (torch's default stream is passed as "the context's own": the cloud must be there)
        box = ctx.rasterExtent(pts, vs)
        assert box[2] * box[3] == S * S, box
        rows.append(row("synthetic, default schedule", pts, vs, box))
        r1 = row("synthetic, one iteration, radius 1", pts, vs, box, max_window_radius=1)
        r128 = row("synthetic, one iteration, radius 128", pts, vs, box, max_window_radius=128, window_base=128, exponential=False)
        rows += [r1, r128]
        res["iteration_ms_radius_128_over_radius_1"] = round(r128["group_ms"]["iterations"] / r1["group_ms"]["iterations"], 3)
    res["rows"] = rows
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
