"""Cost of the raster interpolation (o3dr_raster_interpolate; DESIGN.md "Raster interpolation").

Two workloads, inputs in HBM, device tensors in and out:
  map        BASELINE configs[1]'s frames (synthetic 1280x720, dense, voxel 0.05, outlier removal off): 200 frames into
             cloud_big, merged into the map (o3dr_finalize), the ground filter at the map's voxel size with the default
             schedule and fill_radius 0; its DTM (values on the ground cells only) is the raster that is interpolated;
  synthetic  a 4096 x 4096 raster: the ground filter's DTM of a cloud with one point per cell, then half of its cells
             removed at random.
Each at smooth 0 and 2, next to the ground filter's own call on the same raster from the same run.  Measured: the median
of 7 calls after one warm-up call, bracketed by HIP events on the context's stream (torch's current stream; the call
synchronises), and per kernel group - the pulls with the one-workgroup top, the pushes with the outputs - the library's own
event brackets (o3dr_profile_enable) averaged over the same calls.  Every row carries the compulsory bytes - one read and
one write of the raster, and the levels above it (a count and a value per cell) written once and read once - and the
fraction of the device copy rate measured here (a 256 MiB device-to-device copy, bytes read + written) they amount to.

    python profiles/interpolate_probe.py [--frames 200] [--side 4096] [--out profiles/interpolate_probe.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def compulsory_bytes(width, height):
    cells, upper, w, h = width * height, 0, width, height
    while (w, h) != (1, 1):
        w, h = (w + 1) >> 1, (h + 1) >> 1
        upper += w * h
    return 2 * 4 * cells + 2 * 8 * upper


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
    groups = {"pull": L.K_INTERP_PULL, "push": L.K_INTERP_PUSH}
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

    def rows_for(name, raster, ground_ms):
        H, W = (int(v) for v in raster.shape)
        byt = compulsory_bytes(W, H)
        out = []
        for smooth in (0, 2):
            ms, (_, info) = timed(lambda: ctx.interpolateRaster(raster, smooth=smooth, return_info=True), args.calls)
            group_ms = {g: round(ctx.profileRead(k)[0] / args.calls, 4) for g, k in groups.items()}
            at_copy = byt / copy_rate * 1e3
            out.append({"workload": name, "width": W, "height": H, "smooth": smooth, "call_ms": round(ms, 3), "group_ms": group_ms,
                        "ground_filter_call_ms": round(ground_ms, 3), "compulsory_bytes": byt, "ms_at_copy_rate": round(at_copy, 4),
                        "fraction_of_copy_rate": round(at_copy / ms, 3), "n_levels": info.n_levels, "n_data": info.n_data,
                        "n_filled": info.n_filled, "n_by_level": list(info.n_by_level)})
        return out

    rows = []
    if args.frames > 0:
        disp, bgr = synth.make_frames(0, args.frames)
        poses = synth.make_poses(0, args.frames)
        ctx.accumulateFrames(torch.from_numpy(disp).cuda(), torch.from_numpy(bgr).cuda(), torch.from_numpy(poses).cuda())
        mp = ctx.finalize(device=torch.device("cuda", 0))
        mp = mp if torch.is_tensor(mp) else torch.from_numpy(np.ascontiguousarray(mp).view(np.int32).reshape(-1, 4)).cuda()
        mp = mp.contiguous()
        box = ctx.rasterExtent(mp, vs)
        ground_ms, (_, dtm) = timed(lambda: ctx.groundFilter(mp, vs, bounds=box, return_dtm=True), args.calls)
        rows += rows_for(f"map, {int(mp.shape[0])} points", dtm, ground_ms)
        ctx.cloudBigReset()
        del mp, dtm
    if args.side > 0:
        S = args.side
        g = torch.arange(S, device="cuda", dtype=torch.float32)
        x = ((g + 0.5) * vs).repeat(S)
        y = ((g + 0.5) * vs).repeat_interleave(S)
        z = 0.5 * torch.sin(x * 0.3) * torch.cos(y * 0.2) + 0.01 * torch.rand(S * S, device="cuda")
        pts = torch.stack([x, y, z, torch.zeros_like(x)], 1).view(torch.int32).contiguous()
        del x, y, z, g
        torch.cuda.synchronize()  # (torch's default stream is passed as "the context's own": the cloud must be there)
        box = ctx.rasterExtent(pts, vs)
        assert box[2] * box[3] == S * S, box
        ground_ms, (_, dtm) = timed(lambda: ctx.groundFilter(pts, vs, bounds=box, return_dtm=True), args.calls)
        del pts
        dtm = torch.where(torch.rand(S, S, device="cuda") < 0.5, torch.full_like(dtm, float("nan")), dtm).contiguous()
        torch.cuda.synchronize()
        rows += rows_for("synthetic, half the cells removed", dtm, ground_ms)
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
