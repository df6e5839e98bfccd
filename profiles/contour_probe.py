"""Cost of the contour lines (o3dr_raster_contours; DESIGN.md "Contour lines").

Two workloads, inputs in HBM, device tensors in and out:
  map        BASELINE configs[1]'s frames (synthetic 1280x720, dense, voxel 0.05, outlier removal off): 200 frames into
             cloud_big, merged into the map (o3dr_finalize), the ground filter at the map's voxel size with the default
             schedule, its DTM interpolated (groundFilter(interpolate=True)): the 873 x 624 hole-free raster that is
             contoured at an interval of 0.25 m;
  synthetic  a 4096 x 4096 terrain, smooth hills with a little noise, at an interval of 0.05 m.
Measured per workload: the full call (Context.contourRaster with lines and vertices: the count entry point, the
allocation by its bounds, the call itself), the count entry point alone, and interpolateRaster on the same raster from
the same run for scale.  Each is the median of 7 calls after one warm-up call, bracketed by HIP events on the context's
stream (torch's current stream; the calls synchronise).  Every row carries the compulsory bytes - one read of the raster,
one write of the segment records, the line records and the vertices - and the fraction of the device copy rate measured
here (a 256 MiB device-to-device copy, bytes read + written) they amount to.

    python profiles/contour_probe.py [--frames 200] [--side 4096] [--out profiles/contour_probe.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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
    del a, b
    res = {"device": ctx.device_info()[0], "device_copy_GBps": round(copy_rate / 1e9, 1), "calls": args.calls}

    def count_only(raster, interval, origin):
        H, W = (int(v) for v in raster.shape)
        prm = L.ContourParamsStruct(W, H, float(interval), 0.0, vs, int(origin[0]), int(origin[1]))
        n = C.c_int64(0)
        L.check(ctx._lib.o3dr_raster_contours_count(ctx._h, raster.data_ptr(), C.byref(prm), C.byref(n), L.MEM_DEVICE))
        return int(n.value)

    def row_for(name, raster, interval, origin):
        H, W = (int(v) for v in raster.shape)
        ms, (_, _, _, info) = timed(lambda: ctx.contourRaster(raster, interval, 0.0, vs, origin, return_lines=True, return_vertices=True,
                                                              return_info=True), args.calls)
        count_ms, n = timed(lambda: count_only(raster, interval, origin), args.calls)
        assert n == info.n_segments
        interp_ms, _ = timed(lambda: ctx.interpolateRaster(raster), args.calls)
        byt = 4 * W * H + 48 * info.n_segments + 32 * info.n_lines + 16 * info.n_vertices
        at_copy = byt / copy_rate * 1e3
        return {"workload": name, "width": W, "height": H, "interval": interval, "call_ms": round(ms, 3), "count_call_ms": round(count_ms, 3),
                "interpolate_call_ms": round(interp_ms, 3), "compulsory_bytes": byt, "ms_at_copy_rate": round(at_copy, 4),
                "fraction_of_copy_rate": round(at_copy / ms, 3), "rank_rounds": info.n_segments.bit_length(), **info.__dict__}

    rows = []
    if args.frames > 0:
        disp, bgr = synth.make_frames(0, args.frames)
        poses = synth.make_poses(0, args.frames)
        ctx.accumulateFrames(torch.from_numpy(disp).cuda(), torch.from_numpy(bgr).cuda(), torch.from_numpy(poses).cuda())
        mp = ctx.finalize(device=torch.device("cuda", 0))
        mp = mp if torch.is_tensor(mp) else torch.from_numpy(np.ascontiguousarray(mp).view(np.int32).reshape(-1, 4)).cuda()
        mp = mp.contiguous()
        box = ctx.rasterExtent(mp, vs)
        dtm = ctx.groundFilter(mp, vs, bounds=box, return_dtm=True, interpolate=True)[1]
        rows.append(row_for(f"map, {int(mp.shape[0])} points, interpolated DTM", dtm, 0.25, box[:2]))
        ctx.cloudBigReset()
        del mp, dtm
    if args.side > 0:
        S = args.side
        g = (torch.arange(S, device="cuda", dtype=torch.float32) + 0.5) * vs
        z = 0.5 * torch.sin(g[None, :] * 0.3) * torch.cos(g[:, None] * 0.2) + 0.01 * torch.rand(S, S, device="cuda")
        z = z.contiguous()
        torch.cuda.synchronize()  # (torch's default stream is passed as "the context's own": the raster must be there)
        rows.append(row_for("synthetic terrain", z, 0.05, (0, 0)))
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
