"""Cost of moving-least-squares smoothing (o3dr_mls_smooth; DESIGN.md "MLS").

BASELINE configs[1]'s frames (synthetic 1280x720, dense, voxel 0.05, outlier removal off): 200 frames into cloud_big,
merged into the map (o3dr_finalize, 453k points).  Measured, all clouds in HBM, every call after one warm-up call,
bracketed by HIP events on the context's stream (torch's current stream; the calls synchronise), best of --reps:
  grid      o3dr_nearest_neighbors of ONE query into the map: the search grid's build, which o3dr_mls_smooth shares
  map       o3dr_mls_smooth of the map at r = 2 and 3 voxels (0.1, 0.15 m), orders 0 and 2; smooth_ms = call - grid
            (it still holds the non-finite check and its host round trip)
  frame     one dense 720p per-frame cloud (frame 0 through the per-frame voxel grid, cloud_big after one frame) at
            r = 0.1 m, order 2
  cpu       scipy cKDTree on the host (16 worker threads): build over the map and the fixed-radius neighbour counts at the
            same radii - a CPU reference point for the neighbour search alone, NOT PCL and no fit
Prints one JSON line (and writes it with --out).

    python profiles/mls_probe.py [--frames 200] [--reps 3] [--out profiles/r05_mls.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    import online_3d_reconstruction_amd as o3dr
    from online_3d_reconstruction_amd import POINT, synth

    F = args.frames
    disp, bgr = synth.make_frames(0, F)
    poses = synth.make_poses(0, F)
    stream = torch.cuda.current_stream()
    prm = o3dr.Params(jump_pixels=1, voxel_size=0.05, sor_enable=False)
    ctx = o3dr.Context(0, Q=synth.camera_Q(), params=prm)
    ctx.set_stream(stream)
    ctx.accumulateFrames(torch.from_numpy(disp[:1]).cuda(), torch.from_numpy(bgr[:1]).cuda(), torch.from_numpy(poses[:1]).cuda())
    frame = ctx.cloudBigView().clone()
    ctx.cloudBigReset()
    ctx.accumulateFrames(torch.from_numpy(disp).cuda(), torch.from_numpy(bgr).cuda(), torch.from_numpy(poses).cuda())
    mp = ctx.finalize(device=torch.device("cuda", 0))
    mp = mp if torch.is_tensor(mp) else torch.from_numpy(np.ascontiguousarray(mp).view(np.int32).reshape(-1, 4)).cuda()
    mp = mp.contiguous()
    one = mp[:1].contiguous()

    def timed(fn):
        fn()  # warm-up (workspaces grow once)
        best, out = None, None
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            out = fn()
            e1.record(stream)
            e1.synchronize()
            ms = e0.elapsed_time(e1)
            best = ms if best is None else min(best, ms)
        return best, out

    grid_ms, _ = timed(lambda: ctx.nearestNeighbors(one, mp))
    fgrid_ms, _ = timed(lambda: ctx.nearestNeighbors(frame[:1].contiguous(), frame))
    res = {"device": ctx.device_info()[0], "map_points": int(mp.shape[0]), "frame_points": int(frame.shape[0]),
           "grid_build_ms": round(grid_ms, 3)}

    def row(cloud, r, order, g_ms):
        ms, out = timed(lambda: ctx.mlsSmooth(cloud, r, order, return_info=True))
        info = out[-1]
        sm = ms - g_ms
        return {"radius": r, "order": order, "call_ms": round(ms, 3), "smooth_ms": round(sm, 3),
                "points_per_sec": round(cloud.shape[0] / max(sm, 1e-6) * 1e3, 0), "n_poly": info.n_poly, "n_plane": info.n_plane,
                "n_none": info.n_none, "max_neighbors": info.max_neighbors,
                "mean_neighbors": round(float(out[1].view(torch.int32).to(torch.int64).sum().item()) / max(cloud.shape[0], 1), 2)}

    res["map"] = [row(mp, r, o, grid_ms) for r in (0.1, 0.15) for o in (0, 2)]
    res["frame"] = dict(row(frame, 0.1, 2, fgrid_ms), grid_build_ms=round(fgrid_ms, 3))

    from scipy.spatial import cKDTree
    mh = mp.cpu().numpy().view(POINT).reshape(-1)
    xyz = np.stack([mh["x"], mh["y"], mh["z"]], 1).astype(np.float64)
    t0 = time.perf_counter()
    tree = cKDTree(xyz)
    t1 = time.perf_counter()
    cpu = {"note": "host scipy cKDTree (fp64) neighbour counts only, a CPU reference point, not PCL", "build_ms": round((t1 - t0) * 1e3, 1)}
    for r in (0.1, 0.15):
        t2 = time.perf_counter()
        tree.query_ball_point(xyz, r, workers=16, return_length=True)
        cpu[f"ball_counts_r{r}_ms"] = round((time.perf_counter() - t2) * 1e3, 1)
    res["cpu_reference_scipy_ckdtree_16_threads"] = cpu
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
