"""Cost of the exact nearest-neighbour search and of ICP (o3dr_nearest_neighbors, o3dr_icp_align; DESIGN.md "ICP").

BASELINE configs[1]'s frames (synthetic 1280x720, dense, voxel 0.05, outlier removal off): 200 frames into cloud_big (the
raw cloud: 98M per-frame voxels), merged into the map (o3dr_finalize, 453k points).  Measured, all clouds in HBM, every call after
one warm-up call, bracketed by HIP events on the context's stream (torch's current stream; the calls synchronise):
  grid      o3dr_nearest_neighbors of ONE query into the map: the target grid's build (+ one tiny launch)
  nn        o3dr_nearest_neighbors of the map moved by a small rigid transform into the map -> queries per second
            (grid time subtracted)
  icp_a     the map's every 2nd point, moved, aligned to the map (max_iterations 10)
  icp_b     the raw cloud_big aligned to the map, max_correspondence_distance 0.1 m and +inf (max_iterations 5)
  ms per pass = (call - grid) / (iterations + 1): every call makes iterations + 1 nearest-neighbour passes
  cpu       scipy cKDTree on the host (16 worker threads): build over the map, the same queries - a CPU reference point,
            NOT PCL
Prints one JSON line (and writes it with --out).

    python profiles/icp_probe.py [--frames 200] [--reps 3] [--out profiles/r05_icp.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def rigid(rz, t):
    c, s = np.cos(rz), np.sin(rz)
    T = np.eye(4, dtype=np.float32)
    T[:2, :2] = [[c, -s], [s, c]]
    T[:3, 3] = t
    return T


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
    stream = torch.cuda.current_stream()
    ctx = o3dr.Context(0, Q=synth.camera_Q(), params=o3dr.Params(jump_pixels=1, voxel_size=0.05, sor_enable=False))
    ctx.set_stream(stream)
    ctx.accumulateFrames(torch.from_numpy(disp).cuda(), torch.from_numpy(bgr).cuda(), torch.from_numpy(synth.make_poses(0, F)).cuda())
    raw = ctx.cloudBigView().clone()
    mp = ctx.finalize(device=torch.device("cuda", 0))
    mp = mp if torch.is_tensor(mp) else torch.from_numpy(np.ascontiguousarray(mp).view(np.int32).reshape(-1, 4)).cuda()
    mp = mp.contiguous()
    G = rigid(0.01, [0.05, -0.03, 0.02])
    moved = ctx.transformPtCloud(mp, G).contiguous()
    src_a = ctx.transformPtCloud(mp[::2].contiguous(), G).contiguous()
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
    nn_ms, _ = timed(lambda: ctx.nearestNeighbors(moved, mp))
    res = {"device": ctx.device_info()[0], "map_points": int(mp.shape[0]), "raw_points": int(raw.shape[0]),
           "grid_build_ms": round(grid_ms, 3), "nn_map_ms": round(nn_ms, 3),
           "nn_map_queries_per_sec": round(mp.shape[0] / max(nn_ms - grid_ms, 1e-6) * 1e3, 0)}

    def icp_row(src, max_corr, iters):
        ms, r = timed(lambda: ctx.icpAlign(src, mp, max_iterations=iters, max_correspondence_distance=max_corr))
        passes = r.iterations + 1
        per = (ms - grid_ms) / passes
        return {"queries": int(src.shape[0]), "max_correspondence_distance": max_corr, "call_ms": round(ms, 3),
                "iterations": r.iterations, "reason": r.reason_name, "correspondences": r.n_correspondences,
                "fitness": r.fitness, "ms_per_pass": round(per, 3),
                "nn_queries_per_sec": round(src.shape[0] / max(per, 1e-6) * 1e3, 0)}

    res["icp_a_map_subsample"] = icp_row(src_a, float("inf"), 10)
    res["icp_b_raw_corr_0.1"] = icp_row(raw, 0.1, 5)
    res["icp_b_raw_corr_inf"] = icp_row(raw, float("inf"), 5)

    from scipy.spatial import cKDTree
    mh = mp.cpu().numpy().view(POINT).reshape(-1)
    t_xyz = np.stack([mh["x"], mh["y"], mh["z"]], 1).astype(np.float64)
    mv = moved.cpu().numpy().view(POINT).reshape(-1)
    q_xyz = np.stack([mv["x"], mv["y"], mv["z"]], 1).astype(np.float64)
    t0 = time.perf_counter()
    tree = cKDTree(t_xyz)
    t1 = time.perf_counter()
    tree.query(q_xyz, k=1, workers=16)
    t2 = time.perf_counter()
    rh = raw.cpu().numpy().view(POINT).reshape(-1)
    r_xyz = np.stack([rh["x"], rh["y"], rh["z"]], 1).astype(np.float64)
    t3 = time.perf_counter()
    tree.query(r_xyz, k=1, workers=16)
    t4 = time.perf_counter()
    res["cpu_reference_scipy_ckdtree_16_threads"] = {
        "note": "host scipy cKDTree (fp64), a CPU reference point, not PCL", "build_ms": round((t1 - t0) * 1e3, 1),
        "map_queries_ms": round((t2 - t1) * 1e3, 1), "map_queries_per_sec": round(len(q_xyz) / (t2 - t1), 0),
        "raw_queries_ms": round((t4 - t3) * 1e3, 1), "raw_queries_per_sec": round(len(r_xyz) / (t4 - t3), 0)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
