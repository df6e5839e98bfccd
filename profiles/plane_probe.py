"""Cost of RANSAC plane segmentation (o3dr_segment_plane; DESIGN.md "Plane segmentation").

BASELINE configs[1]'s frames (synthetic 1280x720, dense, voxel 0.05, outlier removal off): 200 frames into cloud_big
(98 M points), merged into the map (o3dr_finalize, 453k points).  Measured, all clouds in HBM, every call after one
warm-up call, bracketed by HIP events on the context's stream (torch's current stream; the calls synchronise), best of
--reps:
  map       o3dr_segment_plane of the map, one tile (s = 0), H = 1000, t = 0.05 m
  raw       o3dr_segment_plane of cloud_big through cloudBigView(), 10 m tiles, H = 200, t = 0.05 m
  cpu       the numpy restatement's score step (tests/test_plane_segmentation.py: fp32, chunks of 64 hypotheses) on
            the map for --cpu-hyps hypotheses - a CPU reference point for the scoring alone, numpy and NOT PCL
The plane tests of a call are sum over tiles of (points x H); the model rate counts 7 unfused fp32 operations per test
(3 mul, 3 add, 1 compare) against the 78.6 T op/s of the MI355X's 157.3 TFLOP/s (FMA = 2) vector peak.  The kernel
time of k_plane_score comes from a separate `rocprofv3 --kernel-trace --stats` run of `--map-only`.
Prints one JSON line (and writes it with --out).

    python profiles/plane_probe.py [--frames 200] [--reps 3] [--map-only] [--out profiles/r05_plane.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK_OPS = 157.3e12 / 2  # unfused fp32 operations per second at the vector peak
OPS_PER_TEST = 7


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--map-only", action="store_true")
    ap.add_argument("--cpu-hyps", type=int, default=64)
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
    ctx.accumulateFrames(torch.from_numpy(disp).cuda(), torch.from_numpy(bgr).cuda(), torch.from_numpy(poses).cuda())
    del disp, bgr
    mp = ctx.finalize(device=torch.device("cuda", 0))
    mp = mp if torch.is_tensor(mp) else torch.from_numpy(np.ascontiguousarray(mp).view(np.int32).reshape(-1, 4)).cuda()
    mp = mp.contiguous()

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

    def row(cloud, t, H, s):
        ms, (inl, tiles) = timed(lambda: ctx.segmentPlane(cloud, t, H, s, 0))
        tests = int(tiles["n_points"][tiles["n_points"] >= 3].astype(np.int64).sum()) * H
        return {"points": int(cloud.shape[0]), "tile_size": s, "H": H, "t": t, "tiles": int(len(tiles)), "call_ms": round(ms, 3),
                "plane_tests": tests, "call_tests_per_sec": float("%.4g" % (tests / (ms * 1e-3))),
                "call_fraction_of_fp32_vector_peak": round(tests * OPS_PER_TEST / PEAK_OPS / (ms * 1e-3), 4),
                "inliers": int(tiles["n_inliers"].astype(np.int64).sum()), "refined_tiles": int(tiles["refined"].sum())}

    res = {"device": ctx.device_info()[0], "map": row(mp, 0.05, 1000, 0.0)}
    c0 = ctx.segmentPlane(mp, 0.05, 1000, 0.0, 0)[1]["coeff"][0]
    res["map"]["coeff"] = [float(x) for x in c0]
    if not args.map_only:
        big = ctx.cloudBigView()
        res["raw"] = row(big, 0.05, 200, 10.0)
        del big
        mh = mp.cpu().numpy().view(POINT).reshape(-1)
        xyz = np.stack([mh["x"], mh["y"], mh["z"]], 1).astype(np.float32)
        rng = np.random.default_rng(0)
        planes = np.concatenate([rng.normal(0, 1, (args.cpu_hyps, 3)), rng.normal(0, 5, (args.cpu_hyps, 1))], 1).astype(np.float32)
        planes[:, :3] /= np.linalg.norm(planes[:, :3], axis=1, keepdims=True)
        x, y, z, tf = xyz[:, 0], xyz[:, 1], xyz[:, 2], np.float32(0.05)
        t0 = time.perf_counter()
        for h in range(args.cpu_hyps):
            A, B, Cc, D = planes[h]
            int((np.abs(((A * x + B * y) + Cc * z) + D) < tf).sum())
        sec = time.perf_counter() - t0
        res["cpu_reference_numpy"] = {"note": "numpy fp32 score step of the restatement, one host thread, NOT PCL",
                                      "hypotheses": args.cpu_hyps, "ms": round(sec * 1e3, 1),
                                      "tests_per_sec": float("%.4g" % (len(xyz) * args.cpu_hyps / sec)),
                                      "map_H1000_estimate_ms": round(sec * 1e3 * 1000 / args.cpu_hyps, 0)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
