"""Cost of the height-field surface mesh (o3dr_mesh_surface; DESIGN.md "Surface mesh").

BASELINE configs[1]'s frames (synthetic 1280x720, dense, voxel 0.05, outlier removal off): 200 frames into cloud_big,
merged into the map (o3dr_finalize, 453k points).  Measured, the map in HBM, every call after one warm-up call,
bracketed by HIP events on the context's stream (torch's current stream; the call synchronises), best of --reps:
  map       o3dr_mesh_surface of the map at cell_size = the map's voxel size, L = inf and L = 3 voxels, without and with
            vertex normals; the counts (shadowed points among them) come from the same call
  host      the same call on a host copy of the map (staging in and out included)
  cpu       tests/test_mesh_surface.py's numpy restatement of the contract on the host, single-threaded: a CPU reference
            point, NOT PCL
The split between the sort and the rest of the call comes from a separate rocprofv3 --kernel-trace --stats run of this
script.  Prints one JSON line (and writes it with --out).

    python profiles/mesh_probe.py [--frames 200] [--reps 3] [--out profiles/r07_mesh.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    import online_3d_reconstruction_amd as o3dr
    from online_3d_reconstruction_amd import POINT, synth

    F = args.frames
    disp, bgr = synth.make_frames(0, F)
    poses = synth.make_poses(0, F)
    stream = torch.cuda.current_stream()
    vs = 0.05
    prm = o3dr.Params(jump_pixels=1, voxel_size=vs, sor_enable=False)
    ctx = o3dr.Context(0, Q=synth.camera_Q(), params=prm)
    ctx.set_stream(stream)
    ctx.accumulateFrames(torch.from_numpy(disp).cuda(), torch.from_numpy(bgr).cuda(), torch.from_numpy(poses).cuda())
    mp = ctx.finalize(device=torch.device("cuda", 0))
    mp = mp if torch.is_tensor(mp) else torch.from_numpy(np.ascontiguousarray(mp).view(np.int32).reshape(-1, 4)).cuda()
    mp = mp.contiguous()
    mh = mp.cpu().numpy().view(POINT).reshape(-1)

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

    res = {"device": ctx.device_info()[0], "map_points": int(mp.shape[0]), "cell_size": vs}
    rows = []
    for L in (float("inf"), 3 * vs):
        for normals in (False, True):
            ms, out = timed(lambda: ctx.meshSurface(mp, vs, L, return_normals=normals, return_info=True))
            info = out[-1]
            rows.append({"max_edge_length": "inf" if L == float("inf") else L, "normals": normals, "call_ms": round(ms, 3),
                         "points_per_sec": round(mp.shape[0] / max(ms, 1e-6) * 1e3, 0), **info.__dict__})
    res["map"] = rows
    ms, _ = timed(lambda: ctx.meshSurface(mh, vs, float("inf"), return_normals=True))
    res["host_memory_call_ms"] = round(ms, 3)
    if not args.no_cpu:
        from test_mesh_surface import mesh_numpy
        xyz = np.stack([mh["x"], mh["y"], mh["z"]], 1).astype(np.float32)
        best = None
        for _ in range(args.reps):
            t0 = time.perf_counter()
            mesh_numpy(xyz, vs, float("inf"), normals=True)
            dt = (time.perf_counter() - t0) * 1e3
            best = dt if best is None else min(best, dt)
        res["cpu_reference_numpy_restatement_ms"] = {"note": "tests/test_mesh_surface.py mesh_numpy, one host thread, with "
                                                     "normals: a CPU reference point, not PCL", "ms": round(best, 1)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
