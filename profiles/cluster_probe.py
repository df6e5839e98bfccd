"""Cost of Euclidean clustering (o3dr_cluster_euclidean; DESIGN.md "Euclidean clustering").

Two workloads, inputs in HBM, device tensors in and out:
  map    BASELINE configs[1]'s frames (synthetic 1280x720, dense, voxel 0.05, outlier removal off): 200 frames into
         cloud_big, merged into the map (o3dr_finalize), clustered at a tolerance of two voxels;
  dense  about a million points uniform in a cube, at the tolerance that gives a point about 30 neighbours.
On the same cloud and radius, in the same run, mlsSmooth(order 0): its pass 1 is the same radius walk over the same grid
without a union-find, so the ratio of the link kernel to the MLS kernel says what the union-find costs on top of the
search.
Measured: the median of 7 calls after one warm-up call, bracketed by HIP events on the context's stream (torch's current
stream; the calls synchronise), and per kernel group - link, number, records - the library's own event brackets
(o3dr_profile_enable) averaged over the same calls; MLS's kernel and the grid build share the `other` bracket, which is
read for each operator on its own.

    python profiles/cluster_probe.py [--frames 200] [--dense 1000000] [--out profiles/cluster_probe.json]
"""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--dense", type=int, default=1000000)
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
    groups = {"link": L.K_CLUSTER_LINK, "number": L.K_CLUSTER_NUMBER, "records": L.K_CLUSTER_RECORDS, "other": L.K_OTHER}
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

    res = {"device": ctx.device_info()[0], "calls": args.calls}

    def row(name, pts, tol):
        n = int(pts.shape[0])
        ms, out = timed(lambda: ctx.clusterCloud(pts, tol, return_clusters=True, return_raw=True, return_sizes=True, return_indices=True,
                                                 return_info=True), args.calls)
        info = out[-1]
        group_ms = {g: round(ctx.profileRead(k)[0] / args.calls, 4) for g, k in groups.items()}
        only_ms, _ = timed(lambda: ctx.clusterCloud(pts, tol), args.calls)
        mls_ms, mls = timed(lambda: ctx.mlsSmooth(pts, tol, 0, return_info=True), args.calls)
        mls_other = round(ctx.profileRead(L.K_OTHER)[0] / args.calls, 4)
        # `other` holds the finite check, the box and the grid build in both operators (once more in the clustering: the box
        # before the grid), and MLS's one kernel on top
        mls_kernel = round(mls_other - group_ms["other"], 4)
        return {"workload": name, "points": n, "tolerance": tol, "call_ms": round(ms, 3), "labels_only_call_ms": round(only_ms, 3),
                "group_ms": group_ms, "pairs_per_point": round(info.n_pairs / max(n, 1), 2), "n_components": info.n_components,
                "largest": info.largest, "n_pairs": info.n_pairs, "mls_order0_call_ms": round(mls_ms, 3), "mls_other_ms": mls_other,
                "mls_kernel_ms_estimate": mls_kernel, "mls_max_neighbors": mls[-1].max_neighbors,
                "link_over_mls_kernel": round(group_ms["link"] / mls_kernel, 3) if mls_kernel > 0 else None,
                "call_over_mls_call": round(ms / mls_ms, 3)}

    rows = []
    if args.frames > 0:
        disp, bgr = synth.make_frames(0, args.frames)
        poses = synth.make_poses(0, args.frames)
        ctx.accumulateFrames(torch.from_numpy(disp).cuda(), torch.from_numpy(bgr).cuda(), torch.from_numpy(poses).cuda())
        mp = ctx.finalize(device=torch.device("cuda", 0))
        mp = mp if torch.is_tensor(mp) else torch.from_numpy(np.ascontiguousarray(mp).view(np.int32).reshape(-1, 4)).cuda()
        mp = mp.contiguous()
        rows.append(row("map, tolerance 2 voxels", mp, 2 * vs))
        ctx.cloudBigReset()
        del mp
    if args.dense > 0:
        n, side = args.dense, 10.0
        tol = (30.0 / (4.0 / 3.0 * math.pi * n / side ** 3)) ** (1.0 / 3.0)  # 30 neighbours in the ball at this density
        g = torch.Generator(device="cuda").manual_seed(1)
        xyz = torch.rand((n, 3), device="cuda", generator=g) * side
        pts = torch.cat([xyz, torch.zeros((n, 1), device="cuda")], 1).view(torch.int32).contiguous()
        del xyz
        torch.cuda.synchronize()  # (torch's default stream is passed as "the context's own": the cloud must be there)
        rows.append(row("dense cube, about 30 neighbours", pts, round(tol, 4)))
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
