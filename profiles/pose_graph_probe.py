"""Cost of the pose-graph refinement (o3dr_pose_graph_refine; DESIGN.md "Pose-graph refinement").

The pose chain probe's world (profiles/pose_chain_probe.py: --frames frames of --rows descriptors in HBM, the 8 frames before
within dist_nearby) goes through poseChain once; its poses, statuses and pair list then go through refinePoses.  Measured
after one warm-up call: ms per refinePoses call (HIP events on the context's stream; the call synchronises), the median of
--reps, and the matching, moments and solve kernels' times from the library's own profile hooks in a further call, next to
the chain kernel's time of a profiled poseChain call for context.
Prints one JSON line (and writes it with --out).

    python profiles/pose_graph_probe.py [--frames 200] [--rows 1500] [--reps 7] [--out profiles/out/pose_graph_probe.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--rows", type=int, default=1500)
    ap.add_argument("--landmarks", type=int, default=3000)
    ap.add_argument("--range_width", type=int, default=8)
    ap.add_argument("--gn_iterations", type=int, default=5)
    ap.add_argument("--cg_iterations", type=int, default=32)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    import online_3d_reconstruction_amd as o3dr
    from online_3d_reconstruction_amd import _lib as L
    from pose_chain_probe import make_world

    desc_h, kp3_h, off, prior = make_world(0, args.frames, args.rows, args.landmarks)
    desc, kp3 = torch.from_numpy(desc_h).cuda(), torch.from_numpy(kp3_h).cuda()
    with o3dr.Context(0, stream=torch.cuda.current_stream()) as ctx:
        stream = torch.cuda.current_stream()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ctx.poseChain(desc, off, kp3, prior, range_width=args.range_width)  # warm-up
        ctx.profileReset()
        ctx.profileEnable(-1, True)
        poses, rec, pairs = ctx.poseChain(desc, off, kp3, prior, range_width=args.range_width, return_pairs=True)
        chain_ms = ctx.profileRead(L.K_POSE_CHAIN)[0]
        ctx.profileEnable(-1, False)
        call = lambda: ctx.refinePoses(desc, off, kp3, poses, rec["status"], pairs, gn_iterations=args.gn_iterations,  # noqa: E731
                                       cg_iterations=args.cg_iterations)
        _p, frames, rr = call()  # warm-up: scratch allocated
        times = []
        for _ in range(args.reps):
            ev[0].record(stream)
            call()
            ev[1].record(stream)
            torch.cuda.synchronize()
            times.append(ev[0].elapsed_time(ev[1]))
        ctx.profileReset()
        ctx.profileEnable(-1, True)
        call()
        kernel_ms = {L.KERNEL_NAMES[k]: ctx.profileRead(k)[0] for k in (L.K_MATCH, L.K_GRAPH_MOMENTS, L.K_GRAPH_SOLVE)}
        ctx.profileEnable(-1, False)
        res = {"device": ctx.device_info()[0], "frames": args.frames, "rows_per_frame": args.rows, "pairs": int(len(pairs)),
               "gn_iterations": args.gn_iterations, "cg_iterations": args.cg_iterations, "edges": rr.n_edges, "free": rr.n_free,
               "n_used": rr.n_used, "energy_before": rr.energy_before, "energy_after": rr.energy_after, "grad_before": rr.grad_before,
               "grad_after": rr.grad_after, "last_step": rr.last_step, "flags": rr.flags, "ms_per_call": statistics.median(times),
               "ms_per_call_all": times, "kernel_ms": kernel_ms, "pose_chain_kernel_ms": chain_ms}
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
