"""Cost of the robust pose chain (o3dr_pose_chain_robust; DESIGN.md "Robust fit").

The world of profiles/pose_chain_probe.py (--frames frames of --rows descriptors in HBM) with --corrupt of every frame's
3-D keypoints replaced by a point 0.5 - 3 m away: the descriptors still match, the 3-D point is wrong.  Measured after one
warm-up call each, the median of --reps (HIP events on the context's stream; the call synchronises): ms per poseChain call
with the filter off - the figure pose_chain_probe.py reports on its uncorrupted world, re-measured here on both worlds -
and on, and the kernels' own times (match, ransac, pose_chain) from the library's profile hooks in a further call of each
kind.  Also: the largest pose error against the truth with and without the filter, and the slots the filter dropped.
Prints one JSON line (and writes it with --out).

    python profiles/ransac_probe.py [--frames 200] [--rows 1500] [--corrupt 0.2] [--threshold 0.05] [--iterations 256]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from pose_chain_probe import make_world  # noqa: E402


def corrupt(kp3_i32, off, share, seed, lo=0.5, hi=3.0):
    rng = np.random.default_rng(seed)
    kp3 = kp3_i32.view(np.float32).copy()
    for f in range(len(off) - 1):
        n = int(off[f + 1] - off[f])
        rows = int(off[f]) + rng.choice(n, int(round(share * n)), replace=False)
        d = rng.normal(size=(len(rows), 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        kp3[rows, :3] = (kp3[rows, :3].astype(np.float64) + d * rng.uniform(lo, hi, (len(rows), 1))).astype(np.float32)
    return kp3.view(np.int32)


def true_poses(frames, step=0.2):
    out = np.zeros((frames, 4, 4))
    for f in range(frames):
        c, s = np.cos(0.01 * f), np.sin(0.01 * f)
        out[f] = [[c, 0, s, step * f], [0, 1, 0, 0], [-s, 0, c, 0], [0, 0, 0, 1]]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--rows", type=int, default=1500)
    ap.add_argument("--landmarks", type=int, default=3000)
    ap.add_argument("--range_width", type=int, default=8)
    ap.add_argument("--corrupt", type=float, default=0.2)
    ap.add_argument("--threshold", type=float, default=0.05)
    ap.add_argument("--iterations", type=int, default=256)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    import online_3d_reconstruction_amd as o3dr
    from online_3d_reconstruction_amd import _lib as L

    desc_h, kp3_h, off, prior = make_world(0, args.frames, args.rows, args.landmarks)
    bad_h = corrupt(kp3_h, off, args.corrupt, 1)
    true = true_poses(args.frames)
    desc, kp3_clean, kp3_bad = torch.from_numpy(desc_h).cuda(), torch.from_numpy(kp3_h).cuda(), torch.from_numpy(bad_h).cuda()

    def truth_error(poses):
        p = poses.cpu().numpy().astype(np.float64).reshape(-1, 4, 4)
        E = p[0] @ np.linalg.inv(true[0])
        return float(np.abs(p - E @ true).max())

    with o3dr.Context(0, stream=torch.cuda.current_stream()) as ctx:
        stream = torch.cuda.current_stream()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        kinds = (L.K_MATCH, L.K_RANSAC, L.K_POSE_CHAIN)

        def measure(kp3, **kw):
            call = lambda: ctx.poseChain(desc, off, kp3, prior, range_width=args.range_width, return_pairs=True, **kw)  # noqa: E731
            out = call()  # warm-up: scratch allocated
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
            kernel_ms = {L.KERNEL_NAMES[k]: ctx.profileRead(k)[0] for k in kinds}
            ctx.profileEnable(-1, False)
            rec = out[1]
            return out, {"ms_per_call": statistics.median(times), "ms_per_call_all": times, "kernel_ms": kernel_ms,
                         "statuses": {L.CHAIN_STATUS_NAMES[s]: int((rec["status"] == s).sum()) for s in range(5)},
                         "n_used_median": float(np.median(rec["n_used"])), "n_used_total": int(rec["n_used"].sum()),
                         "truth_error": truth_error(out[0])}

        rk = dict(ransac_threshold=args.threshold, ransac_iterations=args.iterations, return_ransac=True)
        _, off_clean = measure(kp3_clean)
        (_, rec_off, pairs), off_bad = measure(kp3_bad)
        (_, rec_on, _, rr), on_bad = measure(kp3_bad, **rk)
        _, on_clean = measure(kp3_clean, **rk)
        res = {"device": ctx.device_info()[0], "frames": args.frames, "rows_per_frame": args.rows, "range_width": args.range_width,
               "pairs": int(len(pairs)), "corrupt": args.corrupt, "threshold": args.threshold, "iterations": args.iterations,
               "candidates_per_pair_median": float(np.median(rr["n_candidates"])), "inliers_per_pair_median": float(np.median(rr["n_inliers"])),
               "ransac_statuses": [int((rr["status"] == s).sum()) for s in range(3)],
               "slots_dropped": int(rec_off["n_used"].sum() - rec_on["n_used"].sum()) if (rec_off["status"] == rec_on["status"]).all() else None,
               "clean_off": off_clean, "clean_on": on_clean, "corrupted_off": off_bad, "corrupted_on": on_bad}
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
