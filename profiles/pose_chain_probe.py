"""Cost of the pose chain (o3dr_pose_chain; DESIGN.md "Pose chain").

--frames synthetic frames of --rows descriptors each in HBM: --landmarks landmarks with random 256-bit descriptors, every
frame sees a random subset from a pose 0.2 m further along x (so the 8 frames before lie within the default dist_nearby of
2 m), at most 8 flipped bits per view, priors = the true poses plus up to 5 cm per axis.  Measured after one warm-up call:
ms per poseChain call (HIP events on the context's stream; the call synchronises), the median of --reps, and the matching
and chain kernels' times from the library's own profile hooks in a further call.  For comparison the same chain driven
from Python, one frame at a time, through matchDescriptors and estimateRigidTransform (the median of --baseline_reps): the
operators that existed before o3dr_pose_chain, with the gather and the transform of the targets in torch.
Prints one JSON line (and writes it with --out).

    python profiles/pose_chain_probe.py [--frames 200] [--rows 1500] [--reps 7] [--out profiles/out/pose_chain_probe.json]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_world(seed, frames, rows, landmarks, step=0.2):
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (landmarks, 32), dtype=np.uint8)
    pos = np.stack([rng.uniform(-5, 5 + step * frames, landmarks), rng.uniform(-5, 5, landmarks), rng.uniform(3, 10, landmarks)], 1)
    desc = np.empty((frames * rows, 32), np.uint8)
    kp3 = np.zeros((frames * rows, 4), np.float32)
    prior = np.tile(np.eye(4, dtype=np.float32).reshape(16), (frames, 1))
    for f in range(frames):
        v = rng.choice(landmarks, rows, replace=False)
        d = base[v].copy()
        flips = rng.integers(0, 256, (rows, 8))  # (a repeated position flips back: at most 8 bits differ)
        for k in range(8):
            d[np.arange(rows), flips[:, k] >> 3] ^= (1 << (flips[:, k] & 7)).astype(np.uint8)
        c, s = np.cos(0.01 * f), np.sin(0.01 * f)
        T = np.array([[c, 0, s, step * f], [0, 1, 0, 0], [-s, 0, c, 0], [0, 0, 0, 1]])
        inv = np.linalg.inv(T)
        desc[f * rows:(f + 1) * rows] = d
        kp3[f * rows:(f + 1) * rows, :3] = pos[v] @ inv[:3, :3].T + inv[:3, 3]
        T[:3, 3] += rng.uniform(-0.05, 0.05, 3)
        prior[f] = T.astype(np.float32).reshape(16)
    return desc, kp3.view(np.int32), np.arange(frames + 1, dtype=np.int64) * rows, prior


def python_chain(ctx, torch, desc, kp3, off, prior, pairs, min_matches=30):
    """the same chain, one frame at a time, through the operators that existed before (no rms gate)"""
    F = len(off) - 1
    poses = torch.from_numpy(prior.copy()).cuda()
    status = [0] * F
    xyz = kp3.view(torch.float32)[:, :3]
    by_frame = {}
    for q, t in pairs.tolist():
        by_frame.setdefault(q, []).append(t)
    for i in range(F):
        mine = [j for j in by_frame.get(i, []) if status[j] <= 1]
        if i not in by_frame:
            continue
        status[i] = 2
        if not mine:
            continue
        rec, good = ctx.matchDescriptors(desc, off, [(i, j) for j in mine])
        nq = int(off[i + 1] - off[i])
        src = kp3[off[i]:off[i + 1]].repeat(len(mine), 1)
        tgt = torch.zeros_like(src)
        for k, j in enumerate(mine):
            m = poses[j].reshape(4, 4)
            t = xyz[off[j]:off[j + 1]][rec[k * nq:(k + 1) * nq, 0].to(torch.int64).clamp(0, int(off[j + 1] - off[j]) - 1)]
            tgt.view(torch.float32)[k * nq:(k + 1) * nq, :3] = t @ m[:3, :3].T + m[:3, 3]
        fit = ctx.estimateRigidTransform(src.contiguous(), tgt, mask=good)
        if fit.n_used >= min_matches and fit.status == 0:
            status[i] = 1
            poses[i] = torch.from_numpy(fit.T.astype(np.float32).reshape(16)).cuda()
    torch.cuda.synchronize()
    return poses, status


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--rows", type=int, default=1500)
    ap.add_argument("--landmarks", type=int, default=3000)
    ap.add_argument("--range_width", type=int, default=8)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--baseline_reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import time

    import torch

    import online_3d_reconstruction_amd as o3dr
    from online_3d_reconstruction_amd import _lib as L

    desc_h, kp3_h, off, prior = make_world(0, args.frames, args.rows, args.landmarks)
    desc, kp3 = torch.from_numpy(desc_h).cuda(), torch.from_numpy(kp3_h).cuda()
    with o3dr.Context(0, stream=torch.cuda.current_stream()) as ctx:
        stream = torch.cuda.current_stream()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        call = lambda: ctx.poseChain(desc, off, kp3, prior, range_width=args.range_width, return_pairs=True)  # noqa: E731
        poses, rec, pairs = call()  # warm-up: scratch allocated
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
        kernel_ms = {L.KERNEL_NAMES[k]: ctx.profileRead(k)[0] for k in (L.K_MATCH, L.K_POSE_CHAIN)}
        ctx.profileEnable(-1, False)
        base_times = []
        for _ in range(args.baseline_reps + 1):  # (the first one warms up)
            t0 = time.perf_counter()
            bposes, bstatus = python_chain(ctx, torch, desc, kp3, off, prior, pairs)
            base_times.append((time.perf_counter() - t0) * 1e3)
        diff = float((bposes.cpu().numpy().astype(np.float64) - poses.cpu().numpy().reshape(-1, 16)).__abs__().max())
        res = {"device": ctx.device_info()[0], "frames": args.frames, "rows_per_frame": args.rows, "range_width": args.range_width,
               "pairs": int(len(pairs)), "statuses": {L.CHAIN_STATUS_NAMES[s]: int((rec["status"] == s).sum()) for s in range(5)},
               "slots_per_frame_max": int((rec["n_pairs"].astype(np.int64) * args.rows).max()), "n_used_median": float(np.median(rec["n_used"])),
               "ms_per_call": statistics.median(times), "ms_per_call_all": times, "kernel_ms": kernel_ms,
               "chain_us_per_frame": 1e3 * kernel_ms["pose_chain"] / max(args.frames, 1),
               "python_chain_ms": statistics.median(base_times[1:]), "python_chain_ms_all": base_times[1:],
               "python_chain_statuses_equal": bstatus == rec["status"].tolist(), "python_chain_max_pose_diff": diff}
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
