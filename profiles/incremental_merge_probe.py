"""Cost of o3dr_finalize_incremental against o3dr_finalize over a growing flight (DESIGN.md "Incremental merge").

BASELINE configs[1]'s frames (synthetic 1280x720, dense, voxel 0.05, outlier removal off), 10 steps of 200 frames into one
cloud_big.  After every step: o3dr_finalize, then o3dr_finalize_incremental (the call that folds the step's points), then
the two once more (the incremental one with nothing appended), every call bracketed by HIP events on the context's stream
(torch's current stream), outputs in HBM sized for the whole cloud.  Prints one JSON line.

    python profiles/incremental_merge_probe.py [--steps 10] [--frames 200] [--idle-reps 20]
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
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--idle-reps", type=int, default=20)
    args = ap.parse_args()
    import torch

    import online_3d_reconstruction_amd as o3dr
    from online_3d_reconstruction_amd import _lib as L
    from online_3d_reconstruction_amd import synth

    F = args.frames
    disp, bgr = synth.make_frames(0, F)
    d, c = torch.from_numpy(disp).cuda(), torch.from_numpy(bgr).cuda()
    stream = torch.cuda.current_stream()
    ctx = o3dr.Context(0, Q=synth.camera_Q(), params=o3dr.Params(jump_pixels=1, voxel_size=0.05, sor_enable=False))
    ctx.set_stream(stream)
    lib, h = ctx._lib, ctx._h
    cap = 0
    out = None

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        r = fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1), r

    def call(name):
        n, st = C.c_int64(0), C.c_uint32(0)
        L.check(getattr(lib, name)(h, C.c_void_p(out.data_ptr()), cap, C.byref(n), C.byref(st), L.MEM_DEVICE))
        return n.value

    rows = []
    for k in range(args.steps):
        ctx.accumulateFrames(d, c, torch.from_numpy(synth.make_poses(k * F, F)).cuda())
        n_big = ctx.cloudBigSize()[0]
        if n_big > cap:
            cap = n_big
            out = torch.empty((cap, 4), dtype=torch.int32, device="cuda")
        t_fin, m_fin = timed(lambda: call("o3dr_finalize"))
        t_inc, m_inc = timed(lambda: call("o3dr_finalize_incremental"))
        s = ctx.finalizeIncrementalStats()
        t_fin2, _ = timed(lambda: call("o3dr_finalize"))
        idle = [timed(lambda: call("o3dr_finalize_incremental"))[0] for _ in range(args.idle_reps)]
        assert m_fin == m_inc and s["fallback"] == 0 and s["points_folded"] > 0
        rows.append({"step": k + 1, "cloud_big_points": n_big, "cells": s["cells"], "groups": s["groups"],
                     "state_bytes": s["state_bytes"], "state_bytes_per_cell": round(s["state_bytes"] / max(s["cells"], 1), 1),
                     "points_folded": s["points_folded"], "finalize_ms": [round(t_fin, 4), round(t_fin2, 4)],
                     "incremental_ms": round(t_inc, 4), "incremental_nothing_appended_ms_median": round(float(np.median(idle)), 4),
                     "incremental_nothing_appended_ms_min": round(float(np.min(idle)), 4)})
    # bit-identity of the last step, once more through the Python layer
    a = ctx.finalizeIncremental(device="cuda")
    b = ctx.finalize(device="cuda")
    same = bool(a.shape == b.shape and torch.equal(a, b))
    name, cus, _ = ctx.device_info()
    ctx.close()
    fin1 = float(np.mean(rows[0]["finalize_ms"]))
    res = {"probe": "incremental_merge", "device": name, "cus": cus, "frames_per_step": F, "steps": args.steps,
           "config": "BASELINE configs[1] frames: synthetic 1280x720, jump_pixels 1, voxel 0.05, sor off",
           "last_step_equal_to_finalize": same,
           "step1_incremental_over_finalize": round(rows[0]["incremental_ms"] / fin1, 3),
           "last_over_step1_incremental": round(rows[-1]["incremental_ms"] / rows[0]["incremental_ms"], 3),
           "last_over_step1_finalize": round(float(np.mean(rows[-1]["finalize_ms"])) / fin1, 3),
           "rows": rows}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
