"""Cost of the plane-fitted disparity (o3dr_plane_fit_disparity; DESIGN.md "Plane-fitted disparity").

A stack of --frames synthetic 1280x720 frames in HBM with about --labels labels per frame (a block grid), device tensors
in and out.  Measured after one warm-up call: ms per call (HIP events on torch's current stream = the context's stream;
the call synchronises), best of --reps, and the three kernels' times from the library's own profile hooks in a further
call.  The bytes the two image passes must move - the sums pass reads 1 B of disparity and the label, the evaluate pass
reads them again and writes 8 B - are set against what a plain device copy reaches on the same box.  Prints one JSON line
(and writes it with --out).

    python profiles/plane_disp_probe.py [--frames 200] [--labels 1000] [--label-bytes 2] [--reps 5] [--out profiles/r09_plane_disparity.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--labels", type=int, default=1000)
    ap.add_argument("--label-bytes", type=int, default=2, choices=(1, 2, 4))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    import online_3d_reconstruction_amd as o3dr
    from online_3d_reconstruction_amd import _lib as L
    from online_3d_reconstruction_amd import synth

    rows, cols, F = 720, 1280, args.frames
    side = max(1, int(round((rows * cols / args.labels) ** 0.5)))
    y, x = np.mgrid[0:rows, 0:cols]
    lab = (y // side) * ((cols + side - 1) // side) + x // side
    n_labels = int(lab.max()) + 1
    if args.label_bytes == 1:
        lab, n_labels = lab % 256, min(n_labels, 256)
    ldt = {1: torch.uint8, 2: torch.int16, 4: torch.int32}[args.label_bytes]
    labels = torch.from_numpy(lab.astype(np.int32)).to(ldt).cuda()[None].repeat(F, 1, 1).contiguous()
    disp = torch.from_numpy(synth.make_frames(0, 8, invalid_frac=0.02)[0]).cuda().repeat((F + 7) // 8, 1, 1)[:F].contiguous()
    stream = torch.cuda.current_stream()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    res = {"frames": F, "rows": rows, "cols": cols, "n_labels": n_labels, "label_bytes": args.label_bytes}
    with o3dr.Context(0, stream=stream) as ctx:
        res["device"] = ctx.device_info()[0]
        out = ctx.planeFitDisparity(disp, labels, n_labels=n_labels)  # warm-up: scratch allocated
        times = []
        for _ in range(args.reps):
            ev[0].record(stream)
            out = ctx.planeFitDisparity(disp, labels, n_labels=n_labels)
            ev[1].record(stream)
            torch.cuda.synchronize()
            times.append(ev[0].elapsed_time(ev[1]))
        res["ms_per_call"] = min(times)
        res["ms_per_call_all"] = times
        ctx.profileReset()
        ctx.profileEnable(-1, True)
        ctx.planeFitDisparity(disp, labels, n_labels=n_labels)
        res["kernel_ms"] = {L.KERNEL_NAMES[k]: ctx.profileRead(k)[0] for k in (L.K_PLANE_DISP_SUMS, L.K_PLANE_DISP_FIT, L.K_PLANE_DISP_EVAL)}
        ctx.profileEnable(-1, False)
    # a plain device copy of the output's size on this box: the denominator
    dst = torch.empty_like(out)
    dst.copy_(out)
    ct = []
    for _ in range(args.reps):
        ev[0].record(stream)
        dst.copy_(out)
        ev[1].record(stream)
        torch.cuda.synchronize()
        ct.append(ev[0].elapsed_time(ev[1]))
    copy_gbps = 2 * out.numel() * 8 / (min(ct) * 1e-3) / 1e9
    npix = F * rows * cols
    b_sums, b_eval = npix * (1 + args.label_bytes), npix * (1 + args.label_bytes + 8)
    res["copy_GBps"] = copy_gbps
    res["bytes"] = {"sums_pass": b_sums, "evaluate_pass": b_eval, "per_pixel": (b_sums + b_eval) / npix}
    res["byte_time_ms"] = {"sums_pass": b_sums / copy_gbps / 1e6, "evaluate_pass": b_eval / copy_gbps / 1e6}
    res["fraction_of_copy_rate"] = {
        "sums_pass": res["byte_time_ms"]["sums_pass"] / res["kernel_ms"]["plane_disp_sums"],
        "evaluate_pass": res["byte_time_ms"]["evaluate_pass"] / res["kernel_ms"]["plane_disp_eval"],
        "call": (b_sums + b_eval) / copy_gbps / 1e6 / res["ms_per_call"]}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
