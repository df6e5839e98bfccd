"""Cost of the multi-view fusion next to the filter's (o3dr_multiview_fuse, o3dr_multiview_filter; DESIGN.md "Multi-view
fusion").

The scene is profiles/multiview_probe.py's: 16 synthetic 1280x720 uint8 disparity images in HBM, views of the flat ground
under the benchmark's lawn-mower track, 2 % of the pixels rejected, k = 4 neighbours, the defaults otherwise, device tensor
in and out.  Both operators are timed in the same run, alternating, after one warm-up call each: ms per call (HIP events on
torch's current stream = the context's stream; the call synchronises), the median of --reps, each with every optional count
image asked for; then each kernel's time from the library's own profile hooks in a further call.  The compulsory bytes -
every frame read once; the filter writes the image and two count images, the fusion a float64 image and three count
images: 7 bytes more per pixel - are set against the float4 copy rate of the MI355X (6.29 TB/s).  Prints one JSON line and
writes it to --out.

    python profiles/multiview_fuse_probe.py [--reps 7] [--out profiles/multiview_fuse_probe.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from multiview_probe import COPY_TBPS, K, REJECTED_SHARE, make_frames  # noqa: E402


def measure(ctx, L, torch, disp, poses, nb, reps):
    stream = torch.cuda.current_stream()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    calls = {"filter": lambda: ctx.multiviewFilter(disp, poses, nb, return_support=True, return_violations=True),
             "fuse": lambda: ctx.multiviewFuse(disp, poses, nb, return_votes=True, return_support=True, return_violations=True)}
    info = ctx.multiviewFuse(disp, poses, nb, return_info=True)[1]  # warm-up: scratch allocated
    ctx.multiviewFilter(disp, poses, nb, return_info=True)
    times = {name: [] for name in calls}
    for _ in range(reps):
        for name, call in calls.items():
            ev[0].record(stream)
            outs = call()
            ev[1].record(stream)
            torch.cuda.synchronize()
            times[name].append(ev[0].elapsed_time(ev[1]))
            del outs
    kernel_ms = {}
    for name, call in calls.items():
        ctx.profileReset()
        ctx.profileEnable(-1, True)
        call()
        kernel_ms[name] = ctx.profileRead(L.K_MULTIVIEW)[0]
        ctx.profileEnable(-1, False)
    F, rows, cols = disp.shape
    n = rows * cols
    bytes_ = {"filter": F * n * (1 + 1 + 2), "fuse": F * n * (1 + 8 + 3)}  # read e, write e + 2 / 8 + 3, e = 1
    res = {"frames": F, "neighbors": K, "pairs": int((nb >= 0).sum()),
           "supports": sum(i.filter.n_support for i in info), "votes": sum(i.n_votes for i in info),
           "votes_dropped": sum(i.n_votes_dropped for i in info), "fused_pixels": sum(i.n_fused for i in info),
           "kept_fraction": sum(i.filter.n_kept for i in info) / max(sum(i.filter.n_valid for i in info), 1)}
    for name in calls:
        ms = statistics.median(times[name])
        res[name] = {"ms_per_call": ms, "ms_per_frame": ms / F, "ms_per_call_all": times[name], "kernel_ms": kernel_ms[name],
                     "compulsory_bytes": bytes_[name],
                     "fraction_of_copy_rate": bytes_[name] / (COPY_TBPS * 1e9) / kernel_ms[name] if kernel_ms[name] > 0 else None}
    res["fuse_over_filter_ms_per_call"] = res["fuse"]["ms_per_call"] / res["filter"]["ms_per_call"]
    res["fuse_over_filter_kernel_ms"] = kernel_ms["fuse"] / kernel_ms["filter"] if kernel_ms["filter"] > 0 else None
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multiview_fuse_probe.json"))
    args = ap.parse_args()
    import torch

    import online_3d_reconstruction_amd as o3dr
    from online_3d_reconstruction_amd import _lib as L
    from online_3d_reconstruction_amd import synth

    Q = synth.camera_Q()
    poses = synth.make_poses(0, args.frames)
    nb = o3dr.nearbyFrames(poses, K)
    disp = torch.from_numpy(make_frames(Q, poses)).cuda()
    with o3dr.Context(0, Q=Q, stream=torch.cuda.current_stream()) as ctx:
        res = {"device": ctx.device_info()[0], "rows": 720, "cols": 1280, "elem_bytes": 1, "rejected_share": REJECTED_SHARE,
               "copy_TBps": COPY_TBPS, "stack": measure(ctx, L, torch, disp, poses, nb, args.reps)}
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
