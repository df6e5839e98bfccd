"""Cost of Hamming 2-NN descriptor matching (o3dr_match_knn2_hamming; DESIGN.md "Feature matching").

Random 32-byte descriptors, all in HBM (torch CUDA tensors), every call after one warm-up call, bracketed by HIP events on
the context's stream (torch's current stream; the call synchronises), best of --reps:
  single    one 1500 x 1500 pair per call (the reference's per-frame knnMatch size)
  batched   --sets sets of 1500 rows, every set against the next --per-set sets: 1600 pairs, 3.6e9 descriptor pairs
  cpu       the numpy restatement of tests/test_feature_matching.py (XOR + 256-entry popcount table + partition) on
            --cpu-rows query rows against 1500 train rows - a CPU reference point, numpy and NOT OpenCV
The model counts 22 VALU operations per descriptor pair (8 xor, 8 bit counts, 3 adds, the key, min/max/min) against the
78.6 T lane-operations/s of the MI355X's vector peak.  k_match_* kernel times come from a separate
`rocprofv3 --kernel-trace --stats` run of this script.  Prints one JSON line (and writes it with --out).

    python profiles/match_probe.py [--sets 200] [--per-set 8] [--reps 5] [--out profiles/r06_match.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK_LANE_OPS = 157.3e12 / 2  # 32-bit VALU lane operations per second (the fp32 vector peak without FMA)
OPS_PER_PAIR = 22
ROWS = 1500


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", type=int, default=200)
    ap.add_argument("--per-set", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cpu-rows", type=int, default=100)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    import online_3d_reconstruction_amd as o3dr

    rng = np.random.default_rng(0)
    desc = torch.from_numpy(rng.integers(0, 256, (args.sets * ROWS, 32), dtype=np.uint8)).cuda()
    off = np.arange(args.sets + 1, dtype=np.int64) * ROWS
    pairs = np.array([(s, (s + k) % args.sets) for s in range(args.sets) for k in range(1, args.per_set + 1)], np.int32)
    stream = torch.cuda.current_stream()
    ctx = o3dr.Context(0)
    ctx.set_stream(stream)

    def timed(fn):
        fn()  # warm-up (workspaces grow once)
        best = None
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            ms = e0.elapsed_time(e1)
            best = ms if best is None else min(best, ms)
        return best

    def row(prs):
        ms = timed(lambda: ctx.matchDescriptors(desc, off, prs))
        dp = len(prs) * ROWS * ROWS
        return {"pairs": int(len(prs)), "descriptor_pairs": dp, "call_ms": round(ms, 4),
                "pairs_per_sec": float("%.4g" % (len(prs) / (ms * 1e-3))),
                "descriptor_pairs_per_sec": float("%.4g" % (dp / (ms * 1e-3))),
                "call_fraction_of_valu_model": round(dp * OPS_PER_PAIR / PEAK_LANE_OPS / (ms * 1e-3), 4)}

    res = {"device": ctx.device_info()[0], "single": row(pairs[:1]), "batched": row(pairs)}
    res["batched"]["model_ms"] = round(res["batched"]["descriptor_pairs"] * OPS_PER_PAIR / PEAK_LANE_OPS * 1e3, 3)
    q = desc[:args.cpu_rows].cpu().numpy()
    t = desc[ROWS:2 * ROWS].cpu().numpy()
    pop = np.array([bin(i).count("1") for i in range(256)], np.uint32)
    t0 = time.perf_counter()
    d = pop[q[:, None, :] ^ t[None, :, :]].sum(-1, dtype=np.uint64)
    key = (d << np.uint64(32)) | np.arange(ROWS, dtype=np.uint64)[None, :]
    np.sort(np.partition(key, 1, axis=1)[:, :2], axis=1)
    sec = time.perf_counter() - t0
    res["cpu_reference_numpy"] = {"note": "numpy restatement, one host thread, NOT OpenCV", "query_rows": args.cpu_rows,
                                  "train_rows": ROWS, "ms": round(sec * 1e3, 2),
                                  "descriptor_pairs_per_sec": float("%.4g" % (args.cpu_rows * ROWS / sec)),
                                  "single_pair_estimate_ms": round(sec * 1e3 * ROWS / args.cpu_rows, 1)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
