"""Device time of the depth evaluation (planedepth_amd.metrics.eval_depth_errors) on a synthetic Eigen-shaped split.

    python scripts/bench_eval.py [--images 697] [--reps 20] [--host-images 32]

697 GT maps in the Eigen size mix (375x1242, 370x1224, 374x1238, 376x1241) with ~5 % LiDAR-like valid points quantised to
1/256, predictions at 192x640 and 384x1280, mono (median scaling).  Reports, per prediction size: the device time of one
evaluation (HIP events, median of --reps), the bytes it must read (dense GT + prediction) and their rate, against the
device-to-device copy rate measured in the same run (torch clone of the GT buffer: read + write); the host-to-device copy
of the packed GT, timed on its own; and the numpy restatement of tests/test_depth_eval.py on the host for --host-images
images, scaled to the split.  One JSON line at the end.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SIZES = [(375, 1242), (370, 1224), (374, 1238), (376, 1241)]


def eigen_split(n, seed=0):
    rng = np.random.default_rng(seed)
    gts = []
    for i in range(n):
        H, W = SIZES[i % 4]
        g = np.zeros((H, W), np.float32)
        keep = rng.random((H, W), dtype=np.float32) < 0.05
        g[keep] = (np.round(rng.uniform(2, 85, int(keep.sum())) * 256) / 256).astype(np.float32)
        gts.append(g)
    return gts


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(np.min(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=697)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-images", type=int, default=32)
    args = ap.parse_args()
    import __graft_entry__
    __graft_entry__.build()
    from planedepth_amd import metrics
    gts = eigen_split(args.images)
    gt_bytes = sum(g.nbytes for g in gts)
    t0 = time.perf_counter()
    packed = metrics.pack_gt(gts, "eigen_raw")    # host packing into pinned memory + non-blocking copy
    torch.cuda.synchronize()
    pack_s = time.perf_counter() - t0
    host = packed.data.cpu().pin_memory()
    h2d_ms, _ = timed(lambda: packed.data.copy_(host, non_blocking=True), 5)
    copy_ms, _ = timed(lambda: packed.data.clone(), args.reps)
    copy_gbs = 2 * packed.data.numel() * 4 / copy_ms / 1e6
    result = {"images": args.images, "gt_bytes": gt_bytes, "d2d_copy_GBps": round(copy_gbs, 1),
              "gt_read_floor_ms": round(gt_bytes / (copy_gbs * 1e6), 4), "h2d_gt_ms": round(h2d_ms, 3),
              "host_pack_and_copy_s": round(pack_s, 3)}
    g = torch.Generator(device="cuda").manual_seed(1)
    for h, w in ((192, 640), (384, 1280)):
        pred = torch.rand(args.images, h, w, device="cuda", generator=g) * 59 + 1
        fn = lambda: metrics.eval_depth_errors(pred, packed, width=w)   # noqa: E731
        fn()
        med, best = timed(fn, args.reps)
        moved = gt_bytes + 0.05 * pred.numel() * 4   # dense GT + (at most) the prediction's taps near valid pixels
        result["%dx%d" % (h, w)] = {"ms": round(med, 4), "min_ms": round(best, 4), "GBps": round(moved / med / 1e6, 1),
                                    "of_copy_rate": round(moved / med / 1e6 / copy_gbs, 3),
                                    "x_floor": round(med / result["gt_read_floor_ms"], 2)}
        print("%4dx%-4d  %.3f ms (min %.3f)  %.0f GB/s = %.2f of the copy rate, %.2fx the GT-read floor" % (
            h, w, med, best, moved / med / 1e6, moved / med / 1e6 / copy_gbs, med / result["gt_read_floor_ms"]), flush=True)
        del pred
    from test_depth_eval import restate_eval
    k = min(args.host_images, args.images)
    preds = np.random.default_rng(2).uniform(1, 60, (k, 192, 640)).astype(np.float32)
    t0 = time.perf_counter()
    restate_eval(preds, gts[:k], width=640, split="eigen_raw", pp=False, mono=True)
    host_s = (time.perf_counter() - t0) * args.images / k
    result["host_numpy_s"] = round(host_s, 2)
    result["host_numpy_images_timed"] = k
    print("host numpy restatement: %.2f s for the split (%d images timed, scaled)" % (host_s, k))
    print(json.dumps(result))


if __name__ == "__main__":
    main()
