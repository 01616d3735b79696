"""The fused input pipeline against the torch formulation of the same transforms, on the device, in one process.

From B x V decoded 375x1242 uint8 frames to the 192x640 ``color`` / ``color_aug`` windows of a training step:
  (a) fused  ``ops.resize_crop_augment``: one launch, only the windows are computed;
  (b) torch  what datasets/pair_transforms.py does, moved to the device as it stands: ``.float() / 255``, permute, per sample
             ``F.interpolate(bicubic, align_corners=True)`` of the whole frame, clamp, crop, and the three augmentation ops.
B = 8 with V = 2 and V = 4, parameters from ``pipeline.draw_params`` (factor in [0.75, 1.5], every stage on so that both arms do
the same work on every sample).  The arms alternate in windows of --steps calls (--windows rounds, the order reversed every other
round); every call is timed with device events; reported are the median over all calls of an arm and the spread of its window
medians.  Next to them: the fused call's algorithmic bytes (both outputs written once, the source pixels under the windows read
once) over its time, against the rate of a plain device copy of 256 MiB measured in the same run.  Before anything is timed the
two arms' ``color`` are compared (torch's fp32 coordinate is up to 1e-4 from the exact one at this size).

    python scripts/bench_input_pipeline.py [--steps 20 --windows 8] [--out input_pipeline.json --md profiles/input_pipeline.md]
"""
import argparse
import json
import os
import random
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ARMS = ("fused", "torch")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--md", default=None)
    args = ap.parse_args()
    if args.steps * args.windows < 100:
        ap.error("at least 100 calls per arm (--steps x --windows)")

    import __graft_entry__
    __graft_entry__.build()
    import numpy as np
    import torch
    import torch.nn.functional as F
    from planedepth_amd import ops, pipeline

    if not torch.cuda.is_available():
        raise SystemExit("bench_input_pipeline.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    B, HS, WS, H, W = 8, 375, 1242, 192, 640

    def timed(calls, order):
        per_call, window_medians = {a: [] for a in order}, {a: [] for a in order}
        for w in range(args.windows):
            for arm in (order if w % 2 == 0 else order[::-1]):
                evs = [[torch.cuda.Event(enable_timing=True) for _ in range(2)] for _ in range(args.steps)]
                torch.cuda.synchronize(dev)
                for ev in evs:
                    ev[0].record()
                    calls[arm]()
                    ev[1].record()
                torch.cuda.synchronize(dev)
                t = [ev[0].elapsed_time(ev[1]) for ev in evs]
                per_call[arm] += t
                window_medians[arm].append(statistics.median(t))
        return {a: dict(ms=round(statistics.median(per_call[a]), 4), window_medians_ms=[round(t, 4) for t in window_medians[a]],
                        spread_ms=round(max(window_medians[a]) - min(window_medians[a]), 4)) for a in order}

    res = dict(device=torch.cuda.get_device_name(dev), B=B, frame=[HS, WS], window=[H, W], calls_per_arm=args.steps * args.windows,
               shapes={})
    # the copy rate of this run: 256 MiB device to device, read + written bytes over the median time
    a, b = torch.empty(64 << 20, device=dev), torch.empty(64 << 20, device=dev)
    for _ in range(args.warmup):
        b.copy_(a)
    copy = timed({"copy": lambda: b.copy_(a)}, ("copy",))["copy"]
    copy_gbs = 2 * a.numel() * 4 / copy["ms"] / 1e6
    res["copy"] = dict(copy, mib=256, gb_per_s=round(copy_gbs, 1))
    del a, b

    for V in (2, 4):
        g = torch.Generator().manual_seed(V)
        frames = torch.randint(0, 256, (B, V, HS, WS, 3), generator=g, dtype=torch.uint8).to(dev)
        p = pipeline.draw_params(random.Random(V), np.random.RandomState(V), B, V, [[HS, WS]] * B, H, W)
        p = p._replace(flags=p.flags | 7)      # every stage on every sample (a stage that was not drawn keeps its factor 1)
        host = [t.tolist() for t in p]
        on_dev = [t.to(dev) for t in p]

        def fused():
            return ops.resize_crop_augment(frames, *on_dev, H, W)

        def torch_arm():
            x = frames.float().div(255).permute(0, 1, 4, 2, 3)
            color, color_aug = [], []
            for s in range(B):
                fw, fh, w0, h0 = host[1][s]
                img = x[s].flip(-1) if host[2][s] & 8 else x[s]
                c = F.interpolate(img, size=(fh, fw), mode="bicubic", align_corners=True).clamp(min=0.0, max=1.0)
                c = c[:, :, h0:h0 + H, w0:w0 + W].contiguous()
                f = on_dev[3][s]
                q = c ** f[:, 0, None, None, None]
                q = (q * f[:, 1, None, None, None]).clamp(max=1.0)
                q = (q * f[:, 2:, None, None]).clamp(max=1.0)
                color.append(c)
                color_aug.append(q)
            return torch.stack(color), torch.stack(color_aug)

        calls = dict(fused=fused, torch=torch_arm)
        with torch.no_grad():
            x, y = fused(), torch_arm()
            dist = [float((x[i] - y[i]).abs().max()) for i in range(2)]
            del x, y
            for _ in range(args.warmup):
                for arm in ARMS:
                    calls[arm]()
            r = timed(calls, ARMS)
        written = 2 * B * V * 3 * H * W * 4
        read = sum(V * 3 * min(HS, int(H * HS / fh) + 4) * min(WS, int(W * WS / fw) + 4) for fw, fh, _, _ in host[1])
        r["fused"].update(bytes_written=written, bytes_read=read, gb_per_s=round((written + read) / r["fused"]["ms"] / 1e6, 1))
        r["fused"]["share_of_copy_rate"] = round(r["fused"]["gb_per_s"] / copy_gbs, 3)
        diff, spread = r["torch"]["ms"] - r["fused"]["ms"], max(r["torch"]["spread_ms"], r["fused"]["spread_ms"])
        r.update(V=V, color_distance=dist[0], color_aug_distance=dist[1], torch_over_fused=round(r["torch"]["ms"] / r["fused"]["ms"], 2),
                 verdict=("fused is faster beyond the spread" if diff > spread else
                          "fused is slower beyond the spread" if -diff > spread else "no difference beyond the spread"))
        res["shapes"]["V=%d" % V] = r
        del frames
    print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    if args.md:
        lines = ["# Input pipeline: the fused call against torch's formulation on the device", "",
                 "`scripts/bench_input_pipeline.py --steps %d --windows %d` on %s: B = %d samples of V views, %dx%d uint8 frames into"
                 % (args.steps, args.windows, res["device"], B, HS, WS),
                 "%dx%d `color` / `color_aug` windows, parameters from `pipeline.draw_params` with every stage on.  fused ="
                 % (H, W),
                 "`ops.resize_crop_augment` (one launch); torch = `.float() / 255`, permute, per-sample `F.interpolate` bicubic of the",
                 "whole frame, clamp, crop and the three augmentation ops, on the device.  Device events around every call, the arms",
                 "alternating in one process; median over the %d calls of an arm, spread = max - min of the arm's %d window medians."
                 % (res["calls_per_arm"], args.windows), "",
                 "Bytes of the fused call: both outputs written once plus the source pixels under the windows read once, over the call's",
                 "time (allocations and the host's share included); copy rate = a 256 MiB device-to-device `copy_` in the same run,",
                 "read + written bytes over its median time: %.0f GB/s (%.4f ms, spread %.4f ms)."
                 % (res["copy"]["gb_per_s"], res["copy"]["ms"], res["copy"]["spread_ms"]), "",
                 "| views | arm | call, ms | spread, ms | bytes written | bytes read | GB/s | share of the copy rate |",
                 "|---|---|---|---|---|---|---|---|"]
        for name, r in res["shapes"].items():
            f = r["fused"]
            lines.append("| %s | fused | %.4f | %.4f | %d | %d | %.0f | %.3f |" % (name, f["ms"], f["spread_ms"], f["bytes_written"],
                                                                                f["bytes_read"], f["gb_per_s"], f["share_of_copy_rate"]))
            lines.append("| %s | torch | %.4f | %.4f | | | | |" % (name, r["torch"]["ms"], r["torch"]["spread_ms"]))
        lines += ["", "| views | torch / fused, time | verdict | max distance of the arms' color | of color_aug |", "|---|---|---|---|---|"]
        for name, r in res["shapes"].items():
            lines.append("| %s | %.2f | %s | %.2e | %.2e |" % (name, r["torch_over_fused"], r["verdict"], r["color_distance"],
                                                             r["color_aug_distance"]))
        lines += ["", "The distance between the arms is torch's: it forms scale x index in fp32, the kernel splits the coordinate by an",
                  "integer division (tests/test_input_pipeline.py::test_kitti_sized_frame_is_closer_to_fp64_than_torch)."]
        os.makedirs(os.path.dirname(os.path.abspath(args.md)), exist_ok=True)
        with open(args.md, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
