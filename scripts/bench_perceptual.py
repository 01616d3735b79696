"""Fused perceptual feature distance (ops.feature_distance, forward + backward) against the reference formulation in plain torch
on the same device, in one process.

    python scripts/bench_perceptual.py [--B 8] [--H 192] [--W 640] [--windows 9] [--iters 10] [--json FILE] [--md FILE]

Per VGG level ([B,64,H,W], [B,128,H/2,W/2], [B,256,H/4,W/4]) and for the three together, fp32 and bf16, with and without a
source (automask): both arms run forward + backward in alternating windows of --iters steps (HIP events around a window), and the
report gives per arm the median window's time per step, the window-to-window spread ((max - min) / median), the bytes the arm
must move by the counts of pd_feature_distance.hip's header (fused: 2 reads forward, 3 with a source, 2 reads + 1 write backward;
torch: 6 tensor passes forward, 12 with a source, 4 backward), their rate as a fraction of the device-to-device copy rate
measured in the same run (clone of one level-0 feature tensor: read + write), and the peak device memory above what the inputs
occupy (torch.cuda.max_memory_allocated).  The yardstick is the torch arm of the same run, never an earlier run of the fused code:
``lead_beyond_spread`` says whether fused * (1 + its spread) < torch * (1 - its spread).

Needs a GPU: there is no CPU timing path.  --json / --md write the result files (profiles/perceptual_bench.json, .md).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def torch_formulation(pred_f, target_f, source_f=None):
    """trainer.py:678-685 as the reference writes it."""
    loss = 0
    for i in range(len(pred_f)):
        l_p = ((pred_f[i] - target_f[i]) ** 2).mean(1, True)
        if source_f is not None:
            l_a = ((source_f[i] - target_f[i]) ** 2).mean(1, True)
            l_p, _ = torch.cat([l_p, l_a], dim=1).min(1, True)
        loss += l_p.mean()
    return loss


def window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def peak_above_inputs(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=8)
    ap.add_argument("--H", type=int, default=192)
    ap.add_argument("--W", type=int, default=640)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--json")
    ap.add_argument("--md")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_perceptual.py measures on a GPU; there is no CPU path"
    import __graft_entry__
    __graft_entry__.build()
    from planedepth_amd import ops
    B, H, W = args.B, args.H, args.W
    shapes = [(B, 64, H, W), (B, 128, H // 2, W // 2), (B, 256, H // 4, W // 4)]
    g = torch.Generator(device="cuda").manual_seed(1)
    probe = torch.randn(shapes[0], device="cuda", generator=g)
    for _ in range(3):
        probe.clone()
    copy_ms = float(np.median([window(lambda: probe.clone(), 10) for _ in range(args.windows)]))
    copy_gbs = 2 * probe.numel() * 4 / copy_ms / 1e6
    del probe
    result = {"device": torch.cuda.get_device_name(0), "B": B, "H": H, "W": W, "windows": args.windows, "iters": args.iters,
              "d2d_copy_GBps": round(copy_gbs, 1), "rows": []}
    print("device-to-device copy: %.0f GB/s" % copy_gbs, flush=True)
    for dt_name, dtype in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
        target = [torch.randn(s, device="cuda", generator=g).to(dtype) for s in shapes]
        pred = [(t.float() + 0.3 * torch.randn(t.shape, device="cuda", generator=g)).to(dtype).requires_grad_(True) for t in target]
        source = [(t.float() + 0.3 * torch.randn(t.shape, device="cuda", generator=g)).to(dtype) for t in target]
        for with_source in (False, True):
            for name, idx in (("level0", [0]), ("level1", [1]), ("level2", [2]), ("all", [0, 1, 2])):
                p, t = [pred[i] for i in idx], [target[i] for i in idx]
                s = [source[i] for i in idx] if with_source else None
                arms = {"fused": lambda: torch.autograd.grad(ops.feature_distance(p, t, s), p),
                        "torch": lambda: torch.autograd.grad(torch_formulation(p, t, s), p)}
                F = sum(x.numel() * x.element_size() for x in p)
                moved = {"fused": (5 + with_source) * F, "torch": (10 + 6 * with_source) * F}
                times = {k: [] for k in arms}
                for fn in arms.values():      # warm-up: code objects, the allocator's blocks
                    for _ in range(3):
                        fn()
                for _ in range(args.windows):   # arms interleaved window by window
                    for k, fn in arms.items():
                        times[k].append(window(fn, args.iters))
                row = {"dtype": dt_name, "source": with_source, "levels": name, "feature_bytes": F}
                for k, fn in arms.items():
                    med = float(np.median(times[k]))
                    row[k] = {"ms": round(med, 4), "spread": round((max(times[k]) - min(times[k])) / med, 4),
                              "bytes": moved[k], "GBps": round(moved[k] / med / 1e6, 1),
                              "of_copy_rate": round(moved[k] / med / 1e6 / copy_gbs, 3),
                              "peak_bytes_above_inputs": int(peak_above_inputs(fn))}
                row["torch_over_fused"] = round(row["torch"]["ms"] / row["fused"]["ms"], 3)
                row["lead_beyond_spread"] = bool(row["fused"]["ms"] * (1 + row["fused"]["spread"]) <
                                                 row["torch"]["ms"] * (1 - row["torch"]["spread"]))
                result["rows"].append(row)
                print("%s %-7s %-6s fused %.3f ms (+-%.1f %%, %.2f of copy rate, peak %.0f MB)  torch %.3f ms (+-%.1f %%, peak %.0f MB)  "
                      "x%.2f %s" % (dt_name, "source" if with_source else "plain", name, row["fused"]["ms"],
                                    100 * row["fused"]["spread"], row["fused"]["of_copy_rate"],
                                    row["fused"]["peak_bytes_above_inputs"] / 1e6, row["torch"]["ms"], 100 * row["torch"]["spread"],
                                    row["torch"]["peak_bytes_above_inputs"] / 1e6, row["torch_over_fused"],
                                    "ok" if row["lead_beyond_spread"] else "INSIDE THE SPREAD"), flush=True)
        del target, pred, source
    result["every_lead_beyond_spread"] = all(r["lead_beyond_spread"] for r in result["rows"])
    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)
    if args.md:
        with open(args.md, "w") as f:
            f.write(markdown(result))
    print(json.dumps({k: v for k, v in result.items() if k != "rows"}))


def markdown(r):
    out = ["# Perceptual feature distance: fused operator vs the torch formulation", "",
           "One run of `scripts/bench_perceptual.py` on %s: B = %d, %dx%d, forward + backward, %d alternating windows of %d steps "
           "per arm; median window, spread = (max - min) / median.  Device-to-device copy rate of the same run: **%.0f GB/s** "
           "(the guide's float4 copy: 6290 GB/s).  Bytes by the counts of `planedepth_amd/csrc/pd_feature_distance.hip`; "
           "peak memory is above what the inputs occupy." % (r["device"], r["B"], r["H"], r["W"], r["windows"], r["iters"],
                                                              r["d2d_copy_GBps"]), "",
           "| dtype | source | levels | fused ms | spread | of copy rate | peak MB | torch ms | spread | peak MB | torch / fused | beyond spread |",
           "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for x in r["rows"]:
        f, t = x["fused"], x["torch"]
        out.append("| %s | %s | %s | %.3f | %.1f %% | %.2f | %.0f | %.3f | %.1f %% | %.0f | %.2f | %s |" % (
            x["dtype"], "yes" if x["source"] else "no", x["levels"], f["ms"], 100 * f["spread"], f["of_copy_rate"],
            f["peak_bytes_above_inputs"] / 1e6, t["ms"], 100 * t["spread"], t["peak_bytes_above_inputs"] / 1e6,
            x["torch_over_fused"], "yes" if x["lead_beyond_spread"] else "no"))
    out += ["", "Every lead beyond both arms' spread: **%s**." % ("yes" if r["every_lead_beyond_spread"] else "no"), ""]
    return "\n".join(out)


if __name__ == "__main__":
    main()
