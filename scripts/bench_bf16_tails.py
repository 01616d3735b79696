"""The fused decoder tail with fp32 against bf16 conv outputs (PD_TAIL_BF16), in one process.

Three arms per shape, forward and backward timed separately (device events around each, summed over a window):
  (a) fp32     the fp32 tail on fp32 conv outputs;
  (b) cast     what an autocast user had to write before the tail took bf16: .float() on both bf16 conv outputs, the fp32
               tail, and a backward that includes the two casts' backward (fp32 gradients rounded to bf16);
  (c) bf16     the bf16 tail on the bf16 conv outputs.
The arms run in interleaved windows of --steps steps each (--windows rounds, the order reversed every other round); medians
are reported with the algorithmic bytes of each arm's tail kernels (pd_decoder_tail.hip: forward reads 2N (+N mask) and
writes N (+N with a mask) elements per pixel, backward reads 4N (+N) and writes 2N; the mask is fp32 in every arm) and the
ratios (c)/(a), (c)/(b).  The upstream gradients are those of a training step: logits, sigma (in the tail's output dtype)
and disp.

    python scripts/bench_bf16_tails.py [--steps 20 --windows 7] [--out profiles/bf16_tails.json --md profiles/bf16_tails.md]
Kernel times: run it under rocprofv3 --kernel-trace --stats (a separate run; --windows 2 keeps the trace small).
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ARMS = ("fp32", "cast", "bf16")


def tail_bytes(N, HW, mask, elem):
    """(forward, backward) algorithmic bytes per image of the tail kernels with `elem`-byte conv outputs."""
    m = 4 * N if mask else 0
    fwd = 2 * N * elem + m + (2 * N if mask else N) * elem + 4 * 4
    bwd = 4 * N * elem + m + 2 * N * elem + 5 * 4
    return fwd * HW, bwd * HW


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--md", default=None)
    args = ap.parse_args()

    import __graft_entry__
    __graft_entry__.build()
    import torch
    from planedepth_amd import ops

    dev = torch.device("cuda:0")
    B, H, W = 8, 192, 640
    shapes = [dict(name="N=49, no mask (xy planes)", N=49, mask=False),
              dict(name="N=49, mask", N=49, mask=True),
              dict(name="N=63, mask (xz rows)", N=63, mask=True)]
    results = []
    for sh in shapes:
        N = sh["N"]
        g = torch.Generator().manual_seed(1234 + N)
        rl = (torch.randn(B, N, H, W, generator=g) * 2.5).to(dev)
        rs = (torch.randn(B, N, H, W, generator=g) * 3 - 1).to(dev)
        lv = torch.arange(N, dtype=torch.float32)[None, :, None, None] + torch.rand(B, N, 1, 1, generator=g) - 0.5
        levels = (300.0 * (2.0 / 300.0) ** (lv / (N - 1))).to(dev).requires_grad_(True)
        pm = None
        if sh["mask"]:
            pm = torch.ones(B, N, H, W, device=dev)
            pm[:, N - N // 4:, :H // 2] = 0.0
        g_disp = torch.randn(B, 1, H, W, generator=g).to(dev)
        ups = {dt: (torch.randn(B, N, H, W, generator=g).to(dev).to(dt), torch.randn(B, N, H, W, generator=g).to(dev).to(dt))
               for dt in (torch.float32, torch.bfloat16)}
        leaves = {"fp32": (rl.clone().requires_grad_(True), rs.clone().requires_grad_(True)),
                  "cast": (rl.bfloat16().requires_grad_(True), rs.bfloat16().requires_grad_(True)),
                  "bf16": (rl.bfloat16().requires_grad_(True), rs.bfloat16().requires_grad_(True))}
        del rl, rs

        def step(arm, ev=None):
            lg, sg = leaves[arm]
            if ev:
                ev[0].record()
            a, s = (lg.float(), sg.float()) if arm == "cast" else (lg, sg)
            logits, sigma, disp, _, _ = ops.decoder_tail(a, s, pm, levels.expand(-1, -1, H, W))
            if ev:
                ev[1].record()
            gl, gs = ups[logits.dtype]
            torch.autograd.grad([logits, sigma, disp], [lg, sg, levels], [gl, gs, g_disp])
            if ev:
                ev[2].record()

        for _ in range(args.warmup):
            for arm in ARMS:
                step(arm)
        times = {arm: dict(fwd=[], bwd=[]) for arm in ARMS}
        for w in range(args.windows):
            for arm in (ARMS if w % 2 == 0 else ARMS[::-1]):
                evs = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(args.steps)]
                torch.cuda.synchronize(dev)
                for ev in evs:
                    step(arm, ev)
                torch.cuda.synchronize(dev)
                times[arm]["fwd"].append(sum(ev[0].elapsed_time(ev[1]) for ev in evs) / args.steps)
                times[arm]["bwd"].append(sum(ev[1].elapsed_time(ev[2]) for ev in evs) / args.steps)
        row = dict(shape=sh["name"], B=B, N=N, H=H, W=W, mask=sh["mask"])
        for arm in ARMS:
            by = tail_bytes(N, H * W, sh["mask"], 2 if arm == "bf16" else 4)
            row[arm] = {}
            for i, leg in enumerate(("fwd", "bwd")):
                ms = statistics.median(times[arm][leg])
                row[arm][leg] = dict(ms=round(ms, 4), tail_kernel_bytes_per_image=by[i],
                                     fraction_of_8TBps=round(by[i] * B / (ms * 1e-3) / 8e12, 3),
                                     windows_ms=[round(t, 4) for t in times[arm][leg]])
        for leg in ("fwd", "bwd"):
            c = row["bf16"][leg]
            row["bf16_over_fp32_" + leg] = round(c["ms"] / row["fp32"][leg]["ms"], 3)
            row["bf16_over_cast_" + leg] = round(c["ms"] / row["cast"][leg]["ms"], 3)
            row["bytes_bf16_over_fp32_" + leg] = round(c["tail_kernel_bytes_per_image"] / row["fp32"][leg]["tail_kernel_bytes_per_image"], 3)
        results.append(row)
        print(json.dumps({k: (v if k not in ARMS else {leg: v[leg]["ms"] for leg in v}) for k, v in row.items()}), flush=True)
        del leaves, ups, pm
        torch.cuda.empty_cache()
    out = dict(device=torch.cuda.get_device_name(dev), steps=args.steps, windows=args.windows, results=results)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    if args.md:
        lines = ["# Fused decoder tail: fp32 against bf16 conv outputs", "",
                 "`scripts/bench_bf16_tails.py --steps %d --windows %d` on %s, B = %d, %dx%d; medians over the windows, ms per"
                 % (args.steps, args.windows, out["device"], B, H, W),
                 "call (device events; the arms alternate in one process).  fp32: the fp32 tail on fp32 conv outputs; cast: `.float()`",
                 "on both bf16 conv outputs, the fp32 tail, the casts' backward; bf16: the bf16 tail (PD_TAIL_BF16).  bytes: the",
                 "algorithmic bytes of the bf16 tail kernel over the fp32 one's (the padding mask stays fp32).", "",
                 "| shape | leg | fp32 | cast | bf16 | bf16 / fp32 | bf16 / cast | bytes bf16 / fp32 | bf16 share of 8 TB/s |",
                 "|---|---|---|---|---|---|---|---|---|"]
        for r in results:
            for leg in ("fwd", "bwd"):
                lines.append("| %s | %s | %.4f | %.4f | %.4f | %.3f | %.3f | %.3f | %.3f |" % (
                    r["shape"], leg, r["fp32"][leg]["ms"], r["cast"][leg]["ms"], r["bf16"][leg]["ms"], r["bf16_over_fp32_" + leg],
                    r["bf16_over_cast_" + leg], r["bytes_bf16_over_fp32_" + leg], r["bf16"][leg]["fraction_of_8TBps"]))
        os.makedirs(os.path.dirname(os.path.abspath(args.md)), exist_ok=True)
        with open(args.md, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
