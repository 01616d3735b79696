"""The decoder's geometry head + tail with ground planes: dense maps against the row form, in one process.

Two routes, forward + backward of one training-shaped step (upstream gradients on logits, sigma and disp; the gradient is taken
down to the level residuals and the conv outputs):
  (a) dense   synthetic.decoder_plane_geometry (the reference's torch lines, dense [B,N,H,W] map and mask, autograd backwards) +
              the dense decoder tail (PD_TAIL_DISP_DENSE, dense mask);
  (b) rows    ops.plane_geometry (pd_plane_geometry_fwd / _bwd) + the row-form tail (PD_TAIL_DISP_ROWS | PD_TAIL_MASK_ROWS).
B = 8, 192x640, 49 + 14 planes, mixture, fp32 and bf16 conv outputs.  The routes run in interleaved windows of --steps steps
each (--windows rounds, the order reversed every other round); medians of the windows and the ratio (b) / (a) are reported.
What (b) is measured against is (a) in the same process, never an earlier run.

    python scripts/bench_plane_geometry.py [--steps 20 --windows 7] [--out plane_rows.json --md profiles/plane_rows.md]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROUTES = ("dense", "rows")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--md", default=None)
    args = ap.parse_args()

    import __graft_entry__
    __graft_entry__.build()
    import torch
    from planedepth_amd import ops, synthetic

    dev = torch.device("cuda:0")
    B, H, W, NL, NX = 8, 192, 640, 49, 14
    N = NL + NX
    cfg = dict(no_levels=NL, xz_levels=NX, disp_min=2.0, disp_max=300.0, xz_min=0.1852, xz_max=0.3704)
    g = torch.Generator().manual_seed(1234)
    grid = synthetic.kitti_like_inputs(B, H, W, seed=3)["grid"].to(dev)
    residual = (torch.rand(B, N, generator=g) - 0.5).to(dev).requires_grad_(True)
    g_disp = torch.randn(B, 1, H, W, generator=g).to(dev)
    results = []
    for st in (torch.float32, torch.bfloat16):
        rl = (torch.randn(B, N, H, W, generator=g) * 2.5).to(dev).to(st).requires_grad_(True)
        rs = (torch.randn(B, N, H, W, generator=g) * 3 - 1).to(dev).to(st).requires_grad_(True)
        gl, gs = (torch.randn(B, N, H, W, generator=g).to(dev).to(st) for _ in range(2))

        def step(route, ev=None):
            if ev:
                ev[0].record()
            if route == "rows":
                dl, pm, _, _ = ops.plane_geometry(grid, residual, **cfg)
            else:
                geo = synthetic.decoder_plane_geometry(grid, residual, **cfg)
                dl, pm = geo["disp_layered"], geo["padding_mask"]
            logits, sigma, disp, _, _ = ops.decoder_tail(rl, rs, pm, dl)
            if ev:
                ev[1].record()
            torch.autograd.grad([logits, sigma, disp], [rl, rs, residual], [gl, gs, g_disp])
            if ev:
                ev[2].record()

        for _ in range(args.warmup):
            for route in ROUTES:
                step(route)
        times = {r: dict(fwd=[], bwd=[], total=[]) for r in ROUTES}
        for w in range(args.windows):
            for route in (ROUTES if w % 2 == 0 else ROUTES[::-1]):
                evs = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(args.steps)]
                torch.cuda.synchronize(dev)
                for ev in evs:
                    step(route, ev)
                torch.cuda.synchronize(dev)
                f = sum(ev[0].elapsed_time(ev[1]) for ev in evs) / args.steps
                b = sum(ev[1].elapsed_time(ev[2]) for ev in evs) / args.steps
                times[route]["fwd"].append(f)
                times[route]["bwd"].append(b)
                times[route]["total"].append(f + b)
        row = dict(conv_outputs=str(st).replace("torch.", ""), B=B, N=N, H=H, W=W)
        for route in ROUTES:
            row[route] = {leg: dict(ms=round(statistics.median(v), 4), windows_ms=[round(t, 4) for t in v])
                          for leg, v in times[route].items()}
        for leg in ("fwd", "bwd", "total"):
            row["rows_over_dense_" + leg] = round(row["rows"][leg]["ms"] / row["dense"][leg]["ms"], 3)
        results.append(row)
        print(json.dumps({k: (v if k not in ROUTES else {leg: v[leg]["ms"] for leg in v}) for k, v in row.items()}), flush=True)
        del rl, rs, gl, gs
        torch.cuda.empty_cache()
    out = dict(device=torch.cuda.get_device_name(dev), steps=args.steps, windows=args.windows, results=results)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    if args.md:
        lines = ["# Ground planes: dense geometry + dense tail against the row form", "",
                 "`scripts/bench_plane_geometry.py --steps %d --windows %d` on %s, B = %d, %dx%d, %d + %d planes, mixture; medians"
                 % (args.steps, args.windows, out["device"], B, H, W, NL, NX),
                 "over the windows, ms per call (device events; the routes alternate in one process).  dense:",
                 "`synthetic.decoder_plane_geometry` (the reference's torch lines) + the dense tail; rows: `ops.plane_geometry` + the",
                 "row-form tail.  Forward + backward down to the level residuals and the conv outputs.", "",
                 "| conv outputs | leg | dense | rows | rows / dense |", "|---|---|---|---|---|"]
        for r in results:
            for leg in ("fwd", "bwd", "total"):
                lines.append("| %s | %s | %.4f | %.4f | %.3f |" % (r["conv_outputs"], leg, r["dense"][leg]["ms"], r["rows"][leg]["ms"],
                                                                  r["rows_over_dense_" + leg]))
        os.makedirs(os.path.dirname(os.path.abspath(args.md)), exist_ok=True)
        with open(args.md, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
