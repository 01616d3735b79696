"""Novel views at inference: ``ops.render_views`` against the only route that existed before it, in one process.

From the conv outputs and the source image to V rendered views:
  (a) parent   ``ops.decoder_tail`` under ``no_grad`` (writes logits / sigma [B,N,H,W]), then one ``ops.plane_sweep_disp`` forward per
               view with the source image standing in as target (it computes a loss nobody wants and re-reads both tensors).  It
               serves the rig's own baseline only: views beyond the first two repeat "r" / "l", which costs what another view would;
  (b) fused    ``ops.render_views``: one launch, nothing [B,N,H,W]-sized written, the conv outputs read once however many views.
Shapes, all B = 8, 192x640, mixture: 49 planes per plane without a mask; 49 + 14 planes in the row form from ``ops.plane_geometry``
with the horizon inside the crop; fp32 and bf16 conv outputs; V = 1, 2 and 4.
The arms alternate in windows of --steps calls (--windows rounds, the order reversed every other round); every call is timed with
device events, and the median over all calls of an arm and the spread of its window medians (max - min) are reported.  Next to the
times: the fused arm's algorithmic bytes, (2N e + 3*4 + 5V*4) HW per image with e = 4 or 2 bytes per conv-output element, and their
rate against the rate of a plain device copy measured in the same run.  Before anything is timed the first view of the two arms is
compared (the suite's bound for two evaluations of the same oracle, 2e-4; fp32 only: the parent's bf16 route rounds sigma to bf16).

    python scripts/bench_render.py [--steps 20 --windows 8] [--out render_views.json --md profiles/render_views.md]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ARMS = ("parent", "fused")
VIEWS = (1, 2, 4)
BASELINES = (1.0, -1.0, 1.0, -1.0)   # what the parent route can serve, so that both arms render the same views
SIDES = ("r", "l", "r", "l")


def fused_bytes(N, e, V, H, W):
    """Algorithmic bytes per image of the fused arm: conv outputs once, the image, 5 output floats per view and pixel."""
    return (2 * N * e + 3 * 4 + 5 * V * 4) * H * W


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--md", default=None)
    args = ap.parse_args()
    if args.steps * args.windows < 50:
        ap.error("at least 50 calls per arm (--steps x --windows)")

    import __graft_entry__
    __graft_entry__.build()
    import torch
    from planedepth_amd import ops, synthetic

    if not torch.cuda.is_available():
        raise SystemExit("bench_render.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    B, H, W, NL, NX = 8, 192, 640, 49, 14
    g = torch.Generator().manual_seed(1234)
    inputs = synthetic.kitti_like_inputs(B, H, W, seed=3)
    grid = inputs["grid"].to(dev)
    image = torch.rand(B, 3, H, W, generator=g).to(dev)
    with torch.no_grad():
        dl_rows, pm_rows, _, _ = ops.plane_geometry(grid, (torch.rand(B, NL + NX, generator=g) - 0.5).to(dev), no_levels=NL,
                                                    xz_levels=NX, disp_min=2.0, disp_max=300.0, xz_min=0.1852, xz_max=0.3704)
    rows = ops._rows_of(pm_rows)[:, NL:]
    assert bool((rows == 0).any()) and bool((rows == 1).any()), "the horizon of the ground planes is not inside the crop"
    lv = torch.arange(NL, dtype=torch.float32)[None, :, None, None] + torch.rand(B, NL, 1, 1, generator=g) - 0.5
    dl_plane = (300.0 * (2.0 / 300.0) ** (lv / (NL - 1))).to(dev).expand(B, NL, H, W)
    rl = (torch.randn(B, NL + NX, H, W, generator=g) * 2.5).to(dev)
    rs = (torch.randn(B, NL + NX, H, W, generator=g) * 3 - 1).to(dev)
    rl49, rs49 = rl[:, :NL].contiguous(), rs[:, :NL].contiguous()

    def arms(a, s, pm, dl, V):
        def parent():
            logits, sigma, _, _, _ = ops.decoder_tail(a, s, pm, dl)
            return [ops.plane_sweep_disp(image, image, logits, sigma, dl, pm, target_side=SIDES[v])[0] for v in range(V)]

        def fused():
            return ops.render_views(a, s, pm, dl, image, BASELINES[:V]).rgb
        return parent, fused

    shapes = {
        "N=49 per-plane fp32": (NL, 4, rl49, rs49, None, dl_plane),
        "N=49 per-plane bf16": (NL, 2, rl49.bfloat16(), rs49.bfloat16(), None, dl_plane),
        "N=63 rows fp32": (NL + NX, 4, rl, rs, pm_rows, dl_rows),
        "N=63 rows bf16": (NL + NX, 2, rl.bfloat16(), rs.bfloat16(), pm_rows, dl_rows),
    }

    def timed(fn, n):
        evs = [[torch.cuda.Event(enable_timing=True) for _ in range(2)] for _ in range(n)]
        torch.cuda.synchronize(dev)
        for ev in evs:
            ev[0].record()
            fn()
            ev[1].record()
        torch.cuda.synchronize(dev)
        return [ev[0].elapsed_time(ev[1]) for ev in evs]

    # the copy rate of this run: a device copy of one fp32 conv output (read + write)
    src, dst = rl, torch.empty_like(rl)
    timed(lambda: dst.copy_(src), 5)
    copy_ms = statistics.median(timed(lambda: dst.copy_(src), 40))
    copy_gbs = 2 * src.numel() * 4 / copy_ms / 1e6
    del dst

    res = dict(device=torch.cuda.get_device_name(dev), B=B, H=H, W=W, calls_per_arm=args.steps * args.windows,
               copy_gb_per_s=round(copy_gbs, 1), configs={})
    with torch.no_grad():
        for name, (N, e, a, s, pm, dl) in shapes.items():
            for V in VIEWS:
                calls = dict(zip(ARMS, arms(a, s, pm, dl, V)))
                p, f = calls["parent"](), calls["fused"]()
                err = float((p[0] - f[:, 0]).abs().max() / p[0].abs().max())
                assert e == 2 or err < 2e-4, "%s V=%d: the first view of the two arms differs by %.3g" % (name, V, err)
                del p, f
                for _ in range(args.warmup):
                    for arm in ARMS:
                        calls[arm]()
                per_call = {k: [] for k in ARMS}
                window_medians = {k: [] for k in ARMS}
                for w in range(args.windows):
                    for arm in (ARMS if w % 2 == 0 else ARMS[::-1]):
                        t = timed(calls[arm], args.steps)
                        per_call[arm] += t
                        window_medians[arm].append(statistics.median(t))
                r = dict(N=N, V=V, first_view_rel_diff=err)
                for arm in ARMS:
                    wm = window_medians[arm]
                    r[arm] = dict(ms=round(statistics.median(per_call[arm]), 4), spread_ms=round(max(wm) - min(wm), 4),
                                  window_medians_ms=[round(t, 4) for t in wm])
                nbytes = fused_bytes(N, e, V, H, W) * B
                r["fused"]["algorithmic_mb"] = round(nbytes / 1e6, 1)
                r["fused"]["gb_per_s"] = round(nbytes / r["fused"]["ms"] / 1e6, 1)
                r["fused"]["share_of_copy_rate"] = round(r["fused"]["gb_per_s"] / copy_gbs, 3)
                diff = r["parent"]["ms"] - r["fused"]["ms"]
                spread = max(r["parent"]["spread_ms"], r["fused"]["spread_ms"])
                r["parent_minus_fused_ms"] = round(diff, 4)
                r["time_ratio"] = round(r["fused"]["ms"] / r["parent"]["ms"], 3)
                r["verdict"] = ("fused is faster beyond the spread" if diff > spread else
                                "fused is slower beyond the spread" if -diff > spread else "no difference beyond the spread")
                res["configs"]["%s V=%d" % (name, V)] = r
    print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    if args.md:
        lines = ["# Novel views at inference: the fused operator against the parent's route", "",
                 "`scripts/bench_render.py --steps %d --windows %d` on %s: from the decoder's conv outputs and the source image to V"
                 % (args.steps, args.windows, res["device"]),
                 "rendered views, B = %d, %dx%d, mixture.  parent = `ops.decoder_tail` under `torch.no_grad()`, then one" % (B, H, W),
                 "`ops.plane_sweep_disp` forward per view with the source image standing in as target (the only route before);",
                 "fused = `ops.render_views`, one launch.  Device events around every call (allocations and launches included), the arms",
                 "alternating in one process; median over the %d calls of an arm, spread = max - min of the arm's %d window medians."
                 % (res["calls_per_arm"], args.windows),
                 "Both arms render the same views (+1, -1, +1, -1: the parent route has no other baselines).", "",
                 "Algorithmic bytes of the fused arm: (2N e + 3*4 + 5V*4) HW per image, e = 4 (fp32) or 2 (bf16) bytes per conv-output",
                 "element; GB/s = those bytes over the call time; copy = a device copy of one fp32 conv output in the same run, %.0f GB/s"
                 % res["copy_gb_per_s"], "(read + write).", "",
                 "| configuration | parent, ms | spread | fused, ms | spread | fused / parent | fused MB | GB/s | of copy rate | verdict |",
                 "|---|---|---|---|---|---|---|---|---|---|"]
        for name, r in res["configs"].items():
            lines.append("| %s | %.4f | %.4f | %.4f | %.4f | %.3f | %.1f | %.0f | %.2f | %s |" % (
                name, r["parent"]["ms"], r["parent"]["spread_ms"], r["fused"]["ms"], r["fused"]["spread_ms"], r["time_ratio"],
                r["fused"]["algorithmic_mb"], r["fused"]["gb_per_s"], r["fused"]["share_of_copy_rate"], r["verdict"]))
        lines += ["", "Cost of a view after the first, fused arm: (V = 4 minus V = 1) / 3 against V = 1.", "",
                  "| shape | first view, ms | each further view, ms | ratio |", "|---|---|---|---|"]
        for name in shapes:
            t1, t4 = (res["configs"]["%s V=%d" % (name, V)]["fused"]["ms"] for V in (1, 4))
            lines.append("| %s | %.4f | %.4f | %.2f |" % (name, t1, (t4 - t1) / 3, (t4 - t1) / 3 / t1))
        os.makedirs(os.path.dirname(os.path.abspath(args.md)), exist_ok=True)
        with open(args.md, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
