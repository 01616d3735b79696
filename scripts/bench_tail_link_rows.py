"""The tail link on the row form: ``fuse_sweep_backward=True`` against ``False``, in one process.

One training-shaped step of the decoder side with the reference's default plane set (49 xy + 14 xz planes, the horizon inside
the crop), mixture, fp32: ``fused_plane_geometry`` + ``fused_decoder_tail`` + ``plane_sweep_disp`` forward, then the backward of
``ph_mean + <disp, w>`` down to the conv outputs and the plane residual.
  (a) unfused  the sweep's backward (pd_plane_sweep_bwd) and the tail's (pd_decoder_tail_bwd, row form) as two kernels — the
               behaviour before the row-form link existed, and the yardstick;
  (b) fused    the sweep's backward applies the tail's (pd_plane_sweep_bwd_tail_rows); the tail's kernel does not run.
B = 8, 192x640.  The arms alternate in windows of --steps steps (--windows rounds, the order reversed every other round); every
step is timed with device events, and the median over all steps of an arm and the spread of its window medians are reported.
After the timed windows a separate pass collects the per-kernel times (``ops.KERNEL_EVENTS``: event pairs around each C-ABI
call; they add host work, so they stay out of the step timing).  Before anything is timed the two arms' gradients are compared.

    python scripts/bench_tail_link_rows.py [--steps 10 --windows 8] [--out tail_link_rows.json --md profiles/tail_link_rows.md]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ARMS = ("unfused", "fused")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--windows", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--kernel-steps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--md", default=None)
    args = ap.parse_args()
    if args.steps * args.windows < 50:
        ap.error("at least 50 steps per arm (--steps x --windows)")

    import __graft_entry__
    __graft_entry__.build()
    import torch
    from planedepth_amd import ops, synthetic
    from planedepth_amd.decoder_tail import fused_decoder_tail, fused_plane_geometry

    if not torch.cuda.is_available():
        raise SystemExit("bench_tail_link_rows.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    B, H, W, NL, NX = 8, 192, 640, 49, 14
    N = NL + NX
    cfg = dict(no_levels=NL, xz_levels=NX, disp_min=2.0, disp_max=300.0, xz_min=0.1852, xz_max=0.3704)
    g = torch.Generator().manual_seed(1234)
    grid = synthetic.kitti_like_inputs(B, H, W, seed=3)["grid"].to(dev)
    residual = (torch.rand(B, N, generator=g) - 0.5).to(dev).requires_grad_(True)
    rl = (torch.randn(B, N, H, W, generator=g) * 2.5).to(dev).requires_grad_(True)
    rs = (torch.randn(B, N, H, W, generator=g) * 3 - 1).to(dev).requires_grad_(True)
    src, tgt = (torch.rand(B, 3, H, W, generator=g).to(dev) for _ in range(2))
    w_disp = (torch.randn(B, 1, H, W, generator=g) * 1e-2).to(dev)

    def step(arm, ev=None):
        if ev:
            ev[0].record()
        outputs = fused_plane_geometry({}, grid, residual, **cfg)
        fused_decoder_tail(outputs, rl, rs, use_mixture_loss=True, fuse_sweep_backward=(arm == "fused"))
        link = getattr(outputs["logits"], "_pd_tail_link", None)
        _, _, ph_mean = ops.plane_sweep_disp(src, tgt, outputs["logits"], outputs["sigma"], outputs["disp_layered"],
                                             outputs["padding_mask"], return_mean=True)
        ops.tail_taps(outputs)
        grads = torch.autograd.grad(ph_mean + (outputs["disp"] * w_disp).sum(), [rl, rs, residual])
        if ev:
            ev[1].record()
        return grads, link, outputs

    # the horizon is inside the crop, the fused arm fuses, and the arms agree
    _, link, outputs = step("fused")
    rows = ops._rows_of(outputs["padding_mask"])[:, NL:]
    assert bool((rows == 0).any()) and bool((rows == 1).any()), "the horizon of the ground planes is not inside the crop"
    assert link is not None and link.fused_passes == 1, "the fused arm made no tail link"
    ga, _, _ = step("unfused")
    gb, _, _ = step("fused")
    agree = [float((a - b).abs().max() / a.abs().max()) for a, b in zip(ga, gb)]
    assert max(agree) < 5e-6, agree
    del ga, gb, outputs

    for _ in range(args.warmup):
        for arm in ARMS:
            step(arm)
    per_step = {a: [] for a in ARMS}
    window_medians = {a: [] for a in ARMS}
    for w in range(args.windows):
        for arm in (ARMS if w % 2 == 0 else ARMS[::-1]):
            evs = [[torch.cuda.Event(enable_timing=True) for _ in range(2)] for _ in range(args.steps)]
            torch.cuda.synchronize(dev)
            for ev in evs:
                step(arm, ev)
            torch.cuda.synchronize(dev)
            t = [ev[0].elapsed_time(ev[1]) for ev in evs]
            per_step[arm] += t
            window_medians[arm].append(statistics.median(t))

    kernels = {}
    for arm in ARMS:
        ops.KERNEL_EVENTS = {}
        try:
            for _ in range(args.kernel_steps):
                step(arm)
            torch.cuda.synchronize(dev)
            kernels[arm] = {k: dict(ms=round(statistics.median(a.elapsed_time(b) for a, b in v), 4), calls_per_step=len(v) / args.kernel_steps)
                            for k, v in ops.KERNEL_EVENTS.items() if v}
        finally:
            ops.KERNEL_EVENTS = None

    res = dict(device=torch.cuda.get_device_name(dev), B=B, N=N, H=H, W=W, steps_per_arm=args.steps * args.windows,
               gradients_fused_vs_unfused=agree, kernels=kernels)
    for arm in ARMS:
        wm = window_medians[arm]
        res[arm] = dict(ms=round(statistics.median(per_step[arm]), 4), window_medians_ms=[round(t, 4) for t in wm],
                        spread_ms=round(max(wm) - min(wm), 4))
    diff = res["unfused"]["ms"] - res["fused"]["ms"]
    spread = max(res["unfused"]["spread_ms"], res["fused"]["spread_ms"])
    res["unfused_minus_fused_ms"] = round(diff, 4)
    res["verdict"] = ("fused is faster beyond the spread" if diff > spread else
                      "fused is slower beyond the spread" if -diff > spread else "no difference beyond the spread")
    print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    if args.md:
        lines = ["# Tail link on the row form: fused against unfused", "",
                 "`scripts/bench_tail_link_rows.py --steps %d --windows %d` on %s: `fused_plane_geometry` + `fused_decoder_tail` +"
                 % (args.steps, args.windows, res["device"]),
                 "`plane_sweep_disp`, forward + backward, B = %d, %dx%d, %d + %d planes (horizon inside the crop), mixture, fp32."
                 % (B, H, W, NL, NX),
                 "Device events around every step, the arms alternating in one process; median over the %d steps of an arm, spread ="
                 % res["steps_per_arm"],
                 "max - min of the arm's %d window medians.  unfused (`fuse_sweep_backward=False`) is the behaviour before the row-form"
                 % args.windows,
                 "link and the yardstick.", "",
                 "| arm | step, ms | spread of the window medians, ms |", "|---|---|---|"]
        for arm in ARMS:
            lines.append("| %s | %.4f | %.4f |" % (arm, res[arm]["ms"], res[arm]["spread_ms"]))
        lines += ["", "unfused - fused = %.4f ms: **%s**." % (diff, res["verdict"]), "",
                  "Gradients of the two arms (conv outputs, plane residual), max |a - b| / max |a|: %s." % ", ".join("%.1e" % e for e in agree),
                  "", "Per C-ABI call (`ops.KERNEL_EVENTS`, a pass of its own of %d steps per arm; median ms, calls per step):" % args.kernel_steps,
                  "", "| call | unfused | fused |", "|---|---|---|"]
        for k in sorted(set(kernels["unfused"]) | set(kernels["fused"])):
            cell = lambda a: ("%.4f (%g)" % (kernels[a][k]["ms"], kernels[a][k]["calls_per_step"])) if k in kernels[a] else "-"  # noqa: E731
            lines.append("| %s | %s | %s |" % (k, cell("unfused"), cell("fused")))
        os.makedirs(os.path.dirname(os.path.abspath(args.md)), exist_ok=True)
        with open(args.md, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
