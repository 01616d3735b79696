"""Novel views at arbitrary camera poses: ``ops.render_poses`` against the only route that existed before it, in one process.

From the conv outputs, the planes and the source image to V views, one per 6-DoF pose:
  (a) parent   ``ops.decoder_tail`` under ``no_grad`` (writes logits / sigma [B,N,H,W]), then one ``ops.plane_sweep_homography``
               forward per view with the source image standing in as target (it also writes a loss map and a stash; bf16 conv
               outputs are widened first: the per-plane homography kernels read fp32);
  (b) fused    ``ops.render_poses``: two launches, nothing [B,N,H,W]-sized written.
Shapes, all B = 8, 192x640, mixture: 49 xy planes without a mask; 49 + 14 planes (xz planes with their row mask) from
``ops.plane_geometry`` with the horizon inside the crop; fp32 and bf16 conv outputs; V = 1, 2 and 4; poses
``synthetic.small_pose(rot=0.02, trans=0.05)``.
The arms alternate in windows of --steps calls (--windows rounds, the order reversed every other round); every call is timed with
device events, and the median over all calls of an arm and the spread of its window medians (max - min) are reported, next to
the rate of a plain device copy measured in the same run and the peak allocated bytes of one call of each arm.  No ratio is
expected in advance: the verdict column says whether the fused call is faster beyond the spread, and says so where it is not.
Before anything is timed the first view of the two arms is compared (2 * FWD_CAP = 1e-3, tests/test_render_poses.py; fp32 only).

    python scripts/bench_render_poses.py [--steps 20 --windows 8] [--out render_poses.json --md profiles/render_poses.md]

``--md FILE`` rewrites the file from its "## Timings" heading on and keeps what stands above it (the parity figures).
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
HEADING = "## Timings"


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
        raise SystemExit("bench_render_poses.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    B, H, W, NL, NX = 8, 192, 640, 49, 14
    g = torch.Generator().manual_seed(1234)
    inputs = synthetic.kitti_like_inputs(B, H, W, seed=3)
    grid = inputs["grid"].to(dev)
    K, inv_K = inputs["K"].to(dev), inputs["inv_K"].to(dev)
    image = torch.rand(B, 3, H, W, generator=g).to(dev)
    with torch.no_grad():
        dl_rows, pm_rows, distance, norm = ops.plane_geometry(grid, (torch.rand(B, NL + NX, generator=g) - 0.5).to(dev), no_levels=NL,
                                                              xz_levels=NX, disp_min=2.0, disp_max=300.0, xz_min=0.1852, xz_max=0.3704)
    rows = ops._rows_of(pm_rows)[:, NL:]
    assert bool((rows == 0).any()) and bool((rows == 1).any()), "the horizon of the ground planes is not inside the crop"
    distance, norm = distance.contiguous(), norm.expand(B, NL + NX, 3).contiguous()
    dl49 = ops._rows_of(dl_rows)[:, :NL, :1, None].expand(B, NL, H, W)
    T = torch.stack([synthetic.small_pose(g, B, rot=0.02, trans=0.05) for _ in range(max(VIEWS))], 1).to(dev)   # [B,4,4,4]
    rl = (torch.randn(B, NL + NX, H, W, generator=g) * 2.5).to(dev)
    rs = (torch.randn(B, NL + NX, H, W, generator=g) * 3 - 1).to(dev)
    rl49, rs49 = rl[:, :NL].contiguous(), rs[:, :NL].contiguous()
    d49, n49 = distance[:, :NL].contiguous(), norm[:, :NL].contiguous()

    def arms(a, s, pm, dl, d, n, V):
        Tv = T[:, :V].contiguous()
        per_view = [T[:, v].contiguous() for v in range(V)]

        def parent():
            logits, sigma, _, _, _ = ops.decoder_tail(a, s, pm, dl)
            return [ops.plane_sweep_homography(image, image, logits, sigma, d, n, per_view[v], K, inv_K)[0] for v in range(V)]

        def fused():
            return ops.render_poses(a, s, pm, d, n, image, Tv, K, inv_K).rgb
        return parent, fused

    shapes = {
        "N=49 xy fp32": (NL, rl49, rs49, None, dl49, d49, n49),
        "N=49 xy bf16": (NL, rl49.bfloat16(), rs49.bfloat16(), None, dl49, d49, n49),
        "N=63 xy+xz fp32": (NL + NX, rl, rs, pm_rows, dl_rows, distance, norm),
        "N=63 xy+xz bf16": (NL + NX, rl.bfloat16(), rs.bfloat16(), pm_rows, dl_rows, distance, norm),
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

    def peak_bytes(fn):
        torch.cuda.synchronize(dev)
        before = torch.cuda.memory_allocated(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        out = fn()
        torch.cuda.synchronize(dev)
        peak = torch.cuda.max_memory_allocated(dev) - before
        del out
        return int(peak)

    # the copy rate of this run: a device copy of one fp32 conv output (read + write)
    src, dst = rl, torch.empty_like(rl)
    timed(lambda: dst.copy_(src), 5)
    copy_ms = statistics.median(timed(lambda: dst.copy_(src), 40))
    copy_gbs = 2 * src.numel() * 4 / copy_ms / 1e6
    del dst

    res = dict(device=torch.cuda.get_device_name(dev), B=B, H=H, W=W, calls_per_arm=args.steps * args.windows,
               copy_gb_per_s=round(copy_gbs, 1), configs={})
    with torch.no_grad():
        for name, (N, a, s, pm, dl, d, n) in shapes.items():
            for V in VIEWS:
                calls = dict(zip(ARMS, arms(a, s, pm, dl, d, n, V)))
                p, f = calls["parent"](), calls["fused"]()
                err = float((p[0] - f[:, 0]).abs().max() / p[0].abs().max())
                assert a.dtype != torch.float32 or err <= 1e-3, "%s V=%d: the first view of the two arms differs by %.3g" % (name, V, err)
                del p, f
                for _ in range(args.warmup):
                    for arm in ARMS:
                        calls[arm]()
                r = dict(N=N, V=V, first_view_rel_diff=err, plane_tensor_bytes=B * N * H * W * 4)
                peaks = {arm: peak_bytes(calls[arm]) for arm in ARMS}
                per_call = {k: [] for k in ARMS}
                window_medians = {k: [] for k in ARMS}
                for w in range(args.windows):
                    for arm in (ARMS if w % 2 == 0 else ARMS[::-1]):
                        t = timed(calls[arm], args.steps)
                        per_call[arm] += t
                        window_medians[arm].append(statistics.median(t))
                for arm in ARMS:
                    wm = window_medians[arm]
                    r[arm] = dict(ms=round(statistics.median(per_call[arm]), 4), spread_ms=round(max(wm) - min(wm), 4),
                                  window_medians_ms=[round(t, 4) for t in wm], peak_bytes=peaks[arm])
                diff = r["parent"]["ms"] - r["fused"]["ms"]
                spread = max(r["parent"]["spread_ms"], r["fused"]["spread_ms"])
                r["parent_minus_fused_ms"] = round(diff, 4)
                r["time_ratio"] = round(r["fused"]["ms"] / r["parent"]["ms"], 3)
                r["verdict"] = ("fused is faster beyond the spread" if diff > spread else
                                "fused is SLOWER beyond the spread" if -diff > spread else "no difference beyond the spread")
                res["configs"]["%s V=%d" % (name, V)] = r
    print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    if args.md:
        head = ""
        if os.path.isfile(args.md):
            with open(args.md) as f:
                head = f.read().split(HEADING)[0]
        lines = [HEADING, "",
                 "`scripts/bench_render_poses.py --steps %d --windows %d` on %s: from the decoder's conv outputs, the planes and the"
                 % (args.steps, args.windows, res["device"]),
                 "source image to V views at `small_pose(rot=0.02, trans=0.05)`, B = %d, %dx%d, mixture.  parent = `ops.decoder_tail`" % (B, H, W),
                 "under `torch.no_grad()`, then one `ops.plane_sweep_homography` forward per view with the source image standing in as",
                 "target (the only route before); fused = `ops.render_poses`.  Device events around every call (allocations and launches",
                 "included), the arms alternating in one process; median over the %d calls of an arm, spread = max - min of the arm's"
                 % res["calls_per_arm"],
                 "%d window medians.  Copy rate of the same run (a device copy of one fp32 conv output, read + write): %.0f GB/s."
                 % (args.windows, res["copy_gb_per_s"]),
                 "Peak = peak allocated bytes of one call beyond what was allocated before it, in MB; one [B,N,H,W] fp32 tensor is",
                 "%.1f MB at N = 49 and %.1f MB at N = 63." % (B * NL * H * W * 4 / 1e6, B * (NL + NX) * H * W * 4 / 1e6), "",
                 "| configuration | parent, ms | spread | fused, ms | spread | fused / parent | parent peak, MB | fused peak, MB | verdict |",
                 "|---|---|---|---|---|---|---|---|---|"]
        for name, r in res["configs"].items():
            lines.append("| %s | %.4f | %.4f | %.4f | %.4f | %.3f | %.1f | %.1f | %s |" % (
                name, r["parent"]["ms"], r["parent"]["spread_ms"], r["fused"]["ms"], r["fused"]["spread_ms"], r["time_ratio"],
                r["parent"]["peak_bytes"] / 1e6, r["fused"]["peak_bytes"] / 1e6, r["verdict"]))
        os.makedirs(os.path.dirname(os.path.abspath(args.md)), exist_ok=True)
        with open(args.md, "w") as f:
            f.write(head + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
