"""The inference tails against the training tails under ``torch.no_grad()``, in one process.

From the conv outputs to ``disp`` / ``depth`` / the confidence a depth network's user reads:
  (a) training   ``ops.decoder_tail`` / ``ops.plade_tail`` under ``no_grad`` — the only route before the inference tails existed, and
                 the yardstick.  It writes sigma (+ logits with a mask; logits, dists and sigma for PladeNet) and a stash;
  (b) inference  ``ops.decoder_tail_inference`` / ``ops.plade_tail_inference`` (--want: default depth,confidence): nothing
                 [B,N,H,W]-sized is written.
Shapes, all B = 8, 192x640, mixture: 49 planes per plane without a mask; 49 + 14 planes in the row form from
``ops.plane_geometry`` with the horizon inside the crop, fp32 and bf16; the PladeNet tail at 49 planes.
The arms alternate in windows of --steps calls (--windows rounds, the order reversed every other round); every call is timed
with device events, and the median over all calls of an arm and the spread of its window medians are reported, next to the
algorithmic bytes per pixel computed from the shapes.  After the timed windows a separate pass collects the time of the one C-ABI
call inside each operator (``ops.KERNEL_EVENTS``: an event pair around the launch; it adds host work, so it stays out of the call
timing): the operator's call time includes its allocations and the host's share, the launch time does not.  Before anything is
timed ``disp`` of the two arms is compared bit for bit.

    python scripts/bench_infer_tail.py [--steps 20 --windows 8] [--out infer_tail.json --md profiles/infer_tail.md]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ARMS = ("training", "inference")
# hipcc -Rpass-analysis=kernel-resource-usage on the instantiations these shapes run (4 pixels per lane): VGPRs, waves / SIMD
RESOURCES = {
    "decoder N=49 per-plane fp32": ("tail_fwd_kernel<float,mix,nomask,4,0> 77 VGPRs, 6 waves", "tail_infer_kernel<float,mix,nomask,4,0> 60 VGPRs, 8 waves"),
    "decoder N=63 rows fp32": ("tail_fwd_kernel<float,mix,mask,4,rows> 77 VGPRs, 6 waves", "tail_infer_kernel<float,mix,mask,4,rows> 51 VGPRs, 8 waves"),
    "decoder N=63 rows bf16": ("tail_fwd_kernel<bf16,mix,mask,4,rows> 77 VGPRs, 6 waves", "tail_infer_kernel<bf16,mix,mask,4,rows> 47 VGPRs, 8 waves"),
    "plade N=49 fp32": ("plade_fwd_kernel<float,mix,4> 75 VGPRs, 6 waves", "plade_infer_kernel<float,mix,4> 61 VGPRs, 8 waves"),
}


def bytes_per_pixel_of(kind, N, st, mask, want):
    """Algorithmic bytes per pixel of (training, inference), from the shapes: ``st`` = bytes of a conv-output element; per-plane
    and row operands are [B,N] / [B,N,H] and do not count per pixel."""
    extra = 4 * sum(w in want for w in ("depth", "confidence", "plane_index", "disp_best"))
    if kind == "decoder":
        reads = 2 * N * st
        train = reads + N * st + (N * st if mask else 0) + 4 * 4           # sigma (+ logits), disp, depth, stash[2]
        infer = reads + 4 + extra + (8 if "layers" in want else 0)
    else:
        reads = (N - 1) * st + N * st + 4                                  # conv0, conv_sigma, ray_norm
        train = reads + 2 * N * st + (N - 1) * 4 + 3 * 4                   # logits, sigma, dists, disp, depth, stash
        infer = reads + 4 + extra + (4 if "layers" in want else 0)
    return train, infer


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--kernel-steps", type=int, default=20)
    ap.add_argument("--want", default="depth,confidence")
    ap.add_argument("--out", default=None)
    ap.add_argument("--md", default=None)
    args = ap.parse_args()
    if args.steps * args.windows < 50:
        ap.error("at least 50 calls per arm (--steps x --windows)")
    want = tuple(w for w in args.want.split(",") if w)

    import __graft_entry__
    __graft_entry__.build()
    import torch
    from planedepth_amd import ops, synthetic

    if not torch.cuda.is_available():
        raise SystemExit("bench_infer_tail.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    B, H, W, NL, NX = 8, 192, 640, 49, 14
    g = torch.Generator().manual_seed(1234)
    grid = synthetic.kitti_like_inputs(B, H, W, seed=3)["grid"].to(dev)
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
    rl48 = rl[:, :NL - 1].contiguous()
    rl_b, rs_b = rl.bfloat16(), rs.bfloat16()

    # name -> (kind, N, bytes per conv-output element, mask?, training call, inference call); both return (disp, depth)
    def decoder(a, s, pm, dl):
        return (lambda: ops.decoder_tail(a, s, pm, dl)[2:4]), (lambda: ops.decoder_tail_inference(a, s, pm, dl, want=want)[:2])
    cases = {
        "decoder N=49 per-plane fp32": ("decoder", NL, 4, False) + decoder(rl49, rs49, None, dl_plane),
        "decoder N=63 rows fp32": ("decoder", NL + NX, 4, True) + decoder(rl, rs, pm_rows, dl_rows),
        "decoder N=63 rows bf16": ("decoder", NL + NX, 2, True) + decoder(rl_b, rs_b, pm_rows, dl_rows),
        "plade N=49 fp32": ("plade", NL, 4, False, lambda: ops.plade_tail(rl48, rs49, dl_plane)[3:5],
                            lambda: ops.plade_tail_inference(rl48, rs49, dl_plane, want=want)[:2]),
    }

    res = dict(device=torch.cuda.get_device_name(dev), B=B, H=H, W=W, want=list(want), calls_per_arm=args.steps * args.windows,
               shapes={})
    with torch.no_grad():
        for name, (kind, N, st, mask, train, infer) in cases.items():
            calls = dict(training=train, inference=infer)
            a, b = train(), infer()
            assert torch.equal(a[0], b[0]), "%s: disp of the two arms differs" % name
            assert b[1] is None or torch.equal(a[1], b[1]), "%s: depth of the two arms differs" % name
            del a, b
            for _ in range(args.warmup):
                for arm in ARMS:
                    calls[arm]()
            per_call = {a: [] for a in ARMS}
            window_medians = {a: [] for a in ARMS}
            for w in range(args.windows):
                for arm in (ARMS if w % 2 == 0 else ARMS[::-1]):
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
            launch = {}
            for arm in ARMS:   # the C-ABI call alone (tail_fwd / tail_infer / plade_fwd / plade_infer)
                ops.KERNEL_EVENTS = {}
                try:
                    for _ in range(args.kernel_steps):
                        calls[arm]()
                    torch.cuda.synchronize(dev)
                    (pairs,) = ops.KERNEL_EVENTS.values()
                    launch[arm] = statistics.median(a.elapsed_time(b) for a, b in pairs)
                finally:
                    ops.KERNEL_EVENTS = None
            nbytes = dict(zip(ARMS, bytes_per_pixel_of(kind, N, st, mask, want)))
            r = dict(N=N, disp_bit_identical=True, resources=dict(zip(ARMS, RESOURCES[name])))
            for arm in ARMS:
                wm = window_medians[arm]
                ms = statistics.median(per_call[arm])
                r[arm] = dict(ms=round(ms, 4), window_medians_ms=[round(t, 4) for t in wm], spread_ms=round(max(wm) - min(wm), 4),
                              launch_ms=round(launch[arm], 4), bytes_per_pixel=nbytes[arm],
                              gb_per_s=round(nbytes[arm] * B * H * W / launch[arm] / 1e6, 1))
            diff = r["training"]["ms"] - r["inference"]["ms"]
            spread = max(r["training"]["spread_ms"], r["inference"]["spread_ms"])
            r["training_minus_inference_ms"] = round(diff, 4)
            r["time_ratio"] = round(r["inference"]["ms"] / r["training"]["ms"], 3)
            r["bytes_ratio"] = round(nbytes["inference"] / nbytes["training"], 3)
            r["verdict"] = ("inference is faster beyond the spread" if diff > spread else
                            "inference is slower beyond the spread" if -diff > spread else "no difference beyond the spread")
            res["shapes"][name] = r
    print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    if args.md:
        lines = ["# Inference tails against the training tails under no_grad", "",
                 "`scripts/bench_infer_tail.py --steps %d --windows %d --want %s` on %s: from the conv outputs to `disp` and"
                 % (args.steps, args.windows, args.want, res["device"]),
                 "%s, B = %d, %dx%d, mixture.  training = `ops.decoder_tail` / `ops.plade_tail` under `torch.no_grad()` (the only"
                 % (" / ".join("`%s`" % w for w in want) or "nothing else", B, H, W),
                 "route before the inference tails, and the yardstick); inference = `ops.decoder_tail_inference` /",
                 "`ops.plade_tail_inference`.  Device events around every call (operator included: allocations, one launch), the arms",
                 "alternating in one process; median over the %d calls of an arm, spread = max - min of the arm's %d window medians."
                 % (res["calls_per_arm"], args.windows),
                 "`disp` (and `depth`) of the two arms are bit-identical at every shape (checked before timing).", "",
                 "Algorithmic bytes per pixel are computed from the shapes: the conv outputs read once (N each, N-1 + N and the ray",
                 "length for PladeNet), per-plane and row operands not counted ([B,N] / [B,N,H]), plus what the arm writes — training:",
                 "sigma (+ logits with a mask; logits, sigma and dists for PladeNet), disp, depth and the stash; inference: disp and",
                 "the outputs asked for.", "",
                 "launch = the C-ABI call alone (`ops.KERNEL_EVENTS`, a pass of its own of %d calls per arm, median); GB/s = the algorithmic"
                 % args.kernel_steps,
                 "bytes over that time.", "",
                 "| shape | arm | call, ms | spread, ms | launch, ms | bytes / pixel | GB/s | kernel (VGPRs, waves / SIMD) |",
                 "|---|---|---|---|---|---|---|---|"]
        for name, r in res["shapes"].items():
            for arm in ARMS:
                lines.append("| %s | %s | %.4f | %.4f | %.4f | %d | %.0f | %s |" % (
                    name, arm, r[arm]["ms"], r[arm]["spread_ms"], r[arm]["launch_ms"], r[arm]["bytes_per_pixel"], r[arm]["gb_per_s"],
                    r["resources"][arm]))
        lines += ["", "| shape | inference / training, time | inference / training, bytes | verdict |", "|---|---|---|---|"]
        for name, r in res["shapes"].items():
            lines.append("| %s | %.3f | %.3f | %s |" % (name, r["time_ratio"], r["bytes_ratio"], r["verdict"]))
        f32, b16 = res["shapes"]["decoder N=63 rows fp32"]["inference"], res["shapes"]["decoder N=63 rows bf16"]["inference"]
        lines += ["", "Where the time ratio stays above the bytes ratio the inference kernel is no longer paced by bytes alone: at N = 63 in",
                  "the row form bf16 conv outputs take %.4f ms against %.4f ms with fp32 for %.2fx the bytes (%.0f against %.0f GB/s) — the"
                  % (b16["launch_ms"], f32["launch_ms"], b16["bytes_per_pixel"] / f32["bytes_per_pixel"], b16["gb_per_s"], f32["gb_per_s"]),
                  "per-plane arithmetic (two exponentials, the sigmoid's and the weight's divisions) is the same in both."]
        lines += ["", "Neither inference kernel spills (no scratch), and each runs at least as many waves per SIMD as the training forward",
                  "of the same instantiation (`hipcc -Rpass-analysis=kernel-resource-usage`, gfx950)."]
        os.makedirs(os.path.dirname(os.path.abspath(args.md)), exist_ok=True)
        with open(args.md, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
