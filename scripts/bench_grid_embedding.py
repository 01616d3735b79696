"""The fused grid embedding pyramid against the reference's statements as torch ops on the device, in one process.

From ``inputs["grid"]`` ``[B,2,H,W]`` and an ``epconv`` with ``num_ep = 8`` to the embedding at the decoder's levels:
  (a) fused  ``ops.fused_grid_embedding``: one launch forward (the embedding at the four taps of each output pixel), one kernel plus
             the partials' reduction backward; nothing of the size [B,.,H,W] is written or kept;
  (b) torch  networks/depth_decoder.py:123-139 as it stands: ``epconv(grid)`` on the full grid (Conv2d(2,16,1), in-place ELU,
             Conv2d(16,8,1), in-place ELU), then one ``F.interpolate(bilinear, align_corners=True)`` per level.
B = 8 at 192x640 and B = 4 at 384x1280; the DepthDecoder's five levels (H/32 .. H/2) and the PoseDecoder's single level (H/32);
forward alone (``torch.no_grad``) and forward + backward (upstream gradients ~ randn, made once).  The arms alternate in windows of
--steps calls (--windows rounds, the order reversed every other round); every call is timed with device events; reported are the
median over all calls of an arm and the spread of its window medians.  Peak allocated bytes of one forward + backward of each arm
(``torch.cuda.max_memory_allocated`` above what was allocated before the call), and the rate of a plain device copy of 256 MiB in the
same run as the yardstick for the fused forward's algorithmic bytes (the levels written once, the grid read once).

    python scripts/bench_grid_embedding.py [--steps 20 --windows 8] [--out grid_embedding.json --md profiles/grid_embedding.md]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ARMS = ("fused", "torch")
NUM_EP = 8


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
    import torch
    import torch.nn.functional as F
    from planedepth_amd import ops
    from planedepth_amd.postprocess import crop_grid

    if not torch.cuda.is_available():
        raise SystemExit("bench_grid_embedding.py measures on the GPU; none found")
    dev = torch.device("cuda:0")

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

    def peak_bytes(call):
        torch.cuda.synchronize(dev)
        before = torch.cuda.memory_allocated(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        call()
        torch.cuda.synchronize(dev)
        return torch.cuda.max_memory_allocated(dev) - before

    res = dict(device=torch.cuda.get_device_name(dev), num_ep=NUM_EP, calls_per_arm=args.steps * args.windows, cases={})
    a, b = torch.empty(64 << 20, device=dev), torch.empty(64 << 20, device=dev)
    for _ in range(args.warmup):
        b.copy_(a)
    copy = timed({"copy": lambda: b.copy_(a)}, ("copy",))["copy"]
    copy_gbs = 2 * a.numel() * 4 / copy["ms"] / 1e6
    res["copy"] = dict(copy, mib=256, gb_per_s=round(copy_gbs, 1))
    del a, b

    for B, H, W in ((8, 192, 640), (4, 384, 1280)):
        # crop windows of a 1.2x resize, every other sample flipped as add_flip_right_inputs flips it
        crop = torch.tensor([[int(W * 1.2), int(H * 1.2), 7 + 3 * s, 5 + 2 * s] for s in range(B)], dtype=torch.int32, device=dev)
        grid = crop_grid(crop, H, W)
        grid[1::2, 0] = -grid[1::2, 0].flip(-1)
        torch.manual_seed(B)
        epconv = torch.nn.Sequential(torch.nn.Conv2d(2, 16, kernel_size=1, stride=1, padding=0, bias=True), torch.nn.ELU(inplace=True),
                                     torch.nn.Conv2d(16, NUM_EP, kernel_size=1, stride=1, padding=0, bias=True),
                                     torch.nn.ELU(inplace=True)).to(dev)
        decoder = tuple((H >> k, W >> k) for k in range(5, 0, -1))
        for name, sizes in (("decoder", decoder), ("pose", decoder[:1])):
            g_levels = [torch.randn(B, NUM_EP, h, w, device=dev) for h, w in sizes]

            def fused():
                return ops.fused_grid_embedding(epconv, grid, sizes)

            def torch_arm():
                grids_ep = epconv(grid)
                return [F.interpolate(grids_ep, size=s, align_corners=True, mode="bilinear") for s in sizes]

            def with_backward(fn):
                def call():
                    for p in epconv.parameters():
                        p.grad = None
                    torch.autograd.backward(fn(), g_levels)
                return call

            def forward_only(fn):
                def call():
                    with torch.no_grad():
                        return fn()
                return call

            r = dict(B=B, H=H, W=W, sizes=[list(s) for s in sizes])
            with torch.no_grad():
                x, y = fused(), torch_arm()
                r["distance"] = max(float((p - q).abs().max()) for p, q in zip(x, y))
                del x, y
            grads = {}
            for arm, fn in (("fused", fused), ("torch", torch_arm)):
                with_backward(fn)()
                grads[arm] = [p.grad.clone() for p in epconv.parameters()]
            r["gradient_distance_rel"] = max(float((p - q).abs().max() / q.abs().max()) for p, q in zip(grads["fused"], grads["torch"]))
            for mode, wrap in (("fwd", forward_only), ("fwd_bwd", with_backward)):
                calls = dict(fused=wrap(fused), torch=wrap(torch_arm))
                for _ in range(args.warmup):
                    for arm in ARMS:
                        calls[arm]()
                t = timed(calls, ARMS)
                diff, spread = t["torch"]["ms"] - t["fused"]["ms"], max(t["torch"]["spread_ms"], t["fused"]["spread_ms"])
                t.update(torch_over_fused=round(t["torch"]["ms"] / t["fused"]["ms"], 2),
                         verdict=("fused is faster beyond the spread" if diff > spread else
                                  "fused is slower beyond the spread" if -diff > spread else "no difference beyond the spread"))
                r[mode] = t
            r["peak_bytes"] = {arm: peak_bytes(with_backward(fn)) for arm, fn in (("fused", fused), ("torch", torch_arm))}
            for p in epconv.parameters():
                p.grad = None
            written, read = 4 * B * NUM_EP * sum(h * w for h, w in sizes), 4 * B * 2 * H * W
            gbs = (written + read) / r["fwd"]["fused"]["ms"] / 1e6
            r["fused_fwd_bytes"] = dict(written=written, read=read, gb_per_s=round(gbs, 1), share_of_copy_rate=round(gbs / copy_gbs, 4))
            res["cases"]["%dx%dx%d %s" % (B, H, W, name)] = r
    print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    if args.md:
        lines = ["# Grid embedding pyramid: the fused operator against the reference's statements on the device", "",
                 "`scripts/bench_grid_embedding.py --steps %d --windows %d` on %s: `inputs[\"grid\"]` `[B,2,H,W]` and an `epconv` with"
                 % (args.steps, args.windows, res["device"]),
                 "`num_ep = %d` into the embedding at the DepthDecoder's five levels (H/32 .. H/2) or the PoseDecoder's one (H/32).  fused ="
                 % NUM_EP,
                 "`ops.fused_grid_embedding` (one launch forward; one kernel and the partials' reduction backward); torch = `epconv(grid)` on the",
                 "full grid and one `F.interpolate(bilinear, align_corners=True)` per level, as networks/depth_decoder.py:123-139 states it.",
                 "Device events around every call, the arms alternating in one process; median over the %d calls of an arm, spread = max - min"
                 % res["calls_per_arm"],
                 "of the arm's %d window medians.  fwd: under `torch.no_grad`; fwd + bwd: `torch.autograd.backward` with upstream gradients made"
                 % args.windows,
                 "once.  Peak: `torch.cuda.max_memory_allocated` of one fwd + bwd above what was allocated before it.", "",
                 "Copy rate of this run, a 256 MiB device-to-device `copy_`, read + written bytes over its median time: %.0f GB/s (%.4f ms,"
                 % (res["copy"]["gb_per_s"], res["copy"]["ms"]),
                 "spread %.4f ms)." % res["copy"]["spread_ms"], "",
                 "| case | pass | fused, ms | spread | torch, ms | spread | torch / fused | verdict |", "|---|---|---|---|---|---|---|---|"]
        for name, r in res["cases"].items():
            for mode in ("fwd", "fwd_bwd"):
                t = r[mode]
                lines.append("| %s | %s | %.4f | %.4f | %.4f | %.4f | %.2f | %s |"
                             % (name, mode.replace("_", " + "), t["fused"]["ms"], t["fused"]["spread_ms"], t["torch"]["ms"],
                                t["torch"]["spread_ms"], t["torch_over_fused"], t["verdict"]))
        lines += ["", "| case | peak bytes fused | peak bytes torch | fused fwd: bytes written | read | GB/s | share of the copy rate | "
                  "max distance of the arms' levels | of their gradients (relative to the largest) |", "|---|---|---|---|---|---|---|---|---|"]
        for name, r in res["cases"].items():
            fb = r["fused_fwd_bytes"]
            lines.append("| %s | %d | %d | %d | %d | %.0f | %.4f | %.2e | %.2e |"
                         % (name, r["peak_bytes"]["fused"], r["peak_bytes"]["torch"], fb["written"], fb["read"], fb["gb_per_s"],
                            fb["share_of_copy_rate"], r["distance"], r["gradient_distance_rel"]))
        lines += ["", "The fused call's times include its host share (packing the four parameters, the allocations, the ctypes calls, the",
                  "autograd engine); the share of the copy rate says how far the call is from being paced by its bytes, not how well the",
                  "kernel streams.  This script does not separate the kernels' time from the host's."]
        os.makedirs(os.path.dirname(os.path.abspath(args.md)), exist_ok=True)
        with open(args.md, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
