"""The fused pose path against the same chain as torch operators on the device, in one process.

From the pose decoder's last conv output ``[B,6,h,w]`` and ``inputs["grid"]`` to ``Rt`` (reference networks/pose_net.py:148-155,
layers.py:17-92, trainer.py:386-400):
  (a) fused  ``ops.pose_tail``: one launch forward, one backward (pd_pose_tail.hip);
  (b) torch  the chain operator by operator as the reference states it: two means, scale, view and slices; norm, divide, sin, cos,
             the element-wise products, nine indexed stores into a zero tensor; the translation matrix, transpose / negate, a 4x4
             matmul; ``Rc`` from indexed reads of the grid, ``eye``, ``repeat``, a column store; ``torch.inverse``, two matmuls into
             a ``zeros_like``.  A bf16 conv output is widened first (``.float()``).
B = 8; hw = 6 x 20 (192 x 640) and 12 x 40 (384 x 1280); fp32 and bf16 conv outputs; forward alone (``torch.no_grad``) and forward +
backward (upstream gradient on ``Rt`` ~ randn, made once); and ``pair``: the novel frames -1 and +1 of the mono step, two calls on two
conv outputs, forward + backward.  The arms alternate in windows of --steps calls (--windows rounds, the order reversed every other
round); every call is timed with device events; reported are the median over all calls of an arm and the spread of its window medians.

    python scripts/bench_pose_tail.py [--steps 20 --windows 8] [--out pose_tail.json --md profiles/pose_tail.md]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ARMS = ("fused", "torch")


def torch_chain(out, grid, invert):
    """The reference's chain with its operator sequence (fp32): every assignment below is one launch or one view there too."""
    import torch
    dev = out.device
    pooled = 0.01 * out.float().mean(3).mean(2).view(-1, 1, 1, 6)
    axisangle, translation = pooled[..., :3], pooled[..., 3:]
    vec, shift = axisangle[:, 0], translation[:, 0].clone()
    # axis-angle -> rotation, nine indexed stores into a zero [B,4,4]
    angle = torch.norm(vec, 2, 2, True)
    axis = vec / (angle + 1e-7)
    cos_a, sin_a = torch.cos(angle), torch.sin(angle)
    versine = 1 - cos_a
    u = [axis[..., k].unsqueeze(1) for k in range(3)]
    us = [c * sin_a for c in u]
    uv = [c * versine for c in u]
    cross = {(0, 1): u[0] * uv[1], (1, 2): u[1] * uv[2], (0, 2): u[2] * uv[0]}
    rot = torch.zeros((vec.shape[0], 4, 4)).to(device=dev)
    for k in range(3):
        rot[:, k, k] = torch.squeeze(u[k] * uv[k] + cos_a)
    for (i, j), sign in (((0, 1), -1), ((0, 2), 1), ((1, 2), -1)):
        third = us[3 - i - j]
        rot[:, i, j] = torch.squeeze(cross[(i, j)] + third if sign > 0 else cross[(i, j)] - third)
        rot[:, j, i] = torch.squeeze(cross[(i, j)] - third if sign > 0 else cross[(i, j)] + third)
    rot[:, 3, 3] = 1
    if invert:
        rot = rot.transpose(1, 2)
        shift *= -1
    # translation matrix: four diagonal stores and a column store into a zero [B,4,4], then the 4x4 product
    move = torch.zeros(shift.shape[0], 4, 4).to(device=dev)
    for k in range(4):
        move[:, k, k] = 1
    move[:, :3, 3, None] = shift.contiguous().view(-1, 3, 1)
    Rt = torch.matmul(rot, move) if invert else torch.matmul(move, rot)
    # Rc from the grid's corners, the conjugation through torch.inverse into a zeros_like
    left, right, top, bottom = grid[:, 0, 0, 0], grid[:, 0, 0, -1], grid[:, 1, 0, 0], grid[:, 1, -1, 0]
    centre_x, centre_y, half_width = (right + left) / 2., (bottom + top) / 2., (right - left) / 2.
    column = torch.stack([-centre_x / (2 * 0.58), -centre_y / (2 * 1.92), half_width], dim=1)
    Rc = torch.eye(3).to(dev)[None].repeat(column.shape[0], 1, 1)
    Rc[:, :, 2] = column
    Rt_Rc = torch.zeros_like(Rt)
    Rt_Rc[:, :3, :3] = torch.matmul(Rc, torch.matmul(Rt[:, :3, :3], torch.inverse(Rc)))
    return axisangle, translation, Rc, Rt_Rc


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
    from planedepth_amd import ops
    from planedepth_amd.postprocess import crop_grid

    if not torch.cuda.is_available():
        raise SystemExit("bench_pose_tail.py measures on the GPU; none found")
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

    B = 8
    res = dict(device=torch.cuda.get_device_name(dev), B=B, calls_per_arm=args.steps * args.windows, cases={})
    for H, W in ((192, 640), (384, 1280)):
        h, w = H // 32, W // 32
        crop = torch.tensor([[int(W * 1.2), int(H * 1.2), 7 + 3 * s, 5 + 2 * s] for s in range(B)], dtype=torch.int32, device=dev)
        grid = crop_grid(crop, H, W)
        for dtype in (torch.float32, torch.bfloat16):
            torch.manual_seed(h)
            xs = [(torch.randn(B, 6, h, w, device=dev) * 2 + torch.randn(B, 6, 1, 1, device=dev) * 4).to(dtype).requires_grad_(True)
                  for _ in range(2)]
            g_Rt = [torch.randn(B, 4, 4, device=dev) for _ in range(2)]
            frames = ((xs[0], True, g_Rt[0]), (xs[1], False, g_Rt[1]))   # novel frames -1 (inverted) and +1

            def fused(x, invert):
                return ops.pose_tail(x, grid, invert=invert)[3]

            def torch_arm(x, invert):
                return torch_chain(x, grid, invert)[3]

            def forward_only(fn, todo):
                def call():
                    with torch.no_grad():
                        for x, invert, _ in todo:
                            fn(x, invert)
                return call

            def with_backward(fn, todo):
                def call():
                    for x, invert, g in todo:
                        x.grad = None
                        fn(x, invert).backward(g)
                return call

            r = dict(H=H, W=W, hw=h * w, dtype=str(dtype).replace("torch.", ""))
            with torch.no_grad():
                r["distance"] = max(float((fused(x, inv) - torch_arm(x, inv)).abs().max()) for x, inv, _ in frames)
            grads = {}
            for arm, fn in (("fused", fused), ("torch", torch_arm)):
                with_backward(fn, frames[:1])()
                grads[arm] = xs[0].grad.float().clone()
            r["gradient_distance_rel"] = float((grads["fused"] - grads["torch"]).abs().max() / grads["torch"].abs().max())
            for mode, wrap, todo in (("fwd", forward_only, frames[:1]), ("fwd_bwd", with_backward, frames[:1]),
                                     ("pair_fwd_bwd", with_backward, frames)):
                calls = dict(fused=wrap(fused, todo), torch=wrap(torch_arm, todo))
                for _ in range(args.warmup):
                    for arm in ARMS:
                        calls[arm]()
                t = timed(calls, ARMS)
                diff, spread = t["torch"]["ms"] - t["fused"]["ms"], max(t["torch"]["spread_ms"], t["fused"]["spread_ms"])
                t.update(torch_over_fused=round(t["torch"]["ms"] / t["fused"]["ms"], 2),
                         verdict=("fused is faster beyond the spread" if diff > spread else
                                  "fused is slower beyond the spread" if -diff > spread else "no difference beyond the spread"))
                r[mode] = t
            res["cases"]["%dx%dx%d %s" % (B, h, w, r["dtype"])] = r
    print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    if args.md:
        lines = ["# Pose path: the fused operator against the reference's chain as torch operators on the device", "",
                 "`scripts/bench_pose_tail.py --steps %d --windows %d` on %s: the pose decoder's last conv output `[%d,6,h,w]` and"
                 % (args.steps, args.windows, res["device"], B),
                 "`inputs[\"grid\"]` into `Rt`.  fused = `ops.pose_tail` (one launch each way); torch = networks/pose_net.py:148-155,",
                 "layers.py:17-92 and trainer.py:386-400 operator by operator, `torch.inverse` included (a bf16 conv output widened first).",
                 "Device events around every call, the arms alternating in one process; median over the %d calls of an arm, spread = max - min"
                 % res["calls_per_arm"],
                 "of the arm's %d window medians.  fwd: under `torch.no_grad`; fwd + bwd: `backward` with an upstream gradient on `Rt` made once;"
                 % args.windows,
                 "pair: the novel frames -1 and +1 as the mono step issues them, two calls on two conv outputs, fwd + bwd.", "",
                 "| case | pass | fused, ms | spread | torch, ms | spread | torch / fused | verdict |", "|---|---|---|---|---|---|---|---|"]
        for name, r in res["cases"].items():
            for mode in ("fwd", "fwd_bwd", "pair_fwd_bwd"):
                t = r[mode]
                lines.append("| %s | %s | %.4f | %.4f | %.4f | %.4f | %.2f | %s |"
                             % (name, mode.replace("_fwd_bwd", ": fwd + bwd").replace("fwd_bwd", "fwd + bwd"), t["fused"]["ms"],
                                t["fused"]["spread_ms"], t["torch"]["ms"], t["torch"]["spread_ms"], t["torch_over_fused"], t["verdict"]))
        lines += ["", "| case | max distance of the arms' Rt | of their gradients (relative to the largest) |", "|---|---|---|"]
        for name, r in res["cases"].items():
            lines.append("| %s | %.2e | %.2e |" % (name, r["distance"], r["gradient_distance_rel"]))
        lines += ["", "Both arms' times include their host share (the Python of the operators, the allocations, the autograd engine): with",
                  "kernels this small the call is paced by the host issuing launches, which is what the fused operator removes.  This script",
                  "does not separate the kernels' time from the host's."]
        os.makedirs(os.path.dirname(os.path.abspath(args.md)), exist_ok=True)
        with open(args.md, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
