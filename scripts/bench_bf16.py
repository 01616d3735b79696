"""fp32 against bf16 logits / sigma (PD_LOGITS_BF16) on the sweep's hot path, in one process.

Each step is the fused sweep forward (rgb_rec, ph_map, ph_map.mean()) and its backward into logits, sigma and the plane
disparities, as bench.py's headline leg times it.  The fp32 and the bf16 step run in interleaved windows of --steps steps
each (--windows pairs); the medians are reported per shape with images/s, the algorithmic bytes per image of the [B,N,H,W]
traffic plus colour — (6N+18)*HW*4 in fp32, (3N+18)*HW*4 in bf16 — and the fraction of 8 TB/s they reach.

Shapes: BASELINE configs[1] (B = 8, 192x640, N = 49, mixture, per-plane disparities, target "r"); N = 63 with xz rows and
automask; and one fallback route (a per-pixel padding mask: the bf16 tensors are cast to fp32, so the cast shows up).

    python scripts/bench_bf16.py [--steps 20 --windows 7] [--out profiles/bf16_bench.json]
Kernel times: run it under rocprofv3 --kernel-trace --stats (a separate run; --windows 2 keeps the trace small).
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import __graft_entry__
    __graft_entry__.build()
    import torch
    from planedepth_amd import _capi as C
    from planedepth_amd import _state as S
    from planedepth_amd import ops
    from planedepth_amd.synthetic import build_case

    dev = torch.device("cuda:0")
    torch.backends.cudnn.benchmark = False
    shapes = [
        dict(name="configs[1] N=49 mixture", N=49, n_xz=0, automask=False, mask="none"),
        dict(name="N=63 xz rows + automask", N=63, n_xz=14, automask=True, mask="rows"),
        dict(name="fallback: per-pixel mask N=49", N=49, n_xz=0, automask=False, mask="pixel"),
    ]
    B, H, W = 8, 192, 640
    results = []
    for sh in shapes:
        N = sh["N"]
        case = build_case(B=B, N=N, H=H, W=W, seed=1234, disp_min=2.0, disp_max=300.0, sigma_interior=True, n_xz=sh["n_xz"])
        c = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in case.items()}
        disp_pp = c["disp_pp"].clone().requires_grad_(True)
        mask = None if sh["mask"] == "none" else c["padding_mask"]
        g_rgb = c["g_rgb_rec"]
        one = torch.ones((), device=dev)
        leaves = {}
        for dt in (torch.float32, torch.bfloat16):
            leaves[dt] = (c["logits"].to(dt).requires_grad_(True), c["sigma"].to(dt).requires_grad_(True))

        def step(dt):
            lg, sg = leaves[dt]
            for t in (lg, sg):   # a training step has new logits every time: the fallback's fp32 copy is not reused
                t.__dict__.pop("_pd_f32", None)
            disp = disp_pp.expand(-1, -1, H, W) * c["row_gain"] if sh["n_xz"] else disp_pp.expand(-1, -1, H, W)
            rgb, ph, ph_mean = ops.plane_sweep_disp(c["color_l"], c["color_r"], lg, sg, disp, mask, target_side="r",
                                                    use_mixture_loss=True, automask=sh["automask"],
                                                    row_uniform=sh["mask"] != "pixel", return_mean=True)
            flags = S.LAST_SWEEP_FLAGS
            torch.autograd.grad([ph_mean, rgb], [lg, sg, disp_pp], [one, g_rgb])
            return flags

        flags = {dt: step(dt) for dt in leaves}
        for _ in range(args.warmup):
            for dt in leaves:
                step(dt)
        times = {dt: [] for dt in leaves}
        for w in range(args.windows):
            order = list(leaves) if w % 2 == 0 else list(leaves)[::-1]
            for dt in order:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize(dev)
                e0.record()
                for _ in range(args.steps):
                    step(dt)
                e1.record()
                torch.cuda.synchronize(dev)
                times[dt].append(e0.elapsed_time(e1) / args.steps)
        HW = H * W
        row = dict(shape=sh["name"], B=B, N=N, H=H, W=W)
        for dt, tag in ((torch.float32, "fp32"), (torch.bfloat16, "bf16")):
            ms = statistics.median(times[dt])
            native = bool(flags[dt] & C.PD_LOGITS_BF16)
            nbytes = ((3 * N + 18) if native else (6 * N + 18)) * HW * 4
            row[tag] = dict(ms_per_step=round(ms, 4), images_per_s=round(B / (ms * 1e-3), 1), native_bf16=native,
                            algorithmic_bytes_per_image=nbytes, fraction_of_8TBps=round(nbytes * B / (ms * 1e-3) / 8e12, 3),
                            windows_ms=[round(t, 4) for t in times[dt]])
        row["bf16_over_fp32"] = round(row["bf16"]["ms_per_step"] / row["fp32"]["ms_per_step"], 3)
        results.append(row)
        print(json.dumps({k: (v if k not in ("fp32", "bf16") else {q: v[q] for q in v if q != "windows_ms"})
                          for k, v in row.items()}), flush=True)
    out = dict(device=torch.cuda.get_device_name(dev), steps=args.steps, windows=args.windows, results=results)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
