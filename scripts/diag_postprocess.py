"""Per-call device time of the post-process operators at the benchmark shape (run once per PD_PP_SEG setting: the
library reads the switch once per process).  python scripts/diag_postprocess.py [--batch 4 --planes 49]

--ab name=path [name=path ...]: A/B of library builds on pd_post_process instead — the libraries are loaded side by side through
ctypes and called directly, interleaved round by round (--rounds windows of --iters calls each between two device events); per
library the median and the spread (min .. max) of the windows, and whether each later median lies inside the first one's spread
(--xz K: per-row disparities, PD_PP_DISP_ROWS).

--ab ... --check: every case of tests/test_post_process_routes.py's CASES table through the libraries on the same inputs —
pd_post_process (disp_pp, mask_novel) and pd_warp_softmax / pd_warp_sum for the four (sign, flip) combinations — compared on the
raw bits against the first library, which first runs twice and is compared with itself (the kernels have no atomics: a difference
there is the first library's own); exit 1 on any differing bit."""
import argparse
import ctypes
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from planedepth_amd import ops  # noqa: E402


def load_libs(specs):
    from planedepth_amd import _capi as C
    libs = []
    for spec in specs:
        name, _, path = spec.partition("=")
        libs.append((name, C.bind(ctypes.CDLL(path or C.LIB_PATH))))
    return libs


def check(a):
    """Every case of the route suite's table through the libraries on the same inputs, every output on the raw bits."""
    from planedepth_amd import _capi as C
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import test_post_process_routes as T
    libs, dev = load_libs(a.ab), torch.device("cuda:0")
    st = C.stream_handle(dev)

    def outputs(lib, c):
        z = T.inputs(c.name)
        f = lambda t: t.float().to(dev).contiguous()
        nan = lambda *shape: torch.full(shape, float("nan"), device=dev)
        B, N, H, W, fl = c.B, c.N, c.H, c.W, T.FLAG[c.form]
        logits, prob, disp = f(z["logits"]), f(z["prob"]), f(T.disp_fill(c.name, "real"))
        compact = f({"plane": z["lv"], "rows": z["rows"], "dense": z["dl"]}[c.form])   # the image's half comes first
        ws = nan(int(lib.pd_post_process_workspace_floats(B, N, H, W)) + 2)
        off = (1 if c.ws4 else 0) + (0 if ws.data_ptr() % 8 == 0 else 1)               # 8-byte aligned, or 4 (mod 8): the table's routes
        out = {"disp_pp": nan(B, 1, H, W), "mask_novel": nan(B, 1, H, W)}
        rc = lib.pd_post_process(B, N, H, W, fl, C.ptr(logits), C.ptr(prob), C.ptr(disp), C.ptr(compact),
                                 ctypes.c_void_p(ws.data_ptr() + 4 * off), C.ptr(out["disp_pp"]), C.ptr(out["mask_novel"]), st)
        assert rc == 0, lib.pd_last_error()
        for sign, flip in T.WARP_COMBOS:
            flf = fl | (C.PD_PP_FLIP_SRC if flip else 0)
            sm, su = nan(B, N, H, W), nan(B, 1, H, W)
            rc = lib.pd_warp_softmax(B, N, H, W, sign, flf, C.ptr(logits), C.ptr(compact), C.ptr(sm), st)
            assert rc == 0, lib.pd_last_error()
            rc = lib.pd_warp_sum(B, N, H, W, sign, flf, C.ptr(prob), C.ptr(compact), 1.0, C.ptr(su), st)
            assert rc == 0, lib.pd_last_error()
            out["warp_softmax %+d flip %d" % (sign, flip)], out["warp_sum %+d flip %d" % (sign, flip)] = sm, su
        torch.cuda.synchronize()
        return {k: v.view(torch.int32).cpu() for k, v in out.items()}

    report, bad = {}, 0
    for c in T.CASES:
        first = outputs(libs[0][1], c)
        arms = [(libs[0][0] + " again", outputs(libs[0][1], c))] + [(name, outputs(lib, c)) for name, lib in libs[1:]]
        report[c.name] = {}
        for name, got in arms:
            diff = {k: int((got[k] != first[k]).sum()) for k in first}
            report[c.name][name] = diff
            bad += sum(diff.values())
            print("%-16s %-14s vs %s: %d outputs, %d differing words%s" % (c.name, name, libs[0][0], len(diff), sum(diff.values()),
                  "".join("  %s: %d" % kv for kv in diff.items() if kv[1])))
    print("%d cases, %d differing 32-bit words in all" % (len(T.CASES), bad))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump({"libraries": [n for n, _ in libs], "differing_words": report, "total": bad}, fh, indent=1)
    return 1 if bad else 0


def ab(a, logits, prob, disp, dl):
    from planedepth_amd import _capi as C
    B, N, H, W = a.batch, a.planes, a.height, a.width
    libs = load_libs(a.ab)
    st = C.stream_handle(logits.device)
    # per-plane disparities [2B,N]; --xz: per-row ones [2B,N,H] (PD_PP_DISP_ROWS)
    lv, flags = (dl[:, :, :, 0].contiguous(), C.PD_PP_DISP_ROWS) if a.xz else (dl[:, :, 0, 0].contiguous(), 0)
    ws = torch.empty(max(int(l.pd_post_process_workspace_floats(B, N, H, W)) for _, l in libs), device=logits.device)
    dpp, mn = torch.empty(B, 1, H, W, device=logits.device), torch.empty(B, 1, H, W, device=logits.device)

    def call(lib):
        rc = lib.pd_post_process(B, N, H, W, flags, C.ptr(logits), C.ptr(prob), C.ptr(disp), C.ptr(lv), C.ptr(ws), C.ptr(dpp), C.ptr(mn), st)
        assert rc == 0, lib.pd_last_error()

    times = {name: [] for name, _ in libs}
    for _, lib in libs:
        for _ in range(10):
            call(lib)
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for name, lib in libs:
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(a.iters):
                call(lib)
            e.record()
            torch.cuda.synchronize()
            times[name].append(s.elapsed_time(e) / a.iters)
    med = lambda v: sorted(v)[len(v) // 2] if len(v) % 2 else 0.5 * (sorted(v)[len(v) // 2 - 1] + sorted(v)[len(v) // 2])
    out = {}
    print("pd_post_process %dx%dx%dx%d, ms per call over %d rounds of %d" % (B, N, H, W, a.rounds, a.iters))
    for name, _ in libs:
        t = times[name]
        out[name] = {"median_ms": med(t), "min_ms": min(t), "max_ms": max(t), "rounds": t}
        print("%-12s median %.4f  min %.4f  max %.4f" % (name, med(t), min(t), max(t)))
    first = out[libs[0][0]]
    for name, _ in libs[1:]:
        out[name]["inside_first_spread"] = first["min_ms"] <= out[name]["median_ms"] <= first["max_ms"]
        print("%-12s median %s %s's spread" % (name, "inside" if out[name]["inside_first_spread"] else "OUTSIDE", libs[0][0]))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump({"shape": [B, N, H, W], "results": out}, fh, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--planes", type=int, default=49)
    ap.add_argument("--height", type=int, default=192)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--iters", type=int, default=60)
    ap.add_argument("--xz", type=int, default=0, help="the last K planes get a disparity that grows with the row (ground planes): a [B,N,H,1] map expanded along x")
    ap.add_argument("--ab", nargs="+", default=None, help="name=path of library builds: A/B of pd_post_process, interleaved in this process")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--check", action="store_true", help="with --ab: compare the libraries' outputs on the raw bits instead (exit 1 on any difference)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.check:
        if not a.ab:
            ap.error("--check needs --ab")
        return check(a)
    B, N, H, W = a.batch, a.planes, a.height, a.width
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(5)
    logits = torch.randn(2 * B, N, H, W, generator=g).to(dev)
    prob = torch.softmax(torch.randn(2 * B, N, H, W, generator=g), 1).to(dev)
    lv = torch.arange(N, dtype=torch.float32)[None, :, None, None] + torch.rand(2 * B, N, 1, 1, generator=g) - 0.5
    dl = (300.0 * (2.0 / 300.0) ** (lv / (N - 1))).to(dev).expand(-1, -1, H, W)
    if a.xz:
        rows = dl[:, :, :, :1].clone()                                    # [2B,N,H,1]
        gain = torch.linspace(0.2, 3.0, H, device=dev).view(1, 1, H, 1)
        rows[:, N - a.xz:] = rows[:, N - a.xz:] * gain
        dl = rows.expand(-1, -1, -1, W)
    disp = (prob * dl).sum(1, True)
    if a.ab:
        return ab(a, logits, prob, disp, dl)

    def timed(fn):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(a.iters):
            fn()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) / a.iters

    plr = ops.warp_softmax(logits[:B], dl[:B], +1.0)
    o = ops.warp_sum(plr, dl[B:], -1.0)
    rows = [("warp_softmax +1", lambda: ops.warp_softmax(logits[:B], dl[:B], +1.0)),
            ("warp_softmax -1 flip", lambda: ops.warp_softmax(logits[B:], dl[B:], -1.0, flip_src=True)),
            ("warp_sum -1", lambda: ops.warp_sum(plr, dl[B:], -1.0)),
            ("warp_sum +1", lambda: ops.warp_sum(plr, dl[:B], +1.0)),
            ("pp_combine", lambda: ops.pp_combine(disp, o, o)),
            ("post_process_disp", lambda: ops.post_process_disp(logits, prob, disp, dl)),
            ("... stepwise", lambda: ops.post_process_disp_stepwise(logits, prob, disp, dl))]
    hw4 = H * W * 4 * B
    bytes_ = {"warp_softmax +1": 2 * N * hw4, "warp_softmax -1 flip": 2 * N * hw4, "warp_sum -1": (N + 1) * hw4, "warp_sum +1": (N + 1) * hw4,
              "pp_combine": 5 * hw4, "post_process_disp": (7 * N + 3) * hw4, "... stepwise": (7 * N + 3) * hw4}
    print("PD_PP_SEG=%s  %dx%dx%dx%d" % (os.environ.get("PD_PP_SEG", "-"), B, N, H, W))
    for name, fn in rows:
        t = timed(fn)
        print("%-22s %.4f ms  %7.1f GB/s" % (name, t, bytes_[name] / (t * 1e-3) / 1e9))


sys.exit(main())
