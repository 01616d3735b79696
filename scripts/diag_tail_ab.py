"""A/B of library builds on the fused network tails (pd_decoder_tail_* / pd_plade_tail_*: fwd, layers, bwd, infer), all in ONE
process on one box: every library named on the command line (`name=path`; `product` = the product library) is loaded side by
side through ctypes and its entry points are called directly with the same inputs.

    python scripts/diag_tail_ab.py parent=<path to the other libplanedepth_hip.so> product [--check] [--rounds 7] [--iters 20] [--out F]

--check: small shapes that reach every code path (4 and 1 pixels per lane, partial workgroups, N = 1, N = 63; disparities per
plane / rows / dense x mask none / rows / dense x mixture x fp32 / bf16; the backward in three argument sets) and every output
tensor of every call compared with the first library's on the RAW BITS (bf16 viewed as int16, fp32 as int32: a NaN cannot pass as
unequal-but-ignored).  Outputs are pre-filled with one byte pattern, so what a kernel leaves unwritten compares equal.  Exit
status 1 when any element differs.

Without --check: B = 8, 192 x 640, the libraries interleaved round by round; device events around a window of --iters
back-to-back calls of ONE entry point (the window's device time is printed: many launches long), fwd / layers / infer / bwd
separately.  Verdict per arm and entry point: the last library's median over the rounds against the first library's own
min-max spread in this process.
"""
import argparse
import ctypes
import itertools
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from planedepth_amd import _capi as C  # noqa: E402
from planedepth_amd.tails import camera_ray_norm  # noqa: E402

DEV = torch.device("cuda:0")
SHAPES = [(2, 5, 8, 16), (1, 3, 3, 5), (2, 4, 2, 6), (1, 2, 5, 300), (1, 2, 7, 150), (2, 1, 4, 8), (1, 63, 4, 32)]
BWD_SETS = ("all", "g_disp->g_raw_logits", "->g_disp_layered")


def load(path):
    return C.bind(ctypes.CDLL(path))


def bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


class Case:
    """One tail call's inputs (seeded as tests/test_infer_tail.py seeds them: raw sigma on both clamp bounds, mask plane 0 all ones)
    and its entry points on a given library; every call returns {name: output tensor}."""

    def __init__(self, net, shape, disp_form, mask_form, mix, bf16, seed=0):
        B, N, H, W = self.shape = shape
        self.net, self.mix, self.st = net, mix, (torch.bfloat16 if bf16 else torch.float32)
        g = torch.Generator().manual_seed(seed + sum(shape))
        ch = N - 1 if net == "plade" else N
        self.rl = (torch.randn(B, ch, H, W, generator=g) * 2.5).to(DEV).to(self.st)
        rs = (torch.randn(B, N, H, W, generator=g) * 3 - 1).to(DEV)
        rs.view(-1)[0::7] = -12.0    # sigmoid = 6e-6: clamped to 0.01
        rs.view(-1)[2::11] = 30.0    # sigmoid = 1.0 exactly: on the upper bound
        self.rs = rs.to(self.st) if mix else None
        lv = torch.arange(N, dtype=torch.float32)[None, :, None, None] + 0.5 * (torch.rand(B, N, 1, 1, generator=g) - 0.5)
        lv = (300.0 * (W / 640.0) * (2.0 / 300.0) ** (lv / max(N - 1, 1))).to(DEV)
        self.flags = (C.PD_TAIL_MIXTURE if mix else 0) | (C.PD_TAIL_BF16 if bf16 else 0)
        if disp_form == "plane":
            self.dl = lv[:, :, 0, 0].contiguous()
        elif disp_form == "rows":
            self.dl = (lv[..., 0] * (1.0 + 0.2 * torch.rand(B, 1, H, generator=g).to(DEV))).contiguous()
            self.flags |= C.PD_TAIL_DISP_ROWS
        else:
            self.dl = (lv * (1.0 + 0.2 * torch.rand(B, 1, H, W, generator=g).to(DEV))).contiguous()
            self.flags |= C.PD_TAIL_DISP_DENSE
        self.per_plane = disp_form == "plane"
        self.pm = None
        if mask_form is not None:
            self.pm = (torch.rand(*((B, N, H) if mask_form == "rows" else (B, N, H, W)), generator=g) > 0.4).float().to(DEV)
            self.pm[:, 0] = 1.0
            self.flags |= C.PD_TAIL_MASK_ROWS if mask_form == "rows" else 0
        self.ray = camera_ray_norm(H, W, DEV) if net == "plade" else None
        up = lambda *s, dtype=torch.float32: torch.randn(*s, generator=g).to(DEV).to(dtype)  # noqa: E731
        self.g_logits, self.g_sigma = up(B, N, H, W, dtype=self.st), up(B, N, H, W, dtype=self.st)
        self.g_dists, self.g_disp, self.g_depth = up(B, N - 1, H, W), up(B, 1, H, W), up(B, 1, H, W)
        self.stream, self.prefill = C.stream_handle(DEV), True

    def new(self, *shape, dtype=torch.float32):
        t = torch.empty(shape, dtype=dtype, device=DEV)
        if self.prefill:
            t.view(torch.uint8).fill_(0x7f)
        return t

    def head(self):   # the leading arguments of every entry point of this net
        B, N, H, W = self.shape
        ops = (self.rl, self.rs, self.pm, self.dl) if self.net == "decoder" else (self.rl, self.rs, self.dl, self.ray)
        return (B, N, H, W, self.flags) + tuple(map(C.ptr, ops))

    def call(self, lib, name, *args):
        rc = getattr(lib, "pd_%s_tail_%s" % (self.net, name))(*args, self.stream)
        assert rc == 0, (name, lib.pd_last_error())

    def fwd(self, lib):
        B, N, H, W = self.shape
        o = dict(disp=self.new(B, 1, H, W), depth=self.new(B, 1, H, W), stash=self.new(B, 2 if self.net == "decoder" else 1, H, W))
        if self.mix:
            o["sigma"] = self.new(B, N, H, W, dtype=self.st)
        if self.net == "plade":
            o["logits"], o["dists"] = self.new(B, N, H, W, dtype=self.st), self.new(B, N - 1, H, W)
            outs = ("logits", "dists", "sigma", "disp", "depth", "stash")
        else:
            if self.pm is not None:
                o["logits"] = self.new(B, N, H, W, dtype=self.st)
            outs = ("logits", "sigma", "disp", "depth", "stash")
        self.call(lib, "fwd", *self.head(), *(C.ptr(o.get(k)) for k in outs))
        return o

    def layers(self, lib, f):
        B, N, H, W = self.shape
        o = dict(pi=self.new(B, N, H, W), probability=self.new(B, N, H, W))
        head = self.head()
        self.call(lib, "layers", *(head[:8] if self.net == "decoder" else head), C.ptr(f["stash"]), C.ptr(o["pi"]), C.ptr(o["probability"]))
        return o

    def infer(self, lib):
        B, N, H, W = self.shape
        o = dict(disp=self.new(B, 1, H, W), depth=self.new(B, 1, H, W), confidence=self.new(B, 1, H, W),
                 plane_index=self.new(B, 1, H, W, dtype=torch.int32), disp_best=self.new(B, 1, H, W),
                 stash=self.new(B, 2 if self.net == "decoder" else 1, H, W))
        self.call(lib, "infer", *self.head(), *(C.ptr(o[k]) for k in ("disp", "depth", "confidence", "plane_index", "disp_best", "stash")))
        return o

    def bwd(self, lib, f, which):
        B, N, H, W = self.shape
        every, only_l, only_d = (which == s for s in BWD_SETS)
        up = dict(g_logits=self.g_logits, g_dists=self.g_dists, g_sigma=self.g_sigma if self.mix else None, g_disp=self.g_disp,
                  g_depth=self.g_depth)
        if only_l:
            up = dict(up, g_logits=None, g_dists=None, g_sigma=None, g_depth=None)
        o = {}
        if every or only_l:
            o["g_raw_logits"] = self.new(*self.rl.shape, dtype=self.st)
        if every and self.mix:
            o["g_raw_sigma"] = self.new(B, N, H, W, dtype=self.st)
        ws = None
        if every or only_d:
            o["g_disp_layered"] = self.new(*self.dl.shape)
            if self.per_plane:
                ws = self.new(lib.pd_decoder_tail_bwd_workspace_floats(B, N, H, W))
        ups = ("g_logits", "g_sigma", "g_disp", "g_depth") if self.net == "decoder" else ("g_logits", "g_dists", "g_sigma", "g_disp", "g_depth")
        self.call(lib, "bwd", *self.head(), C.ptr(f["stash"]), C.ptr(f["disp"]), *(C.ptr(up[k]) for k in ups),
                  *(C.ptr(o.get(k)) for k in ("g_raw_logits", "g_raw_sigma", "g_disp_layered")), C.ptr(ws))
        return o


def check_cases():
    for shape, disp_form, mask_form, mix, bf16 in itertools.product(SHAPES, ("plane", "rows", "dense"), (None, "rows", "dense"),
                                                                    (True, False), (False, True)):
        yield "decoder", shape, disp_form, mask_form, mix, bf16
    for shape, disp_form, mix, bf16 in itertools.product([s for s in SHAPES if s[1] >= 2], ("plane", "dense"), (True, False),
                                                         (False, True)):
        yield "plade", shape, disp_form, None, mix, bf16


def run_all(case, lib):
    f = case.fwd(lib)
    out = {"fwd." + k: v for k, v in f.items()}
    out.update(("layers." + k, v) for k, v in case.layers(lib, f).items())
    out.update(("infer." + k, v) for k, v in case.infer(lib).items())
    for which in BWD_SETS:
        out.update(("bwd[%s].%s" % (which, k), v) for k, v in case.bwd(lib, f, which).items())
    return out


def check(libs, out_path):
    cases = tensors = differing = 0
    bad = []
    for spec in check_cases():
        case = Case(*spec)
        ref = None
        for name, lib in libs:
            got = run_all(case, lib)
            torch.cuda.synchronize()
            if ref is None:
                ref = got
                continue
            assert got.keys() == ref.keys()
            for k in got:
                tensors += 1
                n = int((bits(got[k]) != bits(ref[k])).sum())
                if n:
                    differing += n
                    bad.append(dict(case=repr(spec), library=name, tensor=k, differing=n, of=got[k].numel()))
        cases += 1
    res = dict(mode="check", libraries=[n for n, _ in libs], cases=cases, tensors_compared=tensors, differing_elements=differing,
               differing_tensors=bad)
    print("check: %d cases, %d tensors compared on the raw bits against %s, %d differing elements"
          % (cases, tensors, libs[0][0], differing))
    for b in bad[:40]:
        print("  DIFFERS", b)
    if out_path:
        with open(out_path, "w") as fh:
            json.dump(res, fh, indent=1)
    return 1 if differing else 0


ARMS = [("decoder N=49 per plane, no mask, fp32", ("decoder", (8, 49, 192, 640), "plane", None, True, False)),
        ("decoder N=49 per plane, no mask, bf16", ("decoder", (8, 49, 192, 640), "plane", None, True, True)),
        ("decoder N=63 rows, row mask, fp32", ("decoder", (8, 63, 192, 640), "rows", "rows", True, False)),
        ("plade N=49 per plane, fp32", ("plade", (8, 49, 192, 640), "plane", None, True, False))]


def speed(libs, rounds, iters, out_path):
    results, ok = {}, True
    first, last = libs[0][0], libs[-1][0]
    for arm, spec in ARMS:
        case = Case(*spec)
        f = case.fwd(libs[0][1])
        case.prefill = False   # (a window holds launches of the entry point only; its outputs come from the caching allocator)
        ops = dict(fwd=case.fwd, layers=lambda lib: case.layers(lib, f), infer=case.infer, bwd=lambda lib: case.bwd(lib, f, "all"))
        results[arm] = {}
        for op, run in ops.items():
            ms = {name: [] for name, _ in libs}
            for _, lib in libs:   # warm up (code objects, allocator, power state)
                for _ in range(10):
                    run(lib)
            torch.cuda.synchronize()
            for _ in range(rounds):
                for name, lib in libs:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(iters):
                        run(lib)
                    e1.record()
                    torch.cuda.synchronize()
                    ms[name].append(e0.elapsed_time(e1) / iters)
            a, b = ms[first], ms[last]
            med = statistics.median(b)
            verdict = "below" if med < min(a) else "within" if med <= max(a) else "ABOVE"
            ok &= verdict != "ABOVE"
            results[arm][op] = dict(ms, window_ms=statistics.median(a) * iters, verdict=verdict,
                                    **{first + "_min": min(a), first + "_median": statistics.median(a), first + "_max": max(a),
                                       last + "_median": med})
            print("%-40s %-6s %s %.4f [%.4f .. %.4f]  %s median %.4f ms: %s  (window %.1f ms of device time)"
                  % (arm, op, first, statistics.median(a), min(a), max(a), last, med, verdict, statistics.median(a) * iters))
        del case, f, ops
        torch.cuda.empty_cache()
    if out_path:
        with open(out_path, "w") as fh:
            json.dump(dict(mode="speed", rounds=rounds, iters=iters, libraries=[n for n, _ in libs], results=results), fh, indent=1)
    return 0 if ok else 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs="+")
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    libs = []
    for spec in args.libs:
        name, _, path = spec.partition("=")
        libs.append((name, load(path or os.path.join(ROOT, "planedepth_amd", "lib", "libplanedepth_hip.so"))))
    sys.exit(check(libs, args.out) if args.check else speed(libs, args.rounds, args.iters, args.out))


if __name__ == "__main__":
    main()
