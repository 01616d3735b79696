"""A/B of library builds on the headline kernels, all in ONE process on one box: every library named on the command line
(`name=path`, or a bare variant name -> planedepth_amd/lib/libpd_var_<name>.so; `product` = the product library) is loaded
side by side and runs the same forward -> backward sequence (the caches are then in the state the training step leaves
them in), interleaved round by round; HIP events on the launch stream around each C-ABI call.

    python scripts/diag_kernel_ab.py [--impl 0|2] [--rounds 5] [--iters 40] [--batch 8 ...] product occ4 d2 product@4 ...

`name@impl` runs that library under another pd_sweep_impl than --impl (e.g. product@4 = PD_IMPL_ROWS1 next to product);
--check compares every arm's outputs with the first arm's bit for bit (max |difference| per tensor).  The table gives mean,
median and spread (min .. max over the rounds) per arm, and says for every other arm whether its median lies inside the spread
of the arm named `parent` (of the first arm where none is).

    python scripts/diag_kernel_ab.py --cases small parent=<path> product

--cases small: no timing.  Every C entry point of the row kernels (the sweep's forward and backward in all their forms, the two
fused-tail backwards, pd_warp_softmax / pd_warp_sum, pd_post_process) runs in both libraries on the same inputs at B = 2, H = 14
(rows 1-3 lean on the row above, row 7 on the row below: both two-row bodies, both pair roles), W = 64 / 130 / 258 / 65, sign
+-1, with N = 7 disparities that hold a fractional, an integer (irregular path), a (128, 256), a clamped and a NaN shift, and
every output tensor is compared on the raw bits.  Two allowances, both reported as "noisy"; exit status 1 on any other differing bit:
  * the integer-shift plane's rows of g_logits, g_sigma and g_plane (float atomics, sums that meet in LDS in arrival order): an
    entry may differ where the first library differs from ITSELF at that entry between runs on the same input (it runs every case
    eight times), and by no more than it does there;
  * g_plane of the cases the row-shift backward serves (render, per-pixel mask, PD_IMPL_ROWS1, odd W): that kernel's assembly is
    byte-identical in both trees and its waves add a row's sums in arrival order, so the tensor is exempt where the first library
    differs from itself in it.

    python scripts/diag_kernel_ab.py --cases homography parent=<path> product

--cases homography: the same comparison for the kernels behind homography_warp and the general path (pd_plane_sweep.hip,
pd_plane_sweep_uniform.hip, pd_plane_sweep_gather.hip), through pd_plane_sweep_fwd / _bwd, pd_uniform_fwd_pair / pd_uniform_bwd_pair /
pd_uniform_gather_pair and pd_plane_sweep_layers:
  * plane-uniform at (B, N, H, W) = (2, 7, 18, 80) — a partial last 256-thread block, partial 32 x 16 tiles on both axes, an odd N for the
    two-plane staging group — and (1, 5, 6, 96), with the pose draws of tests/test_gpu_parity.py (_f8_pose: ~1 degree, the staged pass 2)
    and the 3x3 block scaled by 1, 2, 4, 2.6 and 0.45 (lists beyond the 12 / 10 register slots: the follow-up kernel; boxes beyond 1024
    elements: the workgroup's direct branch); mixture and L1, softmax and render, automask, g_plane with and without translation weights,
    PD_BWD_ACCUMULATE on and off, PD_IMPL_UNIFORM_DIRECT, the pair entry points and the deferred gather;
  * one matrix per plane at (2, 7, 8, 80) and (1, 5, 6, 96) (tests/test_gpu_parity.py: _gather_case): the gather backward (PD_IMPL_AUTO, and
    its direct pass 2) and the scatter backward (PD_IMPL_GENERAL), one plane made irregular (the fix-up kernel), render and accumulate on
    and off;
  * disp mode on the general kernels (PD_IMPL_GENERAL): a dense map, a per-pixel mask, N = 33 (a second mask word in the stash);
  * pd_plane_sweep_layers in its four instantiations.
Deterministic tensors (rgb_rec, ph_map, the stash, g_dists, g_logits / g_sigma of the plane-uniform and gather backwards, the layer
tensors) must agree bit for bit.  The order-dependent sums — the scatter backward's g_logits / g_sigma and the fix-up's plane (float
atomics), g_plane (waves meet in LDS in arrival order), ph_mean (one atomic per workgroup) — get the per-entry allowance above: an entry
may differ where the first library differs from itself at that entry over its eight runs, and by no more than it does there.
"""
import argparse
import ctypes
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from planedepth_amd import _capi as C  # noqa: E402
from planedepth_amd.synthetic import survey_fullsize_case  # noqa: E402


def load(path):
    return C.bind(ctypes.CDLL(path))


IRR = 1                                          # small cases: index of the integer-shift plane
kRefRuns = 8                                     # the first library runs every case this often: its own run-to-run difference
                                                 # (a fixed count: a comparison outside the allowance fails, it is not re-sampled)
bits = lambda t: t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


class Compare:
    """Raw-bit comparison of libs[1:] against libs[0], case by case; the report and the counts."""

    def __init__(self, libs):
        self.libs, self.report, self.bad, self.noisy = libs, [], 0, 0

    def __call__(self, case, runs, rowshift_bwd=False, order_dependent=None):
        """runs: {lib name: [outputs of run 1, run 2, ...]} (dict name -> tensor, or 'rc').  rowshift_bwd: the case's backward is
        the row-shift backward (pd_plane_sweep_rowshift.hip), not the row-stream one.  order_dependent (the homography cases):
        {tensor name: True, or a bool mask} — where the per-entry allowance applies instead of the small cases' irregular-plane rows."""
        libs = self.libs
        ref_name = libs[0][0]
        ref, again = runs[ref_name][0], runs[ref_name][1:]
        for name, _ in libs[1:]:
            got = runs[name][0]
            row = {"case": case, "lib": name, "rc": got["rc"], "rc_ref": ref["rc"], "tensors": {}}
            ok = got["rc"] == ref["rc"]
            for k, t in ref.items():
                if k == "rc" or t is None:
                    continue
                ne = bits(t) != bits(got[k])
                n_ne = int(ne.sum())
                ent = {"differing": n_ne, "of": t.numel()}
                if n_ne:
                    # Per ENTRY: what the first library's other runs differ from its first run by, on the same input.
                    absd = lambda x: (x.float() - t.float()).abs()
                    own = torch.stack([absd(r2[k]) for r2 in again]).amax(0)
                    own_ne = torch.stack([bits(r2[k]) != bits(t) for r2 in again]).any(0)
                    ent.update(max_abs=float(absd(got[k]).nan_to_num(0).max()), reference_run_to_run_differing=int(own_ne.sum()),
                               reference_run_to_run_max_abs=float(own.nan_to_num(0).max()))
                    if order_dependent is not None:
                        # ORDER-DEPENDENT SUMS of the homography cases: only the tensors (or the part of one) the case names, and there
                        # only entries at which the first library differs from itself, by no more than it does at that entry.
                        ent["allowance"] = "order-dependent sum, per entry" if k in order_dependent else "none"
                        region = torch.zeros_like(ne)
                        if k in order_dependent:
                            region |= order_dependent[k] if torch.is_tensor(order_dependent[k]) else torch.ones_like(ne)
                        allowed = region & own_ne & (absd(got[k]) <= own)      # (a NaN difference compares False)
                    elif k == "g_plane" and rowshift_bwd:
                        # ROW-SHIFT G_PLANE EXCEPTION.  The row-shift backward's waves add their disparity-gradient sums of a row
                        # in LDS in the order they arrive, so entries of every plane in view differ between two runs of ONE library;
                        # its assembly is byte-identical in both trees (profiles/row_layer_refactor_ab.md §1.1), so the new
                        # library's draw of that order is as good as another run of the first.  Exempt where the first library does
                        # differ from itself in this tensor; the entries beyond its own sampled difference are counted, not judged.
                        ent["allowance"] = "row-shift backward's g_plane: identical assembly, the first library differs from itself"
                        ent["beyond_reference_run_to_run"] = int((ne & ~(own_ne & (absd(got[k]) <= own))).sum())
                        allowed = ne if bool(own_ne.any()) else torch.zeros_like(ne)
                    else:
                        # IRREGULAR-PLANE ALLOWANCE.  Only the integer-shift plane's rows of g_logits, g_sigma and g_plane (float
                        # atomics into zero-filled rows; the row's sums meet in LDS in arrival order), and there only entries at
                        # which the first library differs from itself, by no more than it does at that entry.
                        ent["allowance"] = "irregular plane's rows, per entry"
                        region = torch.zeros_like(ne)
                        if k in ("g_logits", "g_sigma", "g_plane"):
                            region[:, IRR] = True
                        allowed = region & own_ne & (absd(got[k]) <= own)      # (a NaN difference compares False)
                    outside = ne & ~allowed
                    ent["outside_allowance"] = int(outside.sum())
                    if t.numel() <= 64:
                        ent["at"] = [list(map(int, i)) for i in ne.nonzero()[:8]]
                    if ent["outside_allowance"]:   # where, what the first library's first run holds, and both differences from it
                        ent["outside_at"] = [{"index": list(map(int, i)), "reference": float(t[tuple(i)]), "abs": float(absd(got[k])[tuple(i)]),
                                              "reference_run_to_run_abs": float(own[tuple(i)])} for i in outside.nonzero()[:8]]
                    if ent["outside_allowance"]:
                        ok = False
                    else:
                        row["noisy"] = True
                row["tensors"][k] = ent
            row["ok"] = ok
            self.bad += 0 if ok else 1
            self.report.append(row)
            diff = {k: v for k, v in row["tensors"].items() if v["differing"]}
            self.noisy += 1 if (ok and row.get("noisy")) else 0
            print("%-4s %-58s %-10s rc %d/%d  %s" % (("noisy" if row.get("noisy") else "ok") if ok else "FAIL", case, name, got["rc"], ref["rc"], diff or "0 differing bits in %d tensors" % len(row["tensors"])),
                  flush=True)

    def finish(self, mode, out_path):
        print("%d comparisons, %d failed, %d differing inside an allowance only (noisy)" % (len(self.report), self.bad, self.noisy))
        if out_path:
            with open(out_path, "w") as fh:
                json.dump({"mode": mode, "libs": [n for n, _ in self.libs], "failed": self.bad, "noisy": self.noisy, "reference_runs": kRefRuns,
                           "comparisons": self.report}, fh, indent=1)
        return 1 if self.bad else 0


def small_cases(libs, out_path):
    """Raw-bit comparison of libs[1:] against libs[0] over small shapes that reach every path of the row kernels."""
    dev = torch.device("cuda:0")
    st = C.stream_handle(dev)
    B, H, N = 2, 14, 7
    g = torch.Generator().manual_seed(20)
    rnd = lambda *sh: torch.randn(*sh, generator=g).to(dev)
    uni = lambda *sh: torch.rand(*sh, generator=g).to(dev)
    base = torch.tensor([0.37, 3.0, 200.5, 5000.0, float("nan"), 1.75, 17.25])
    compare = Compare(libs)

    def fresh(*sh, dtype=torch.float32):   # outputs start from the same pattern in every run: an unwritten element compares equal
        return torch.full(sh, -7.0, device=dev, dtype=dtype)

    def sweep_case(W, sign, form):
        mixture = form != "l1" and form != "l1_auto"
        flags = (C.PD_MIXTURE if mixture else 0) | (C.PD_AUTOMASK if form in ("mix_auto", "l1_auto") else 0)
        impl = {"fast_rows": C.PD_IMPL_FAST_ROWS, "rows1": C.PD_IMPL_ROWS1}.get(form, C.PD_IMPL_AUTO)
        rows = form in ("rows_masked", "tail_rows")
        if rows:
            flags |= C.PD_DISP_ROWS | C.PD_MASK_ROWS
        if form == "render":
            flags |= C.PD_RENDER_PROB
        bf16 = form == "bf16"
        if bf16:
            flags |= C.PD_LOGITS_BF16
        dt = torch.bfloat16 if bf16 else torch.float32
        src, tgt = uni(B, 3, H, W), uni(B, 3, H, W)
        logits = rnd(B, N, H, W).to(dt)
        sigma = (0.01 + 0.99 * uni(B, N, H, W))
        sigma[:, :, :, ::9] = 0.01                                    # the clamp's lower bound (the tail's gate reads raw_sigma there)
        sigma = sigma.to(dt)
        plane = base.to(dev)[None, :].repeat(B, 1)
        plane[1, 0] = 0.81
        mask = None
        if rows:
            plane = plane[:, :, None].repeat(1, 1, H) * torch.linspace(1.0, 1.5, H, device=dev)[None, None, :]
            plane[:, IRR] = 3.0                                       # stays an integer on every row
            mask = torch.ones(B, N, H, device=dev)
            mask[1, 5, 3] = 0.0                                       # one masked (plane, row)
        if form == "pixel_mask":
            mask = (uni(B, N, H, W) > 0.2).float()
        dists = (0.05 + uni(B, N - 1, H, W)) if form == "render" else None
        g_rgb, gphm = rnd(B, 3, H, W), torch.ones(1, device=dev)
        raw_sigma, tstash, tdisp = rnd(B, N, H, W), torch.cat([rnd(B, 1, H, W), 0.5 + uni(B, 1, H, W)], 1), 0.5 + uni(B, 1, H, W)
        g_disp, g_depth = rnd(B, 1, H, W), rnd(B, 1, H, W)
        d = C.SweepDesc(B, N, H, W, C.PD_WARP_DISP, flags, sign, impl)
        P = lambda t: None if t is None else C.ptr(t)
        runs = {}
        for name, lib in libs:
            runs[name] = []
            for _ in range(kRefRuns if name == libs[0][0] else 1):
                k = lib.pd_sweep_stash_floats(ctypes.byref(d)) // (H * W)
                rgb, ph, stash = fresh(B, 3, H, W), fresh(B, 1, H, W), fresh(B, max(k, 1), H, W)
                gl, gs, gp = fresh(B, N, H, W, dtype=dt), fresh(B, N, H, W, dtype=dt), fresh(*plane.shape)
                gd = fresh(B, N - 1, H, W) if dists is not None else None
                ws = fresh(max(int(lib.pd_sweep_bwd_workspace_floats(ctypes.byref(d))), 1))
                rc = lib.pd_plane_sweep_fwd(ctypes.byref(d), P(src), P(tgt), P(logits), P(sigma) if mixture else None, P(plane), None, None,
                                            P(mask), P(dists), P(rgb), P(ph), None, P(stash), st)
                if rc == 0 and form == "tail":
                    rc = lib.pd_plane_sweep_bwd_tail(ctypes.byref(d), P(src), P(tgt), P(logits), P(sigma), P(plane), P(rgb), P(stash), P(g_rgb), None,
                                                     P(gphm), P(raw_sigma), P(tstash), P(tdisp), P(g_disp), P(g_depth), P(gl), P(gs), P(gp), P(ws), st)
                elif rc == 0 and form == "tail_rows":
                    rc = lib.pd_plane_sweep_bwd_tail_rows(ctypes.byref(d), P(src), P(tgt), P(logits), P(sigma), P(plane), P(mask), P(rgb), P(stash),
                                                          P(g_rgb), None, P(gphm), P(raw_sigma), P(tstash), P(tdisp), P(g_disp), P(g_depth), P(gl),
                                                          P(gs), P(gp), P(ws), st)
                elif rc == 0:
                    rc = lib.pd_plane_sweep_bwd(ctypes.byref(d), P(src), P(tgt), P(logits), P(sigma) if mixture else None, P(plane), None, None, P(mask),
                                                P(dists), P(rgb), P(stash), P(g_rgb), None, P(gphm), P(gl), P(gs) if mixture else None, P(gp), P(gd),
                                                P(ws), st)
                torch.cuda.synchronize()
                runs[name].append({"rc": rc, "rgb_rec": rgb, "ph_map": ph, "stash": stash, "g_logits": gl, "g_sigma": gs, "g_plane": gp, "g_dists": gd})
        # rowstream_bwd_applicable()'s conditions at these shapes (the row's LDS always fits): anything else is the row-shift backward
        rowshift_bwd = form in ("render", "pixel_mask", "rows1") or W % 2 == 1
        compare("sweep %-11s W=%-3d sign=%+d" % (form, W, int(sign)), runs, rowshift_bwd)

    def warp_case(W, sign, n, flip, rows):
        flags = (C.PD_PP_FLIP_SRC if flip else 0) | (C.PD_PP_DISP_ROWS if rows else 0)
        planes = rnd(B, n, H, W)
        disp = base.to(dev)[None, :n].repeat(B, 1)
        if rows:
            disp = disp[:, :, None].repeat(1, 1, H) * torch.linspace(1.0, 1.5, H, device=dev)[None, None, :]
            disp[:, IRR] = 3.0
        runs = {}
        for name, lib in libs:
            runs[name] = []
            for _ in range(kRefRuns if name == libs[0][0] else 1):
                sm, su = fresh(B, n, H, W), fresh(B, 1, H, W)
                rc = lib.pd_warp_softmax(B, n, H, W, sign, flags, C.ptr(planes), C.ptr(disp), C.ptr(sm), st)
                rc = rc or lib.pd_warp_sum(B, n, H, W, sign, flags, C.ptr(planes), C.ptr(disp), 1.0, C.ptr(su), st)
                torch.cuda.synchronize()
                runs[name].append({"rc": rc, "warp_softmax": sm, "warp_sum": su})
        compare("warp flip=%d rows=%d W=%-3d sign=%+d" % (flip, rows, W, int(sign)), runs)

    def pp_case(W, n):
        logits, prob, disp = rnd(2 * B, n, H, W), torch.softmax(rnd(2 * B, n, H, W), 1), 0.5 + uni(2 * B, 1, H, W)
        lv = torch.cat([base[:min(n, N)], 0.31 + 2.71 * torch.arange(max(n - N, 0), dtype=torch.float32)]).to(dev)
        dl = lv[None, :].repeat(2 * B, 1).contiguous()
        runs = {}
        for name, lib in libs:
            runs[name] = []
            for _ in range(kRefRuns if name == libs[0][0] else 1):
                ws = fresh(max(int(lib.pd_post_process_workspace_floats(B, n, H, W)), 1))
                dpp, mn = fresh(B, 1, H, W), fresh(B, 1, H, W)
                rc = lib.pd_post_process(B, n, H, W, 0, C.ptr(logits), C.ptr(prob), C.ptr(disp), C.ptr(dl), C.ptr(ws), C.ptr(dpp), C.ptr(mn), st)
                torch.cuda.synchronize()
                runs[name].append({"rc": rc, "disp_pp": dpp, "mask_novel": mn})
        compare("post_process N=%-2d W=%-3d" % (n, W), runs)

    forms = ["mix", "mix_auto", "l1", "l1_auto", "rows_masked", "render", "bf16", "pixel_mask", "fast_rows", "rows1", "tail", "tail_rows"]
    for W in (64, 130, 258, 65):
        for sign in (1.0, -1.0):
            for form in forms:
                if form == "bf16" and W % 2:
                    continue                                          # PD_LOGITS_BF16 is only served at even W
                sweep_case(W, sign, form)
            for flip in (0, 1):
                for rows in (0, 1):
                    warp_case(W, sign, N, flip, rows)
        pp_case(W, N)
        pp_case(W, 63)
    return compare.finish("cases small", out_path)


def homography_cases(libs, out_path):
    """Raw-bit comparison of libs[1:] against libs[0] over small shapes that reach every branch of the homography-mode and general
    kernels (the module docstring lists them)."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_gpu_parity import _f8_pose, _gather_case   # the suite's pose and per-plane-matrix draws
    from planedepth_amd import ops
    from planedepth_amd.synthetic import intrinsics
    dev = torch.device("cuda:0")
    st = C.stream_handle(dev)
    compare = Compare(libs)
    P = lambda t: None if t is None else C.ptr(t)
    fresh = lambda *sh: torch.full(sh, -7.0, device=dev)   # outputs start from the same pattern in every run
    ALL = True

    def each_run(fn):
        """fn(lib) -> outputs; the first library kRefRuns times."""
        runs = {}
        for name, lib in libs:
            runs[name] = []
            for _ in range(kRefRuns if name == libs[0][0] else 1):
                out = fn(lib)
                torch.cuda.synchronize()
                runs[name].append(out)
        return runs

    def inputs(B, N, H, W, seed):
        g = torch.Generator().manual_seed(seed)
        z = dict(src=torch.rand(B, 3, H, W, generator=g), tgt=torch.rand(B, 3, H, W, generator=g), tgt2=torch.rand(B, 3, H, W, generator=g),
                 logits=torch.randn(B, N, H, W, generator=g), sigma=0.011 + 0.978 * torch.rand(B, N, H, W, generator=g),
                 g_rgb=torch.randn(B, 3, H, W, generator=g) * 0.1, g_ph=torch.randn(B, 1, H, W, generator=g) * 0.1,
                 dists=torch.rand(B, N - 1, H, W, generator=g) * 2.0, distance=0.5 + 5 * torch.rand(B, N, generator=g))
        z["sigma"][:, :, :, ::9] = 0.005                                  # below the clamp: the gate closes
        return {k: v.to(dev).contiguous() for k, v in z.items()}

    def sweep(lib, d, z, plane, aux, iK, mask, mix, render, tgt="tgt", ph_mean=True, want_plane=True):
        """One forward + backward through pd_plane_sweep_fwd / _bwd; every output tensor."""
        B, N, H, W = d.B, d.N, d.H, d.W
        k = lib.pd_sweep_stash_floats(ctypes.byref(d)) // (H * W)
        o = dict(rgb_rec=fresh(B, 3, H, W), ph_map=fresh(B, 1, H, W), ph_mean=fresh(1) if ph_mean else None, stash=fresh(B, max(k, 1), H, W),
                 g_logits=fresh(B, N, H, W), g_sigma=fresh(B, N, H, W) if mix else None,
                 g_plane=fresh(*plane.shape) if want_plane else None, g_dists=fresh(B, N - 1, H, W) if render else None)
        ws = fresh(max(int(lib.pd_sweep_bwd_workspace_floats(ctypes.byref(d))), 1))
        sg, dd = (P(z["sigma"]) if mix else None), (P(z["dists"]) if render else None)
        rc = lib.pd_plane_sweep_fwd(ctypes.byref(d), P(z["src"]), P(z[tgt]), P(z["logits"]), sg, P(plane), P(aux), P(iK), P(mask), dd,
                                    P(o["rgb_rec"]), P(o["ph_map"]), P(o["ph_mean"]), P(o["stash"]), st)
        if rc == 0:
            rc = lib.pd_plane_sweep_bwd(ctypes.byref(d), P(z["src"]), P(z[tgt]), P(z["logits"]), sg, P(plane), P(aux), P(iK), P(mask), dd,
                                        P(o["rgb_rec"]), P(o["stash"]), P(z["g_rgb"]), P(z["g_ph"]), P(z["g_phm"]), P(o["g_logits"]),
                                        P(o["g_sigma"]), P(o["g_plane"]), P(o["g_dists"]), P(ws), st)
        o["rc"] = rc
        o["workspace"] = ws   # (kept alive; the deferred gather reads it)
        return o

    def drop_ws(runs):
        for rr in runs.values():
            for r in rr:
                r.pop("workspace", None)
        return runs

    FORMS = [("mix", True, False, False), ("mix_auto", True, True, False), ("l1", False, False, False), ("l1_auto", False, True, False),
             ("mix_render", True, False, True), ("l1_render_auto", False, True, True)]

    # ---- plane-uniform -------------------------------------------------------------------------------------------------------
    def uniform_matrices(z, B, N, H, W, rot, zoom, seed):
        K, inv_K = (t.to(dev) for t in intrinsics(B, H, W))
        norm = torch.tensor([0.0, 0.0, 1.0])[None, None].repeat(B, N, 1)
        norm[:, N // 2:] = torch.nn.functional.normalize(torch.tensor([0.0, 1.0, 0.07]), dim=0)   # "xz planes": the facing test differs per plane
        norm = norm.to(dev)
        Rt = _f8_pose(B, seed, rot, dev)
        Rt[:, :2, :3] *= zoom
        with torch.no_grad():
            Hm, Rn = ops.homography_matrices_fused(z["distance"], norm, Rt, K, inv_K, C.PD_HMAT_UNIFORM)
            tw = (norm / z["distance"][..., None]).contiguous()
        return Hm.contiguous(), Rn.reshape(B * N, 3).contiguous(), inv_K[:, :3, :3].contiguous(), tw

    for (B, N, H, W) in ((2, 7, 18, 80), (1, 5, 6, 96)):
        z = inputs(B, N, H, W, 900 + W + N)
        z["g_phm"] = torch.full((1,), 2.0, device=dev)
        for rot, zoom in ((0.02, 1.0), (0.02, 2.0), (0.02, 4.0), (0.05, 2.6), (0.05, 0.45)):
            Hm, Rn, iK, tw = uniform_matrices(z, B, N, H, W, rot, zoom, 31 + H)
            Hm2, Rn2, iK2, tw2 = uniform_matrices(z, B, N, H, W, 0.03 if zoom == 1.0 else 0.02, 1.55 if zoom == 2.6 else 1.0, 32 + H)   # view B
            for form, mix, automask, render in FORMS:
                fl = C.PD_HOMO_UNIFORM | (C.PD_MIXTURE if mix else 0) | (C.PD_AUTOMASK if automask else 0) | (C.PD_RENDER_PROB if render else 0)
                for impl in (C.PD_IMPL_AUTO, C.PD_IMPL_UNIFORM_DIRECT):
                    for acc in (0, C.PD_BWD_ACCUMULATE):
                        for weights in (True, False):
                            d = C.SweepDesc(B, N, H, W, C.PD_WARP_HOMOGRAPHY, fl | acc, 0.0, impl)
                            runs = each_run(lambda lib: sweep(lib, d, z, Hm, Rn, iK, tw if weights else None, mix, render))
                            compare("uniform %dx%dx%dx%d rot %.2f zoom %.2f %-14s impl %d acc %d tw %d" % (B, N, H, W, rot, zoom, form, impl, bool(acc), weights),
                                    drop_ws(runs), order_dependent={"g_plane": ALL, "ph_mean": ALL})
                # the two views of a step: pd_uniform_fwd_pair + pd_uniform_bwd_pair, and the deferred form (two first passes + pd_uniform_gather_pair)
                for acc in (0, C.PD_BWD_ACCUMULATE):
                    d = C.SweepDesc(B, N, H, W, C.PD_WARP_HOMOGRAPHY, fl | acc, 0.0, C.PD_IMPL_AUTO)

                    def pair(lib):
                        k = lib.pd_sweep_stash_floats(ctypes.byref(d)) // (H * W)
                        nws = max(int(lib.pd_sweep_bwd_workspace_floats(ctypes.byref(d))), 1)
                        o, views, keep = {}, [], []
                        for v, (tgt, hm, rn, ik, w) in enumerate((("tgt", Hm, Rn, iK, tw), ("tgt2", Hm2, Rn2, iK2, tw2))):
                            t = dict(rgb_rec=fresh(B, 3, H, W), ph_map=fresh(B, 1, H, W), ph_mean=fresh(1), stash=fresh(B, k, H, W),
                                     g_plane=fresh(B, 4, 3, 3), g_dists=fresh(B, N - 1, H, W) if render else None)
                            ws = fresh(nws)
                            keep.append(ws)
                            views.append(C.sweep_view(tgt=z[tgt], plane=hm, plane_aux=rn, inv_K3=ik, padding_mask=w, dists=z["dists"] if render else None,
                                                      g_rgb_rec=z["g_rgb"], g_ph_map=z["g_ph"], g_ph_mean=z["g_phm"], workspace=ws, **t))
                            o.update({"%s%d" % (kk, v): vv for kk, vv in t.items()})
                        o["g_logits"], o["g_sigma"] = fresh(B, N, H, W), (fresh(B, N, H, W) if mix else None)
                        sg = P(z["sigma"]) if mix else None
                        rc = lib.pd_uniform_fwd_pair(ctypes.byref(d), P(z["src"]), P(z["logits"]), sg, ctypes.byref(views[0]), ctypes.byref(views[1]), st)
                        if rc == 0:
                            rc = lib.pd_uniform_bwd_pair(ctypes.byref(d), P(z["src"]), P(z["logits"]), sg, ctypes.byref(views[0]), ctypes.byref(views[1]),
                                                         P(o["g_logits"]), P(o["g_sigma"]), st)
                        torch.cuda.synchronize()
                        o["rc"] = rc
                        return o
                    compare("uniform pair %dx%dx%dx%d rot %.2f zoom %.2f %-14s acc %d" % (B, N, H, W, rot, zoom, form, bool(acc)), each_run(pair),
                            order_dependent={"g_plane0": ALL, "g_plane1": ALL, "ph_mean0": ALL, "ph_mean1": ALL})

                    dd = C.SweepDesc(B, N, H, W, C.PD_WARP_HOMOGRAPHY, fl | acc | C.PD_BWD_DEFER_GATHER, 0.0, C.PD_IMPL_AUTO)

                    def deferred(lib):
                        a = sweep(lib, dd, z, Hm, Rn, iK, tw, mix, render, want_plane=False)
                        b = sweep(lib, dd, z, Hm2, Rn2, iK2, tw2, mix, render, tgt="tgt2", want_plane=False)
                        o = {"g_logits": fresh(B, N, H, W), "g_sigma": fresh(B, N, H, W) if mix else None, "g_dists0": a["g_dists"], "g_dists1": b["g_dists"]}
                        rc = a["rc"] or b["rc"] or lib.pd_uniform_gather_pair(ctypes.byref(dd), P(Hm), P(iK), P(a["workspace"]), P(Hm2), P(iK2), P(b["workspace"]),
                                                                              P(o["g_logits"]), P(o["g_sigma"]), st)
                        torch.cuda.synchronize()
                        o["rc"] = rc
                        return o
                    compare("uniform deferred gather %dx%dx%dx%d rot %.2f zoom %.2f %-14s acc %d" % (B, N, H, W, rot, zoom, form, bool(acc)), each_run(deferred),
                            order_dependent={})

    # ---- one matrix per plane: the gather backward (and its direct pass 2) and the scatter backward -----------------------------------
    for (B, N, H, W) in ((2, 7, 8, 80), (1, 5, 6, 96)):
        z = inputs(B, N, H, W, 300 + W + N)
        z["g_phm"] = torch.full((1,), 3.0, device=dev)
        _, _, _, _, _, Hm0, Rn0, iK = [t.to(dev).contiguous() for t in _gather_case(B, N, H, W, 300 + W + N)]
        for irregular in (False, True):
            Hm, Rn = Hm0.clone(), Rn0.clone()
            irr = torch.zeros(B, N, H, W, dtype=torch.bool, device=dev)
            if irregular:   # one plane the gather hands to its atomic fix-up: 16 target pixels per source pixel (_gather_case's first)
                Hm[0] = torch.tensor([[0.25, 0.0, 0.3 * W], [0.0, 0.25, 0.3 * H], [0.0, 0.0, 1.0]], device=dev)
                Rn[0] = torch.tensor([0.0, 0.0, 1.0], device=dev)
                irr[0, 0] = True
            for form, mix, automask, render in FORMS:
                fl = (C.PD_MIXTURE if mix else 0) | (C.PD_AUTOMASK if automask else 0) | (C.PD_RENDER_PROB if render else 0)
                for impl in (C.PD_IMPL_AUTO, C.PD_IMPL_UNIFORM_DIRECT, C.PD_IMPL_GENERAL):
                    for acc in (0, C.PD_BWD_ACCUMULATE):
                        d = C.SweepDesc(B, N, H, W, C.PD_WARP_HOMOGRAPHY, fl | acc, 0.0, impl)
                        runs = each_run(lambda lib: sweep(lib, d, z, Hm, Rn, iK, None, mix, render))
                        scatter = impl == C.PD_IMPL_GENERAL
                        od = {"g_plane": ALL, "ph_mean": ALL, "g_logits": ALL if scatter else irr, "g_sigma": ALL if scatter else irr}
                        compare("planes %dx%dx%dx%d %-14s impl %d acc %d irregular %d" % (B, N, H, W, form, impl, bool(acc), irregular), drop_ws(runs),
                                order_dependent=od)

    # ---- disp mode on the general kernels: dense map, per-pixel mask, a second mask word ------------------------------------------------
    B, N, H, W = 2, 33, 8, 80
    z = inputs(B, N, H, W, 77)
    z["g_phm"] = torch.full((1,), 1.0, device=dev)
    g = torch.Generator().manual_seed(78)
    dense = (torch.rand(B, N, H, W, generator=g) * 30.0 - 4.0).to(dev)
    mask = (torch.rand(B, N, H, W, generator=g) > 0.2).float().to(dev)
    planes = (torch.rand(B, N, generator=g) * 30.0).to(dev)
    for form, mix, automask, render in FORMS:
        for name, plane, dflag, mk in (("dense+mask", dense, C.PD_DISP_DENSE, mask), ("dense", dense, C.PD_DISP_DENSE, None), ("scalar+mask", planes, 0, mask)):
            for sign in (1.0, -1.0):
                fl = dflag | (C.PD_MIXTURE if mix else 0) | (C.PD_AUTOMASK if automask else 0) | (C.PD_RENDER_PROB if render else 0)
                d = C.SweepDesc(B, N, H, W, C.PD_WARP_DISP, fl, sign, C.PD_IMPL_GENERAL)
                runs = each_run(lambda lib: sweep(lib, d, z, plane, None, None, mk, mix, render))
                # (a dense map's g_plane is a per-pixel store: deterministic)
                od = {"g_logits": ALL, "g_sigma": ALL, "ph_mean": ALL}
                if not dflag:
                    od["g_plane"] = ALL
                compare("disp general %-11s %-14s sign %+d" % (name, form, int(sign)), drop_ws(runs), order_dependent=od)

    # ---- pd_plane_sweep_layers: <disp | homography> x <L1 | mixture>, softmax and render ---------------------------------------------------
    zh = inputs(2, 7, 8, 80, 387)
    _, _, _, _, _, Hm, Rn, iK = [t.to(dev).contiguous() for t in _gather_case(2, 7, 8, 80, 387)]
    for mode, zz, plane, aux, ik, mk, (B, N, H, W) in ((C.PD_WARP_DISP, z, dense, None, None, mask, (2, 33, 8, 80)),
                                                      (C.PD_WARP_HOMOGRAPHY, zh, Hm, Rn, iK, None, (2, 7, 8, 80))):
        for mix in (True, False):
            for render in (False, True):
                fl = (C.PD_DISP_DENSE if mode == C.PD_WARP_DISP else 0) | (C.PD_MIXTURE if mix else 0) | (C.PD_RENDER_PROB if render else 0)
                d = C.SweepDesc(B, N, H, W, mode, fl, 1.0, C.PD_IMPL_AUTO)

                def layers(lib):
                    o = dict(rgb_rec_layered=fresh(B, N, 3, H, W), logit_rec=fresh(B, N, H, W), probability_rec=fresh(B, N, H, W),
                             sigma_rec=fresh(B, N, H, W) if mix else None, pi_rec=fresh(B, N, H, W) if mix else None)
                    o["rc"] = lib.pd_plane_sweep_layers(ctypes.byref(d), P(zz["src"]), P(zz["logits"]), P(zz["sigma"]) if mix else None, P(plane), P(aux), P(ik),
                                                        P(mk), P(zz["dists"]) if render else None, P(o["rgb_rec_layered"]), P(o["logit_rec"]),
                                                        P(o["probability_rec"]), P(o["sigma_rec"]), P(o["pi_rec"]), st)
                    return o
                compare("layers mode %d mix %d render %d" % (mode, mix, render), each_run(layers), order_dependent={})
    return compare.finish("cases homography", out_path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs="+")
    ap.add_argument("--impl", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--planes", type=int, default=49)
    ap.add_argument("--height", type=int, default=192)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--automask", action="store_true")
    ap.add_argument("--fwd_only", action="store_true")
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--out", default="")
    ap.add_argument("--cases", choices=["small", "homography"], default=None, help="raw-bit comparison over small shapes instead of timing")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    if args.cases:
        named, seen = [], {}
        for spec in args.libs:
            name, _, path = spec.partition("=")
            path = path or os.path.join(ROOT, "planedepth_amd", "lib", "libplanedepth_hip.so" if name == "product" else "libpd_var_%s.so" % name)
            seen.setdefault(path, load(path))
            named.append((name, seen[path]))
        sys.exit((small_cases if args.cases == "small" else homography_cases)(named, args.out))
    c = survey_fullsize_case(B=args.batch, N=args.planes, H=args.height, W=args.width, seed=1234)
    c = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in c.items()}
    B, N, H, W = c["logits"].shape
    plane = c["disp_pp"][:, :, 0, 0].contiguous()
    flags = C.PD_MIXTURE | (C.PD_AUTOMASK if args.automask else 0) | C.PD_PH_MEAN_ZEROED   # (no memset launch in front of the forward)
    d = C.SweepDesc(B, N, H, W, C.PD_WARP_DISP, flags, 1.0, args.impl)
    libs, descs, loaded = [], {}, {}
    for spec in args.libs:
        name, _, path = spec.partition("=")
        base, _, impl = name.partition("@")
        if not path:
            path = (os.path.join(ROOT, "planedepth_amd", "lib", "libplanedepth_hip.so") if base == "product"
                    else os.path.join(ROOT, "planedepth_amd", "lib", "libpd_var_%s.so" % base))
        if path not in loaded:
            loaded[path] = load(path)
        libs.append((name, loaded[path]))
        descs[name] = C.SweepDesc(B, N, H, W, C.PD_WARP_DISP, flags, 1.0, int(impl) if impl else args.impl)
    lib0 = libs[0][1]
    k = lib0.pd_sweep_stash_floats(ctypes.byref(d)) // (H * W)
    rgb = torch.empty(B, 3, H, W, device=dev)
    ph = torch.empty(B, 1, H, W, device=dev)
    stash = torch.empty(B, k, H, W, device=dev)
    gl, gs, gp = torch.empty_like(c["logits"]), torch.empty_like(c["sigma"]), torch.empty_like(plane)
    ws = torch.empty(max(l.pd_sweep_bwd_workspace_floats(ctypes.byref(d)) for _, l in libs), device=dev)
    phm = torch.zeros(1, device=dev)
    gphm = torch.ones(1, device=dev)
    st = C.stream_handle(dev)

    def fwd(lib, d=d):
        rc = lib.pd_plane_sweep_fwd(ctypes.byref(d), C.ptr(c["color_l"]), C.ptr(c["color_r"]), C.ptr(c["logits"]),
                                    C.ptr(c["sigma"]), C.ptr(plane), None, None, None, None, C.ptr(rgb), C.ptr(ph), C.ptr(phm),
                                    C.ptr(stash), st)
        assert rc == 0, lib.pd_last_error()

    def bwd(lib, d=d):
        rc = lib.pd_plane_sweep_bwd(ctypes.byref(d), C.ptr(c["color_l"]), C.ptr(c["color_r"]), C.ptr(c["logits"]),
                                    C.ptr(c["sigma"]), C.ptr(plane), None, None, None, None, C.ptr(rgb), C.ptr(stash),
                                    C.ptr(c["g_rgb_rec"]), None, C.ptr(gphm), C.ptr(gl), C.ptr(gs), C.ptr(gp), None, C.ptr(ws), st)
        assert rc == 0, lib.pd_last_error()

    res = {name: {"fwd": [], "bwd": []} for name, _ in libs}
    ref = None
    for name, lib in libs:   # warm up (code objects, power state)
        for _ in range(20):
            fwd(lib, descs[name])
            if not args.fwd_only:
                gp.zero_()
                bwd(lib, descs[name])
        if args.check:
            torch.cuda.synchronize()
            outs = {"rgb_rec": rgb.clone(), "ph_map": ph.clone(), "stash": stash[:, :3].clone(), "g_logits": gl.clone(), "g_sigma": gs.clone(), "g_plane": gp.clone()}
            if ref is None:
                ref = outs
            else:
                print("check %-20s vs %s: " % (name, libs[0][0]) + ", ".join(
                    "%s %.3g (of %.3g)" % (k, float((outs[k] - ref[k]).abs().max()), float(ref[k].abs().max())) for k in outs))
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for name, lib in libs:
            ev = []
            for _ in range(args.iters):
                e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
                e[0].record(); fwd(lib, descs[name]); e[1].record()
                if not args.fwd_only:
                    bwd(lib, descs[name])
                e[2].record()
                ev.append(e)
            torch.cuda.synchronize()
            skip = args.iters // 4
            res[name]["fwd"].append(sum(e[0].elapsed_time(e[1]) for e in ev[skip:]) / (len(ev) - skip))
            res[name]["bwd"].append(sum(e[1].elapsed_time(e[2]) for e in ev[skip:]) / (len(ev) - skip))
    print("%-22s %9s %9s %9s %9s %9s %9s %9s %9s   (ms over %d rounds of %d, impl %d)"
          % ("library", "fwd", "fwd med", "fwd min", "fwd max", "bwd", "bwd med", "bwd min", "bwd max", args.rounds, args.iters, args.impl))
    summary = {}
    med = lambda v: sorted(v)[len(v) // 2] if len(v) % 2 else 0.5 * (sorted(v)[len(v) // 2 - 1] + sorted(v)[len(v) // 2])
    for name, _ in libs:
        f, b = res[name]["fwd"], res[name]["bwd"]
        summary[name] = {"fwd_ms": sum(f) / len(f), "fwd_median_ms": med(f), "fwd_min_ms": min(f), "fwd_max_ms": max(f),
                         "bwd_ms": sum(b) / len(b), "bwd_median_ms": med(b), "bwd_min_ms": min(b), "bwd_max_ms": max(b), "fwd_rounds": f, "bwd_rounds": b}
        print("%-22s %9.4f %9.4f %9.4f %9.4f %9.4f %9.4f %9.4f %9.4f" % (name, sum(f) / len(f), med(f), min(f), max(f), sum(b) / len(b), med(b), min(b), max(b)))
    ref_name = "parent" if "parent" in summary else libs[0][0]   # the arm whose spread the other arms' medians are held against
    first = summary[ref_name]
    for name in summary:
        if name == ref_name:
            continue
        for kk in ("fwd", "bwd"):
            m = summary[name][kk + "_median_ms"]
            summary[name][kk + "_inside_%s_spread" % ref_name] = first[kk + "_min_ms"] <= m <= first[kk + "_max_ms"]
            print("%-22s %s median %.4f %s %s's spread %.4f .. %.4f" % (name, kk, m, "inside" if first[kk + "_min_ms"] <= m <= first[kk + "_max_ms"] else "OUTSIDE",
                                                                       ref_name, first[kk + "_min_ms"], first[kk + "_max_ms"]))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump({"args": vars(args), "results": summary}, fh, indent=1)


if __name__ == "__main__":
    main()
