"""Perceptual feature distance (planedepth_amd.ops.feature_distance, pd_feature_distance.hip) against the reference's
``Trainer.perceptual_loss`` (trainer.py:672-685).

Reference: ``restate`` below — the three reference lines in plain torch, dtype-generic — pinned to the reference's own method by
tests/golden/perceptual.npz (tests/golden/make_perceptual_golden.py), then evaluated in fp64 on the CPU, autograd for the gradient.

Bars (bar 1 of tests/test_operator_sweeps.py):
  fp32   the scalar at 1e-4 relative to the fp64 restatement; the gradient per element,
         ``elementwise_report(got, ref64, rtol=1e-4, floor=1e-4)["frac_beyond"] == 0``;
  bf16   against the restatement on the SAME bf16-rounded inputs with fp32 accumulation: the scalar at 1e-4 relative, every gradient
         element within one bf16 ulp of that fp32 gradient (the kernel rounds an fp32 value once: half an ulp, plus the last bits of
         two fp32 evaluations).
Automask near-ties: a pixel with ``|l_p - l_a| <= 1e-5 * max(l_p, l_a)`` in the fp64 restatement may fall on either side of the
``min`` in fp32 and is left out of the per-element gradient comparison and of the selection-map comparison.  The selection comes
from the fp64 reference alone; its share is capped at 1 % (MAX_SHARE) and ``test_conditions_cpu`` proves for every GPU case,
without a GPU, that the share holds and that the restatement's own fp32 run meets the bars the product is held to.  Inputs:
independent noise on the prediction's and the source's features around the target's, so the two distances differ by O(1/sqrt(C))
of themselves at almost every pixel.

Cases (CASES): the three headline levels at B = 2 and their 384x1280 counterparts (at B = 1: the fp64 reference of a
[1,64,384,1280] level already holds a quarter of a gigabyte per tensor); h*w not a multiple of 4 (63, 297: one pixel per lane),
a multiple of 4 but not of 8 (12: fp32 takes 16-byte lanes, bf16 does not); a base address that is not 16-byte aligned (a slice
along B of a larger buffer with an odd image size, and a view one element into a flat buffer); C in {1, 3, 64, 65, 256} (fewer
channels than the four channel slices of a workgroup, a remainder after the unrolled loop); maps smaller than one workgroup
(15 and 16 pixels) and one spanning several (384); B = 1; each with and without a source, fp32 and bf16.
"""
import ctypes
import json
import math
import os
import subprocess
import sys
import types
import zlib

import numpy as np
import pytest
import torch
from torch import nn

from cases import elementwise_report, rel_err
from conftest import GOLDEN, ROOT

gpu = pytest.mark.gpu
DEV = "cuda"
MAX_SHARE = 0.01      # the project's cap on elements left out of a per-element comparison
NEAR_TIE = 1e-5
G_LOSS = 1.7          # upstream gradient of the scalar in every comparison (so that g_loss is really read)
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}


# =====================================================================================================================
# The reference lines, restated
# =====================================================================================================================
def restate(pred_f, target_f, source_f=None):
    """trainer.py:678-685 on the feature levels themselves."""
    loss = 0
    for i in range(len(pred_f)):
        l_p = ((pred_f[i] - target_f[i]) ** 2).mean(1, True)
        if source_f is not None:
            l_a = ((source_f[i] - target_f[i]) ** 2).mean(1, True)
            l_p, _ = torch.cat([l_p, l_a], dim=1).min(1, True)
        loss = loss + l_p.mean()
    return loss


def restate_with_grad(pred_f, target_f, source_f, dtype):
    """(loss, [gradient per level]) of ``G_LOSS * restate(...)`` evaluated in ``dtype``."""
    p = [t.detach().to(dtype).clone().requires_grad_(True) for t in pred_f]
    t = [x.detach().to(dtype) for x in target_f]
    s = [x.detach().to(dtype) for x in source_f] if source_f is not None else None
    loss = restate(p, t, s)
    grads = torch.autograd.grad(loss * G_LOSS, p)
    return loss.detach(), [g.detach() for g in grads]


def distances(pred_f, target_f, source_f, dtype=torch.float64):
    """(l_p, l_a) [B,h,w] of one level."""
    p, t = pred_f.to(dtype), target_f.to(dtype)
    l_p = ((p - t) ** 2).mean(1)
    l_a = ((source_f.to(dtype) - t) ** 2).mean(1) if source_f is not None else None
    return l_p, l_a


# =====================================================================================================================
# Cases
# =====================================================================================================================
HEADLINE = [(2, 64, 192, 640), (2, 128, 96, 320), (2, 256, 48, 160)]
HEADLINE_HR = [(1, 64, 384, 1280), (1, 128, 192, 640), (1, 256, 96, 320)]
SMALL = [(2, 5, 7, 9), (3, 3, 9, 33), (2, 8, 2, 6), (2, 1, 12, 20), (2, 3, 12, 20), (2, 64, 12, 20), (2, 65, 12, 20),
         (2, 256, 12, 20), (2, 8, 3, 5), (1, 16, 4, 4), (1, 64, 24, 80), (2, 7, 16, 24)]
# (B, C, h, w, source, dtype, layout)
CASES = ([s + (True, "f32", "plain") for s in HEADLINE + HEADLINE_HR] +
         [s + (True, "bf16", "plain") for s in HEADLINE] + [s + (False, "f32", "plain") for s in HEADLINE] +
         [s + (src, dt, "plain") for s in SMALL for src in (True, False) for dt in ("f32", "bf16")] +
         [(2, 3, 7, 9, True, dt, "slice_b") for dt in ("f32", "bf16")] +
         [(2, 8, 8, 16, True, dt, "offset_1") for dt in ("f32", "bf16")] +
         [(2, 8, 8, 16, False, "f32", "offset_1")])


def case_id(spec):
    B, C, h, w, src, dt, layout = spec
    return "%dx%dx%dx%d-%s-%s%s" % (B, C, h, w, "src" if src else "nosrc", dt, "" if layout == "plain" else "-" + layout)


def make_inputs(spec):
    """(pred_f, target_f, source_f | None) on the CPU in the case's dtype: independent noise around the target's features."""
    B, C, h, w, src, dt, _ = spec
    g = torch.Generator().manual_seed(zlib.crc32(repr(spec).encode()) % 100000)
    target = torch.randn(B, C, h, w, generator=g)
    # A single channel of bf16 features has no sum to break ties: with noise of 0.3 the differences to the target lie on a grid
    # of about 2^-9 and one pixel in fifty has |p - t| == |s - t| exactly (1.9 % in the fp64 reference, beyond the cap).  Noise of
    # 4 spreads them over ten times as many grid points.
    amp = 0.3 if C > 1 else 4.0
    pred = target + amp * torch.randn(B, C, h, w, generator=g)
    source = target + amp * torch.randn(B, C, h, w, generator=g) if src else None
    cast = lambda t: None if t is None else t.to(DTYPES[dt])   # noqa: E731
    return cast(pred), cast(target), cast(source)


def references(spec, inputs):
    """What a case is held to, from the restatement alone: fp64 and fp32 runs on the (already rounded) inputs, the near-tie
    pixels and the fp64 selection."""
    pred, target, source = inputs
    lv = lambda t: None if t is None else [t]   # noqa: E731
    loss64, (g64,) = restate_with_grad(lv(pred), lv(target), lv(source), torch.float64)
    loss32, (g32,) = restate_with_grad(lv(pred), lv(target), lv(source), torch.float32)
    l_p, l_a = distances(pred, target, source)
    if source is not None:
        near = (l_p - l_a).abs() <= NEAR_TIE * torch.maximum(l_p, l_a)
        sel = l_p <= l_a
    else:
        near = torch.zeros_like(l_p, dtype=torch.bool)
        sel = torch.ones_like(l_p, dtype=torch.bool)
    share = float(near.double().mean())
    assert share <= MAX_SHARE, "%s: %.3f %% of the pixels are near-ties (at most 1 %%)" % (case_id(spec), 100 * share)
    return dict(loss64=loss64, g64=g64, loss32=loss32, g32=g32, near=near, sel=sel, share=share)


def bf16_ulp(ref):
    """One bf16 unit in the last place at the magnitude of each element of ``ref`` (8 significant bits)."""
    _, e = torch.frexp(ref.double().abs())          # |ref| = m * 2^e, m in [0.5, 1)
    return torch.ldexp(torch.ones_like(ref, dtype=torch.float64), (e - 8).clamp_min(-133))


def hold_to_bars(spec, who, loss, grad, sel, ref):
    """The bars of the module docstring on one result (the product's on the GPU, the restatement's fp32 run on the CPU)."""
    dt = spec[5]
    keep = ~ref["near"]
    keep_e = keep[:, None].expand_as(ref["g64"])
    if sel is not None:
        assert torch.equal(sel.bool()[keep], ref["sel"][keep]), "%s %s: selection map differs outside the near-ties" % (who, case_id(spec))
    if dt == "f32":
        e = abs(float(loss) - float(ref["loss64"])) / abs(float(ref["loss64"]))
        rep = elementwise_report(grad[keep_e], ref["g64"][keep_e], rtol=1e-4, floor=1e-4)
        print("%s %s: loss rel err %.3e, gradient %s, near-tie share %.2e" % (who, case_id(spec), e, rep, ref["share"]))
        assert e <= 1e-4, (who, case_id(spec), e)
        assert math.isfinite(rep["worst_over_allowance"]) and rep["frac_beyond"] == 0, (who, case_id(spec), rep)
    else:
        e = abs(float(loss) - float(ref["loss32"])) / abs(float(ref["loss32"]))
        got, want = grad.double()[keep_e], ref["g32"].double()[keep_e]
        err = (got - want).abs()
        worst = float((err / bf16_ulp(want)).max())
        print("%s %s: loss rel err %.3e, gradient worst %.3f bf16 ulp, near-tie share %.2e" % (who, case_id(spec), e, worst, ref["share"]))
        assert e <= 1e-4, (who, case_id(spec), e)
        assert worst <= 1.0, (who, case_id(spec), worst)
        assert bool((got[want == 0] == 0).all())


@pytest.mark.parametrize("spec", CASES, ids=[case_id(s) for s in CASES])
def test_conditions_cpu(spec):
    """Every GPU case, without a GPU: the near-tie share is inside the cap (asserted in ``references``) and the restatement's own
    fp32 run (for bf16: rounded to bf16 once, as the kernel does) meets the bars the product is held to."""
    inputs = make_inputs(spec)
    ref = references(spec, inputs)
    grad = ref["g32"] if spec[5] == "f32" else ref["g32"].to(torch.bfloat16)
    l_p, l_a = distances(*inputs, dtype=torch.float32)
    sel32 = (l_p <= l_a) if l_a is not None else torch.ones_like(l_p, dtype=torch.bool)
    hold_to_bars(spec, "restatement_fp32", ref["loss32"], grad, sel32, ref)


def test_case_table_covers_the_kernel_constants():
    """A later edit that drops one of the sizes the kernels' constants ask for fails here, without a GPU."""
    assert {s[1] for s in CASES} >= {1, 3, 64, 65, 256} and {s[0] for s in CASES} >= {1, 2, 3}
    hw = {s[2] * s[3] for s in CASES}
    assert hw >= {15, 16, 12, 63, 297, 384, 192 * 640, 96 * 320, 48 * 160, 384 * 1280}
    assert {s[4:6] for s in CASES} == {(True, "f32"), (False, "f32"), (True, "bf16"), (False, "bf16")}
    assert {s[6] for s in CASES} == {"plain", "slice_b", "offset_1"}
    assert set(HEADLINE) | set(HEADLINE_HR) <= {s[:4] for s in CASES if s[4:] == (True, "f32", "plain")}


# =====================================================================================================================
# CPU: the restatement is the reference's method; the boundary refuses on the host
# =====================================================================================================================
def load_golden():
    z = np.load(os.path.join(GOLDEN, "perceptual.npz"))
    meta = json.loads(bytes(z["meta"]).decode())
    return {k: torch.from_numpy(z[k]) for k in z.files if k != "meta"}, meta


def test_restatement_equals_the_reference_fixture():
    """tests/golden/perceptual.npz holds what the reference's Trainer.perceptual_loss returned, and the gradient it sent to the
    prediction's features, on a seeded stand-in net: the restatement gives the same, with and without a source."""
    z, meta = load_golden()
    n = meta["levels"]
    assert n == 3 and [tuple(z["pred_f%d" % i].shape) for i in range(n)] == [(2, 8, 12, 20), (2, 16, 6, 10), (2, 32, 3, 5)]
    pred, target, source = ([z["%s_f%d" % (k, i)] for i in range(n)] for k in ("pred", "target", "source"))
    picked = []
    for tag, src in (("plain", None), ("auto", source)):
        p = [t.clone().requires_grad_(True) for t in pred]
        loss = restate(p, target, src)
        grads = torch.autograd.grad(loss, p)
        assert rel_err(loss.detach(), z["loss_" + tag]) <= 1e-6, tag
        for i in range(n):
            assert rel_err(grads[i], z["g_%s_%d" % (tag, i)]) <= 1e-6, (tag, i)
            picked.append(float((z["g_%s_%d" % (tag, i)] != 0).double().mean()))
    assert float(z["loss_auto"]) < float(z["loss_plain"])            # the min took the source's branch somewhere ...
    assert all(0.05 < f < 0.95 for f in picked[n:]), picked           # ... at every level, and not everywhere


def _lib():
    from planedepth_amd import _capi as C
    return C, C.load()


def test_host_side_refusals_need_no_gpu():
    C, lib = _lib()
    one = ctypes.c_void_p(64)    # a non-NULL address nothing dereferences: every call below is refused before any launch
    fwd = lambda B, Cc, h, w, dt, *p: lib.pd_feature_distance_fwd(B, Cc, h, w, dt, *p, 0, None)   # noqa: E731
    bwd = lambda B, Cc, h, w, dt, *p: lib.pd_feature_distance_bwd(B, Cc, h, w, dt, *p, None)      # noqa: E731
    err = lambda: lib.pd_last_error()   # noqa: E731
    for call, n in ((fwd, 6), (bwd, 5)):
        for shape in ((0, 8, 4, 4), (1, 0, 4, 4), (1, 8, 0, 4), (1, 8, 4, -1)):
            assert call(*shape, C.PD_DTYPE_F32, *([one] * n)) == 1 and b"positive" in err(), shape
        assert call(65536, 8, 4, 4, C.PD_DTYPE_F32, *([one] * n)) == 1 and b"65535" in err()
        assert call(2, 8, 32768, 32768, C.PD_DTYPE_F32, *([one] * n)) == 1 and b"2^31" in err()
        assert call(1, 8, 65536, 32768, C.PD_DTYPE_BF16, *([one] * n)) == 1 and b"2^31" in err()
        for dt in (2, -1, 7):
            assert call(1, 8, 4, 4, dt, *([one] * n)) == 1 and b"dtype %d" % dt in err()
        assert call(1, 8, 4, 4, C.PD_DTYPE_F32, *([None] * n)) == 1 and b"NULL" in err()
    # each required pointer on its own; the forward's source (slot 2) may be NULL
    for k in (0, 1, 3, 4, 5):
        p = [one] * 6
        p[k] = None
        assert fwd(1, 8, 4, 4, C.PD_DTYPE_BF16, *p) == 1 and b"NULL" in err(), k
    for k in range(5):
        p = [one] * 5
        p[k] = None
        assert bwd(1, 8, 4, 4, C.PD_DTYPE_F32, *p) == 1 and b"NULL" in err(), k


def test_operator_refuses_cpu_tensors_and_gradients_it_cannot_give():
    from planedepth_amd import ops
    from planedepth_amd._capi import PlaneDepthHipError
    p, t, s = (torch.randn(2, 4, 3, 5) for _ in range(3))
    with pytest.raises(PlaneDepthHipError):
        ops.feature_distance(p, t)
    with pytest.raises(PlaneDepthHipError):
        ops.feature_distance([p, p], [t, t], [s, s])
    with pytest.raises(ValueError, match="requires grad"):
        ops.feature_distance(p, t.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="requires grad"):
        ops.feature_distance([p], [t], [s.clone().requires_grad_(True)])
    with pytest.raises(ValueError, match="levels"):
        ops.feature_distance([p, p], [t])
    with pytest.raises(TypeError, match="float16"):
        ops.feature_distance(p.half(), t.half())
    with pytest.raises(ValueError):
        ops.feature_distance(p[0], t[0])
    import planedepth_amd
    assert planedepth_amd.patch_trainer_perceptual and planedepth_amd.perceptual_loss is planedepth_amd.trainer_path.perceptual_loss

    class T:
        pass
    before = dict(vars(T))
    planedepth_amd.patch_trainer(T)
    assert "perceptual_loss" not in vars(T) and "perceptual_loss" not in before     # patch_trainer leaves it alone
    planedepth_amd.patch_trainer_perceptual(T)
    assert T.perceptual_loss is planedepth_amd.perceptual_loss


# =====================================================================================================================
# GPU
# =====================================================================================================================
def place(t, layout):
    """The tensor on the device in the case's memory layout: contiguous in every layout, so the operator reads it in place."""
    if t is None:
        return None
    if layout == "plain":
        out = t.to(DEV)
    elif layout == "slice_b":
        big = torch.empty((t.shape[0] + 1,) + tuple(t.shape[1:]), dtype=t.dtype, device=DEV)
        out = big[1:]
        out.copy_(t)
    else:
        flat = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
        out = flat[1:].view(t.shape)
        out.copy_(t)
    assert out.is_contiguous() and (layout == "plain" or out.data_ptr() % 16 != 0)
    return out


def abi_forward(p, t, s, loss=None, accumulate=0):
    """pd_feature_distance_fwd on device tensors -> (loss [1], sel [B,h,w] uint8)."""
    C, lib = _lib()
    B, Cc, h, w = p.shape
    sel = torch.empty(B, h, w, dtype=torch.uint8, device=p.device)
    partials = torch.empty(B * ((h * w + 63) // 64), device=p.device)
    loss = torch.empty(1, device=p.device) if loss is None else loss
    dt = C.PD_DTYPE_BF16 if p.dtype == torch.bfloat16 else C.PD_DTYPE_F32
    C.check(lib.pd_feature_distance_fwd(B, Cc, h, w, dt, C.ptr(p), C.ptr(t), C.ptr(s), C.ptr(sel), C.ptr(partials), C.ptr(loss),
                                        accumulate, C.stream_handle(p.device)), "pd_feature_distance_fwd")
    return loss, sel


def run_operator(p, t, s):
    from planedepth_amd import ops
    p = p.detach().requires_grad_(True)
    loss = ops.feature_distance(p, t, s)
    g, = torch.autograd.grad(loss * G_LOSS, p)
    return loss.detach(), g


@gpu
@pytest.mark.parametrize("spec", CASES, ids=[case_id(s) for s in CASES])
def test_parity(spec):
    """Value, gradient and selection map against the restatement; unselected pixels hold exact zeros; two runs give the same
    bits (value, map, gradient)."""
    inputs = make_inputs(spec)
    ref = references(spec, inputs)
    p, t, s = (place(x, spec[6]) for x in inputs)
    loss, g = run_operator(p, t, s)
    abi_loss, sel = abi_forward(p, t, s)
    assert loss.dtype == torch.float32 and loss.dim() == 0 and g.dtype == p.dtype and g.shape == p.shape
    assert torch.equal(abi_loss.reshape(()), loss)
    hold_to_bars(spec, "product", loss.cpu(), g.cpu(), sel.cpu(), ref)
    assert bool(((sel == 0) | (sel == 1)).all())
    off = (sel == 0)[:, None].expand_as(g)
    assert bool((g[off].view(torch.int16 if spec[5] == "bf16" else torch.int32) == 0).all())     # +0.0, bit for bit
    if not spec[4]:
        assert bool((sel == 1).all())
    loss2, g2 = run_operator(p, t, s)
    _, sel2 = abi_forward(p, t, s)
    assert torch.equal(loss2.view(torch.int32), loss.view(torch.int32)) and torch.equal(sel2, sel)
    assert torch.equal(g2.view(torch.int16 if spec[5] == "bf16" else torch.int32), g.view(torch.int16 if spec[5] == "bf16" else torch.int32))


@gpu
@pytest.mark.parametrize("spec", [(2, 64, 12, 20, True, "f32", "plain"), (2, 65, 7, 9, True, "f32", "plain"),
                                  (2, 64, 12, 20, True, "bf16", "plain"), (3, 3, 9, 33, True, "bf16", "plain"),
                                  (2, 128, 96, 320, True, "f32", "plain")], ids=case_id)
def test_exact_ties_select_the_prediction(spec):
    """source_f = pred_f.clone(): a tie at every pixel, bit for bit, and the prediction takes it: the gradient is the no-source
    gradient, bit for bit, and non-zero wherever pred differs from target."""
    pred, target, _ = make_inputs(spec)
    p, t = pred.to(DEV), target.to(DEV)
    s = p.clone()
    loss_tie, g_tie = run_operator(p, t, s)
    loss_plain, g_plain = run_operator(p, t, None)
    _, sel = abi_forward(p, t, s)
    assert bool((sel == 1).all())
    as_int = torch.int16 if spec[5] == "bf16" else torch.int32
    assert torch.equal(loss_tie.view(torch.int32), loss_plain.view(torch.int32))
    assert torch.equal(g_tie.view(as_int), g_plain.view(as_int))
    if spec[5] == "f32":   # (a bf16 gradient element may round to zero at the bottom of the range only; here none is that small)
        assert bool(((g_tie != 0) | (p == t)).all())
    assert float((g_tie != 0).double().mean()) > 0.99


@gpu
def test_non_contiguous_features_are_copied():
    """Channels-last and sliced features give what their contiguous copies give (the operator copies them)."""
    spec = (2, 16, 12, 20, True, "f32", "plain")
    pred, target, source = (x.to(DEV) for x in make_inputs(spec))
    want = run_operator(pred, target, source)
    got = run_operator(pred.contiguous(memory_format=torch.channels_last), target.contiguous(memory_format=torch.channels_last),
                       source.contiguous(memory_format=torch.channels_last))
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    wide = torch.randn(2, 16, 12, 31, device=DEV)
    wide[..., 3:23] = pred
    got = run_operator(wide[..., 3:23], target, source)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


@gpu
def test_levels_accumulate_on_the_device():
    """The three levels through one operator call equal the sum of three single-level calls (the finishing kernel's accumulate
    switch adds in level order, as the Python sum does), value and gradients; a bare tensor is one level."""
    from planedepth_amd import ops
    shapes = [(2, 64, 24, 80), (2, 128, 12, 40), (2, 256, 6, 20)]
    feats = [[x.to(DEV) for x in make_inputs(s + (True, "f32", "plain"))] for s in shapes]
    for with_source in (True, False):
        preds = [f[0].clone().requires_grad_(True) for f in feats]
        targets, sources = [f[1] for f in feats], [f[2] for f in feats] if with_source else None
        total = ops.feature_distance(preds, targets, sources)
        grads = torch.autograd.grad(total * G_LOSS, preds)
        single, s_grads = torch.zeros((), device=DEV), []
        for i in range(3):
            p = feats[i][0].clone().requires_grad_(True)
            one = ops.feature_distance(p, targets[i], sources[i] if with_source else None)
            s_grads.append(torch.autograd.grad(one * G_LOSS, p)[0])
            single = single + one
        assert torch.equal(total, single), (float(total), float(single))
        for a, b in zip(grads, s_grads):
            assert torch.equal(a, b)
        # the ABI's switch itself: accumulate = 1 adds to what `loss` holds
        loss = torch.full((1,), 3.0, device=DEV)
        first, _ = abi_forward(feats[0][0], feats[0][1], None)
        abi_forward(feats[0][0], feats[0][1], None, loss=loss, accumulate=1)
        assert torch.equal(loss, first + 3.0)
    # mixed precision across levels: each level in its own dtype
    mixed = ops.feature_distance([feats[0][0], feats[1][0].bfloat16()], [feats[0][1], feats[1][1].bfloat16()])
    want = ops.feature_distance(feats[0][0], feats[0][1]) + ops.feature_distance(feats[1][0].bfloat16(), feats[1][1].bfloat16())
    assert torch.equal(mixed, want)


# ---------------------------------------------------------------------------------------------------------------------
# Every element written, nothing written beyond: the C entry points on buffers pre-filled with a recognisable pattern (a quiet NaN
# no kernel produces for the float outputs, a byte that is neither 0 nor 1 for the map) and guard bytes behind the documented
# extent.  Reads of memory the test owns; nothing is provoked.
# ---------------------------------------------------------------------------------------------------------------------
GUARD = 1024   # bytes
PATTERNS = {torch.float32: 0x7FC0BEEF, torch.bfloat16: 0x7FC1, torch.uint8: 0xEE}
AS_INT = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.uint8: torch.uint8}


class Guarded:
    def __init__(self, n, dtype):
        self.n, self.dtype = n, dtype
        pat = PATTERNS[dtype]
        self.pat = pat - (1 << 16) if (dtype == torch.bfloat16 and pat >= 1 << 15) else pat
        self.buf = torch.full((n + GUARD // max(1, torch.empty(0, dtype=dtype).element_size()),), self.pat, dtype=AS_INT[dtype], device=DEV)

    @property
    def ptr(self):
        return ctypes.c_void_p(self.buf.data_ptr())

    def check(self, what, written=None):
        host = self.buf.cpu()
        assert bool((host[self.n:] == self.pat).all()), "%s: written past its end" % what
        w = self.n if written is None else written
        left = int((host[:w] == self.pat).sum())
        assert left == 0, "%s: %d of %d elements never written" % (what, left, w)

    def values(self):
        return self.buf[:self.n].view(self.dtype)


def guarded_input(t):
    g = Guarded(t.numel(), t.dtype)
    g.values().copy_(t.reshape(-1).to(DEV))
    return g


@gpu
@pytest.mark.parametrize("B,C,h,w", [(3, 5, 9, 33), (3, 4, 1, 257), (3, 9, 257, 2), (2, 6, 16, 24), (2, 3, 2, 6)])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_guards(B, C, h, w, dt):
    Cc, lib = _lib()
    dtype = DTYPES[dt]
    code = Cc.PD_DTYPE_BF16 if dt == "bf16" else Cc.PD_DTYPE_F32
    pred, target, source = make_inputs((B, C, h, w, True, dt, "plain"))
    n, npix, npart = B * C * h * w, B * h * w, B * ((h * w + 63) // 64)
    p, t, s = guarded_input(pred), guarded_input(target), guarded_input(source)   # a read past an input's end brings the NaN in
    stream = Cc.stream_handle(torch.device(DEV))
    for src in (s, None):
        sel, partials, loss, g = Guarded(npix, torch.uint8), Guarded(npart, torch.float32), Guarded(1, torch.float32), Guarded(n, dtype)
        Cc.check(lib.pd_feature_distance_fwd(B, C, h, w, code, p.ptr, t.ptr, src.ptr if src else None, sel.ptr, partials.ptr,
                                             loss.ptr, 0, stream), "pd_feature_distance_fwd")
        torch.cuda.synchronize()
        sel.check("fwd sel"), loss.check("fwd loss"), partials.check("fwd partials", written=0)
        assert bool(torch.isfinite(loss.values()).all()) and bool((sel.values() <= 1).all())
        want = restate([pred.float()], [target.float()], [source.float()] if src else None)
        assert rel_err(loss.values().cpu()[0], want) <= 1e-4
        g_loss = torch.full((1,), G_LOSS, device=DEV)
        Cc.check(lib.pd_feature_distance_bwd(B, C, h, w, code, p.ptr, t.ptr, sel.ptr, Cc.ptr(g_loss), g.ptr, stream),
                 "pd_feature_distance_bwd")
        torch.cuda.synchronize()
        g.check("bwd g_pred")
        assert bool(torch.isfinite(g.values().float()).all())
        for inp in (p, t, s):
            inp.check("an input", written=0)     # inputs and their guards untouched


@gpu
def test_stream_and_graph_replay_in_a_child_process():
    """The operator enqueues on torch's current stream (a side stream's producer is waited for, in stream order) and survives
    capture and replay in a single-stream torch.cuda.graph — in a process of its own with its own time limit, so that a
    capture that goes wrong cannot take the suite down."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "feature_distance_graph_check.py")], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and "stream and graph replay: ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])


# ---------------------------------------------------------------------------------------------------------------------
# Trainer level: patch_trainer + patch_trainer_perceptual against the same trainer with the reference formulation in torch
# ---------------------------------------------------------------------------------------------------------------------
class StandInNet(nn.Module):
    """Seeded three-level convolutional stand-in for the perceptual net: 64 @ H, 128 @ H/2, 256 @ H/4, frozen."""

    def __init__(self, seed=5):
        super().__init__()
        torch.manual_seed(seed)
        self.slice1 = nn.Sequential(nn.Conv2d(3, 64, 3, padding=1), nn.ReLU())
        self.slice2 = nn.Sequential(nn.MaxPool2d(2), nn.Conv2d(64, 128, 3, padding=1), nn.ReLU())
        self.slice3 = nn.Sequential(nn.MaxPool2d(2), nn.Conv2d(128, 256, 3, padding=1), nn.ReLU())
        for p in self.parameters():
            p.requires_grad = False

    def forward(self, x):
        f1 = self.slice1(x)
        f2 = self.slice2(f1)
        return f1, f2, self.slice3(f2)


def torch_perceptual_loss(self, pred, target, source=None):
    """The reference formulation on the device: the other arm of the trainer-level comparison."""
    pred_f, target_f = self.pc_net(pred), self.pc_net(target)
    source_f = self.pc_net(source) if source is not None else None
    return restate(pred_f[:3], target_f[:3], None if source_f is None else source_f[:3])


def run_trainer(case, fused, automask, mask_novel):
    import planedepth_amd
    c = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in case.items()}
    B, N, H, W = c["logits"].shape
    logits, sigma = c["logits"].clone().requires_grad_(True), c["sigma"].clone().requires_grad_(True)
    disp_layered = c["disp_pp"].expand(-1, -1, H, W)
    inputs = {("color", "l"): c["color_l"], ("color", "r"): c["color_r"], "K": c["K"], "inv_K": c["inv_K"]}
    outputs = {"probability": torch.empty(B, N, H, W, device="meta"), "logits": logits, "sigma": sigma,
               "disp_layered": disp_layered, "padding_mask": c["padding_mask"],
               "disp": (torch.softmax(logits.detach(), 1) * disp_layered).sum(1, True)}
    if mask_novel:
        outputs["mask_novel"] = torch.rand(B, 1, H, W, generator=torch.Generator().manual_seed(9)).to(DEV)
    opt = types.SimpleNamespace(warp_type="disp_warp", match_aug=False, use_mixture_loss=True, automask=automask,
                                render_probability=False, alpha_pc=0.1, alpha_self=0.0, self_distillation=0.0,
                                gamma_smooth=2.0, alpha_smooth=0.04, use_ssim=True)

    class StubTrainer:
        def __init__(self):
            self.opt, self.target_sides, self.device = opt, ["r"], torch.device(DEV)
            self.pc_net = StandInNet().to(DEV)

    planedepth_amd.patch_trainer(StubTrainer)
    assert not hasattr(StubTrainer, "perceptual_loss")
    if fused:
        planedepth_amd.patch_trainer_perceptual(StubTrainer)
    else:
        StubTrainer.perceptual_loss = torch_perceptual_loss
    trainer = StubTrainer()
    trainer.pred_novel_images(inputs, outputs)
    losses = trainer.compute_losses(inputs, outputs)
    losses["loss/total_loss"].backward()
    return {"loss/pc_loss": losses["loss/pc_loss"], "loss/total_loss": losses["loss/total_loss"], "g_logits": logits.grad,
            "g_sigma": sigma.grad}


@gpu
@pytest.mark.parametrize("automask,mask_novel", [(False, False), (True, False), (True, True)],
                         ids=["plain", "automask", "automask-mask_novel"])
def test_trainer_with_the_fused_perceptual_loss(automask, mask_novel):
    """compute_losses with alpha_pc > 0 through a stub Trainer: both arms run the same convolutions, so the difference is the new
    operator alone — loss/pc_loss, loss/total_loss, g_logits, g_sigma at 1e-4 relative."""
    from planedepth_amd.synthetic import build_case
    case = build_case(B=2, N=9, H=24, W=80, seed=11, disp_min=0.5, disp_max=40.0, sigma_interior=True)
    got = run_trainer(case, True, automask, mask_novel)
    want = run_trainer(case, False, automask, mask_novel)
    assert float(want["loss/pc_loss"]) > 0 and float(want["g_logits"].abs().max()) > 0
    for k in ("loss/pc_loss", "loss/total_loss", "g_logits", "g_sigma"):
        e = rel_err(got[k].detach().cpu(), want[k].detach().cpu())
        print("trainer %s %s: rel err %.3e" % ("automask" if automask else "plain", k, e))
        assert e <= 1e-4, (k, e)
