"""Novel views at inference (pd_render_views): every kernel instantiation, per PIXEL against the oracle in fp64.

tests/test_render_views.py holds the operator to the fp32 oracle under ``cases.rel_err`` — max|a-b| / max|b| of the tensor, with
max|b| ~ 1 for rgb and coverage: a pixel worth 0.01 may be 1 % wrong there.  Such pixels are the normal case for this operator (a
plane shifted out of view enters the mixture with sigma_rec clamped to 0.01: 100 times the weight in the normaliser), and they
are where the guard cells, the tap clamp, ``clamp_shift``, the target-row mask and the online softmax's rescale act.

One table (``CASES``).  Each row states, written down by hand from the rule (W > 1024, or W >= 513 and V <= 2), how many columns a
lane owns in the launches it makes; ``ops.render_cols_per_lane`` — the function the entry point itself switches on — must agree, on
the CPU, and the table must reach each of the 32 instantiations (fp32 | bf16) x (mixture | not) x V = 1..4 x (1 | 2 columns).

Reference: tests/test_render_views.py's composition — ``oracle.decoder_tail``, ``oracle.disp_grid(float32(s) * disp_layered,
"r")``, ``oracle.plane_sweep`` of the image and of a ones image, ``(probability_rec * disp_layered).sum(1)`` — run twice on the
CPU on the exactly widened inputs, in fp64 and in fp32.

Measure, per output (rgb, coverage, disp) of one view: ``cases.px_report`` with FLOOR,
    px_err(a, ref) = max over pixels of |a - ref| / max(|ref|, FLOOR * max|ref|),
pixels whose fp64 reference is exactly 0 apart (|a| <= 1e-6 * max|ref| there, and counted).

The bar (GPU):  px_err(product, fp64) <= 2 * E_ref + 1e-4,  E_ref = px_err(oracle fp32, fp64) of the same case, view and output.
The factor 2 and the 1e-4 are ``cases.three_way``'s; the tails, which use the same __expf / fast_rcp, are held to 1e-4 relative.
``test_conditions_cpu`` proves from the references alone what keeps that bar from hiding a failure: E_ref <= 1e-3 for every output,
view and case; per case at least 0.5 % of the pixels of its views have 0 < coverage < 0.05 and at least 10 % have coverage > 0.5.
``test_floor_is_the_smallest_that_holds``: FLOOR is the smallest of 1e-3, 1e-2, 1e-1 at which E_ref <= 1e-3 holds for the table.

Inputs.  Logits, raw sigma and the image are band-limited (noise at 1/16 resolution, bicubic: test_post_process_routes's
``_band_limited``); raw sigma has smooth regions <= -12 and >= 30 (both ends of the clamp).  All logits are lowered by 7 over the
outer tenth of the source row on each side (a smooth gate): where the far planes have left the view, what is still in view is
weak against the out-of-view planes' logit 0 — the weak pixels this module exists for, without the mixture too; and they shrink to
min(1, 64 / W) of their value over the 16 columns next to the border (test_post_process_routes's ``_border_window``: zero padding
makes a step of the border logit's size at the edge of view, which the fp32 coordinate chain turns into E_ref in proportion to W).
E_ref is heavy-tailed all the same — it is set by the one pixel per plane and row whose tap straddles the edge of view, where the
mixture's 1 / clamp(sigma_rec, .01, 1) is steep: 1.3e-4 .. 1.9e-3 over seven draws of one case — so the ``draw`` of six cases was
moved on until E_ref stayed under E_REF_MAX with a margin (chosen from the references alone, on the CPU).  Disparities as
the decoders space them, up to 0.47 W; from N = 5 on plane 0 has d = W - 1 (column 0 lands on column W - 1), plane 1 an even
integer (s * d is an integer for s = 1, -1, 0.5, -0.5), the last plane d = 0, and plane N // 2 has its logits lowered by 8
(probability ~1e-4).  N = 2..4: the even integer and d = 0.  N = 1: d = k + 0.97, which leaves one column of coverage 0.03.
The forward is continuous in the sampling coordinate, so no margin from integers is kept and no pixel is excluded.
``order``: logits strictly increasing with the plane index at every pixel (the running maximum moves at every plane), strictly
decreasing (it never moves), or +40 on planes 1 and 3 and -40 on the others (the rescale factor underflows).

The far baselines (1e6, -1e6, 3e38, 1e-30) run on four rows whose d = 0 plane is given a positive disparity (s * 0 is in view at
any s).  For the first three every plane is out of view: rgb and coverage must be exactly 0 and disp the fp64 reference's (every
plane enters with logit 0 and sigma 0.01), within the bar's 1e-4 alone — 3e38 * d overflows fp32, where the oracle's own fp32 run
is NaN.  1e-30 * d is far below half an ulp of any column: that view IS the source camera, so its coverage is 1 in the interior,
not 0; it is held to the fp64 reference under the bar like any other view.

PD_RENDER_PARITY_JSON=<file> writes, per case and view, the columns per lane, E_ref, the product's px_err, the share of weak
pixels and the count of zero pixels: the source of profiles/render_views_parity.md."""
import functools
import json
import math
import os
import zlib
from typing import NamedTuple

import pytest
import torch
import torch.nn.functional as F

from cases import px_report
from oracle import planedepth_oracle as orc
from planedepth_amd import ops

gpu = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
FLOOR = 1e-3          # the smallest of 1e-3, 1e-2, 1e-1 at which E_ref <= E_REF_MAX for the whole table
E_REF_MAX = 1e-3
FACTOR, TOL = 2.0, 1e-4
WEAK_BELOW, WEAK_SHARE, STRONG_ABOVE, STRONG_SHARE = 0.05, 0.005, 0.5, 0.10
MAX_VIEWS = 4         # PD_RENDER_MAX_VIEWS: ops.render_views serves a longer list in chunks of four, per image
OUTPUTS = ("rgb", "coverage", "disp")
REPORT = {}

V1, V1L, V2, V3, V4 = (1.0,), (-1.0,), (0.5, -0.5), (1.0, -1.0, 0.25), (1.0, -1.0, 0.25, 3.0)
V5 = (1.0, -1.0, 0.5, 0.25, 3.0)
V9 = (1.0, -1.0, 0.5, -0.5, 0.25, -0.25, 2.0, -2.0, 3.0)
FAR = (1e6, -1e6, 3e38, 1e-30)


class Case(NamedTuple):
    name: str
    shape: tuple            # (B, N, H, W)
    bf16: bool
    mix: bool
    views: tuple            # the baseline set
    cpl: int                # columns per lane the launches are meant to take, by hand from the rule
    form: str = "plane"     # disparities: plane | rows (a row view) | rows_slice (view[:B] of a larger row view)
    mask: str = "none"      # none | rows (a row view; with rows_slice a batch slice too)
    applied: bool = False   # tail_applied: logits / sigma as a tail wrote them
    order: str = "rand"     # rand | inc | dec | spread
    draw: int = 0           # which seeded draw of the inputs: moved on where a case misses a condition of test_conditions_cpu
    gain: float = 0.2       # rows: the per-row disparity gain is in [1 - gain, 1]


CASES = [
    # ---- fp32, mixture
    Case("f32_mix_v1_w64_rows",   (2,  9, 14,   64), False, True,  V1,  1, form="rows", mask="rows"),
    Case("f32_mix_v2_w66_n2",     (1,  2, 14,   66), False, True,  V2,  1),
    Case("f32_mix_v3_w130_n49",   (1, 49, 14,  130), False, True,  V3,  1),
    Case("f32_mix_v4_w1024",      (1,  9, 14, 1024), False, True,  V4,  1, applied=True, draw=1),
    Case("f32_mix_v1_w514",       (1,  9, 14,  514), False, True,  V1L, 2),   # threads = 320: lanes 194..319 own no second column
    Case("f32_mix_v2_w1024_h7",   (1,  5,  7, 1024), False, True,  V2,  2),
    Case("f32_mix_v3_w1026",      (1,  5, 14, 1026), False, True,  V3,  2),   # threads = 576: the second column partial
    Case("f32_mix_v4_w2048",      (1,  5, 14, 2048), False, True,  V4,  2, draw=6),
    # ---- fp32, no mixture
    Case("f32_pi_v1_w66_n63",     (1, 63, 14,   66), False, False, V1L, 1),
    Case("f32_pi_v2_w130_rows",   (2,  9, 14,  130), False, False, V2,  1, form="rows", mask="rows", applied=True),
    Case("f32_pi_v3_w514",        (1,  5, 14,  514), False, False, V3,  1),
    Case("f32_pi_v4_w64_n65",     (1, 65, 14,   64), False, False, V4,  1),
    Case("f32_pi_v1_w1024",       (1,  5, 14, 1024), False, False, V1,  2),
    Case("f32_pi_v2_w514",        (1,  9, 14,  514), False, False, V2,  2),
    Case("f32_pi_v3_w2048",       (1,  2, 14, 2048), False, False, V3,  2),
    Case("f32_pi_v4_w1026",       (1,  5, 14, 1026), False, False, V4,  2, applied=True),
    # ---- bf16, mixture
    Case("bf16_mix_v1_w130_n65",  (1, 65, 14,  130), True,  True,  V1,  1),
    Case("bf16_mix_v2_w64_n49",   (1, 49, 14,   64), True,  True,  V2,  1),
    Case("bf16_mix_v3_w66_slice", (2,  9, 14,   66), True,  True,  V3,  1, form="rows_slice", mask="rows"),
    Case("bf16_mix_v4_w514",      (1,  5, 14,  514), True,  True,  V4,  1, draw=1),
    Case("bf16_mix_v1_w1024",     (1,  5, 14, 1024), True,  True,  V1L, 2, applied=True),
    Case("bf16_mix_v2_w514",      (1,  9, 14,  514), True,  True,  V2,  2, draw=6),
    Case("bf16_mix_v3_w1026",     (1,  5, 14, 1026), True,  True,  V3,  2, draw=1),
    Case("bf16_mix_v4_w2048",     (1,  2, 14, 2048), True,  True,  V4,  2),
    # ---- bf16, no mixture
    Case("bf16_pi_v1_w64_n1",     (1,  1, 14,   64), True,  False, V1,  1),
    Case("bf16_pi_v2_w66_n63",    (1, 63, 14,   66), True,  False, V2,  1),
    Case("bf16_pi_v3_w130",       (1,  9, 14,  130), True,  False, V3,  1, applied=True),
    Case("bf16_pi_v4_w130_rows",  (2,  9, 14,  130), True,  False, V4,  1, form="rows", mask="rows"),
    Case("bf16_pi_v1_w514",       (1,  5, 14,  514), True,  False, V1L, 2),
    Case("bf16_pi_v2_w1024",      (1,  5, 14, 1024), True,  False, V2,  2),
    Case("bf16_pi_v3_w2048",      (1,  5, 14, 2048), True,  False, V3,  2, draw=1),
    Case("bf16_pi_v4_w1026",      (1,  9, 14, 1026), True,  False, V4,  2),
    # ---- the entry point's minimum; the logit orders; lists longer than a launch (chunks of 4, per image: B = 2, row masks)
    Case("min_w2_h2",             (1,  1,  2,    2), False, True,  V1,  1),
    Case("inc_w66",               (1,  9, 14,   66), False, True,  V2,  1, order="inc"),
    Case("dec_w66",               (1,  9, 14,   66), True,  True,  V2,  1, order="dec"),
    Case("spread_w130",           (1,  9, 14,  130), False, False, V3,  1, order="spread"),
    Case("chunk5_w64",            (2,  9, 14,   64), False, True,  V5,  1, form="rows", mask="rows"),
    Case("chunk9_w66",            (2,  5, 14,   66), True,  False, V9,  1, form="rows", mask="rows"),
]
BY_NAME = {c.name: c for c in CASES}
IDS = [c.name for c in CASES]
FAR_CASES = ["f32_mix_v1_w64_rows", "f32_pi_v1_w66_n63", "bf16_mix_v3_w66_slice", "bf16_pi_v3_w130"]
LAYOUT_CASES = ["f32_mix_v1_w64_rows", "f32_pi_v2_w130_rows", "bf16_mix_v3_w66_slice", "bf16_pi_v4_w130_rows"]


def launches(c):
    """The view counts of the launches ``ops.render_views`` makes for a case's baseline set."""
    V = len(c.views)
    return [min(MAX_VIEWS, V - v0) for v0 in range(0, V, MAX_VIEWS)]


# =====================================================================================================================
# Inputs and references
# =====================================================================================================================
def _band_limited(g, shape, amp):
    """Noise at 1/16 resolution, bicubically upsampled: [M, N, H, W] (test_post_process_routes._band_limited)."""
    M, N, H, W = shape
    low = torch.randn(M, N, max(2, -(-H // 16) + 1), max(2, -(-W // 16) + 1), generator=g, dtype=torch.float64)
    return amp * F.interpolate(low, size=(H, W), mode="bicubic", align_corners=True)


def _edge_gate(W):
    """1 on the outer tenth of the row on each side, falling smoothly to 0 at 0.15 W from the border: [1,1,1,W]."""
    x = torch.arange(W, dtype=torch.float64)
    t = torch.minimum(x, W - 1 - x) / max(W - 1, 1)
    u = ((0.15 - t) / 0.05).clamp(0.0, 1.0)
    return (u * u * (3.0 - 2.0 * u)).view(1, 1, 1, W)


def _border_window(W):
    """1 in the interior, falling over 16 columns to min(1, 64 / W) at the left and right border
    (test_post_process_routes._border_window): zero padding makes a step of the border logit's size at the edge of view, which
    the fp32 coordinate chain (~W * 6e-8 px) turns into an error of the oracle's own fp32 run in proportion."""
    x = torch.arange(W, dtype=torch.float64)
    edge = min(1.0, 64.0 / W)
    return (edge + (1.0 - edge) * (torch.minimum(x, W - 1 - x) / 16.0).clamp(max=1.0)).view(1, 1, 1, W)


def _specials(N):
    """Which plane carries which special disparity: (last_column, even_integer, zero, low_probability); None = the case has none."""
    if N >= 5:
        return 0, 1, N - 1, N // 2
    if N >= 2:
        return None, 0, N - 1, None
    return None, None, None, None


@functools.lru_cache(maxsize=None)
def inputs(name, far=False):
    """fp64 CPU tensors of a case, every value representable in what the operator reads (fp32; bf16 for the conv outputs of a bf16
    case), so that every precision sees the same inputs: rl, rs [B,N,H,W] (raw, or as a tail wrote them under ``applied``), image
    [B,3,H,W], lv [B,N], drows / mrows [B,N,H] (None without the row form / a mask), dl / pm [B,N,H,W] (the dense maps the oracle
    reads).  ``far``: the d = 0 plane gets the spacing's own value (the far baselines)."""
    c = BY_NAME[name]
    B, N, H, W = c.shape
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()) % (1 << 31) + 7919 * c.draw)
    band = _band_limited(g, c.shape, 1.0)
    n = torch.arange(N, dtype=torch.float64).view(1, N, 1, 1)
    if c.order == "rand":
        rl = 2.5 * band
    elif c.order in ("inc", "dec"):
        rl = (1.5 * (n - (N - 1)) if c.order == "inc" else -1.5 * n) + 0.2 * torch.tanh(band)
    else:
        rl = band + torch.where((n == 1) | (n == 3), 40.0, -40.0)
    rl = (rl - 7.0 * _edge_gate(W)) * _border_window(W)
    last_col, even_int, zero, low = _specials(N)
    if low is not None and c.order == "rand":
        rl[:, low] -= 8.0
    q = _band_limited(g, c.shape, 1.0)
    xs = torch.arange(W, dtype=torch.float64).view(1, 1, 1, W) / W
    ys = torch.arange(H, dtype=torch.float64).view(1, 1, H, 1) / (2 * H)
    q = 0.5 * q + 1.6 * torch.sin(2.0 * math.pi * (xs + ys + n / 3.0))     # every plane has both signs, as regions
    rs = 3.0 * _band_limited(g, c.shape, 1.0) - 1.0 + 40.0 * torch.relu(q - 0.7) - 16.0 * torch.relu(-q - 0.7)
    image = (0.5 + 0.4 * torch.tanh(_band_limited(g, (B, 3, H, W), 1.0))).float().double()
    # disparities as the decoders space them, decreasing with the plane index, up to 0.47 W
    lv = n[..., 0, 0] + 0.5 * (torch.rand(B, N, generator=g, dtype=torch.float64) - 0.5)
    lv = 0.47 * W * (2.0 / 300.0) ** (lv.clamp_min(0.0) / max(N - 1, 1))
    if N == 1:
        lv[:] = math.floor(0.3 * W) + 0.97
    if even_int is not None:
        lv[:, even_int] = (2.0 * torch.round(lv[:, even_int] / 2.0)).clamp(2.0, max(2.0, 2.0 * ((W - 2) // 2)))
    if last_col is not None:
        lv[:, last_col] = float(W - 1)
    if zero is not None and not far:
        lv[:, zero] = 0.0
    lv = lv.float().double()
    drows = mrows = None
    if c.form != "plane":
        row_gain = 1.0 - c.gain * torch.rand(B, 1, H, generator=g, dtype=torch.float64).expand(B, N, H).clone()
        for p in (last_col, even_int):
            if p is not None:
                row_gain[:, p] = 1.0     # (these keep their exact values on every row)
        drows = (lv[:, :, None] * row_gain).float().double()
        dl = drows[..., None].expand(B, N, H, W).clone()
    else:
        dl = lv[:, :, None, None].expand(B, N, H, W).clone()
    if c.mask == "rows":
        mrows = (torch.rand(B, N, H, generator=g, dtype=torch.float64) > 0.2).double()
        mrows[:, 0] = 1.0
        pm = mrows[..., None].expand(B, N, H, W).clone()
    else:
        pm = torch.ones(B, N, H, W, dtype=torch.float64)
    if c.applied:
        rl, rs = rl * pm, torch.clamp(torch.sigmoid(rs), 0.01, 1.0)
    store = (lambda t: t.to(BF).double()) if c.bf16 else (lambda t: t.float().double())
    return dict(rl=store(rl), rs=store(rs), image=image, lv=lv, drows=drows, mrows=mrows, dl=dl, pm=pm)


def _oracle_views(c, z, views, dtype):
    """[(rgb [B,3,H,W], coverage [B,1,H,W], disp [B,1,H,W]) per view]: test_render_views._oracle's composition in ``dtype``."""
    W = c.shape[3]
    rl, rs, pm, dl, image = (z[k].to(dtype) for k in ("rl", "rs", "pm", "dl", "image"))
    if c.applied:
        logits, sigma = rl, rs
    else:
        tail = orc.decoder_tail(rl, rs, pm, dl, W, c.mix)
        logits, sigma = tail["logits"], tail.get("sigma")
    mask, ones_img, res = pm[:, :, None], torch.ones_like(image), []
    for s in views:
        grid = orc.disp_grid(torch.tensor(s, dtype=torch.float32).to(dtype) * dl, "r")
        out = orc.plane_sweep(image, logits, sigma, grid, mask, use_mixture_loss=c.mix)
        ones = orc.plane_sweep(ones_img, logits, sigma, grid, mask, use_mixture_loss=c.mix)
        res.append((out["rgb_rec"], ones["rgb_rec"][:, :1], (out["probability_rec"] * dl).sum(1, True)))
    return res


@functools.lru_cache(maxsize=None)
def reference(name, dtype, far=False):
    """The views of a case in ``dtype``: computed once per process, shared by every test; nobody writes into it."""
    c = BY_NAME[name]
    return _oracle_views(c, inputs(name, far), FAR if far else c.views, dtype)


def e_ref(name, v, k, floor=FLOOR, far=False):
    return px_report(reference(name, torch.float32, far)[v][k], reference(name, torch.float64, far)[v][k], floor)["err"]


def bar(e0):
    return FACTOR * e0 + TOL


def weak_share(cov64):
    return float(((cov64 > 0) & (cov64 < WEAK_BELOW)).double().mean())


# =====================================================================================================================
# CPU: the table against the query, its coverage, the boundaries, the inputs' conditions
# =====================================================================================================================
def _by_hand(W, V):
    return 2 if (W > 1024 or (W >= 513 and V <= 2)) else 1


@pytest.mark.parametrize("name", IDS)
def test_table_matches_the_query(name):
    c = BY_NAME[name]
    B, N, H, W = c.shape
    for V in launches(c):
        assert ops.render_cols_per_lane(W, V) == c.cpl == _by_hand(W, V), (name, V)
    assert B in (1, 2) and B * N * H * W * len(c.views) <= 4 * 9 * 14 * 2048
    assert c.form == "plane" or (B == 2 and c.mask == "rows")


def test_every_instantiation_is_in_the_table():
    reached = {(c.bf16, c.mix, V, c.cpl) for c in CASES for V in launches(c)}
    every = {(bf, mix, V, cpl) for bf in (False, True) for mix in (False, True) for V in (1, 2, 3, 4) for cpl in (1, 2)}
    assert len(every) == 32 and reached == every
    # widths: one wave, a second partial wave, 130; one column per lane at W >= 513 (V = 3, 4); two columns with lanes that own no
    # second column (514), full (1024, 2048) and partial at V = 3, 4 (1026)
    one = {c.shape[3] for c in CASES if c.cpl == 1}
    assert {2, 64, 66, 130} <= one and one & {514, 1024}
    assert {c.shape[3] for c in CASES if c.cpl == 2 and len(c.views) <= 2} == {514, 1024}
    assert {c.shape[3] for c in CASES if c.cpl == 2 and len(c.views) >= 3} == {1026, 2048}
    assert {c.shape[2] for c in CASES} == {2, 7, 14} and sum(c.shape[2] == 7 for c in CASES) == sum(c.shape[2] == 2 for c in CASES) == 1
    assert {1, 2, 9, 49, 63, 65} <= {c.shape[1] for c in CASES}
    assert {c.bf16 for c in CASES if c.shape[1] == 65} == {False, True}
    for bf in (False, True):      # row-view disparities and masks with B = 2 per dtype x mix; a batch slice; the orders; the lists
        for mix in (False, True):
            assert any(c.form != "plane" and c.mask == "rows" and c.shape[0] == 2 for c in CASES if (c.bf16, c.mix) == (bf, mix))
            assert any(c.applied for c in CASES if (c.bf16, c.mix) == (bf, mix))
    assert any(c.form == "rows_slice" for c in CASES)
    assert {c.order for c in CASES} == {"rand", "inc", "dec", "spread"}
    assert {c.views for c in CASES} == {V1, V1L, V2, V3, V4, V5, V9}
    assert [launches(BY_NAME[n]) for n in ("chunk5_w64", "chunk9_w66")] == [[4, 1], [4, 4, 1]]
    assert all(BY_NAME[n].shape[0] == 2 and BY_NAME[n].mask == "rows" for n in ("chunk5_w64", "chunk9_w66"))


def test_query_at_the_boundaries():
    q = ops.render_cols_per_lane
    assert [q(512, V) for V in (1, 2, 3, 4)] == [1, 1, 1, 1]
    assert [q(513, V) for V in (1, 2, 3, 4)] == [2, 2, 1, 1]
    assert [q(1024, V) for V in (1, 2, 3, 4)] == [2, 2, 1, 1]
    assert [q(1025, V) for V in (1, 2, 3, 4)] == [2, 2, 2, 2]
    assert [q(2048, V) for V in (1, 2, 3, 4)] == [2, 2, 2, 2]
    assert [q(2049, V) for V in (1, 2, 3, 4)] == [0, 0, 0, 0]
    assert q(2, 1) == 1 and q(1, 1) == 0 and q(640, 0) == 0 and q(640, 5) == 0
    for W in range(2, 2050):
        for V in (1, 2, 3, 4):
            assert q(W, V) == (_by_hand(W, V) if W <= 2048 else 0), (W, V)


def test_floor_is_the_smallest_that_holds():
    holds = {f: all(e_ref(c.name, v, k, f) <= E_REF_MAX for c in CASES for v in range(len(c.views)) for k in range(3))
             for f in (1e-3, 1e-2, 1e-1)}
    print("E_ref <= %g for the whole table at FLOOR:" % E_REF_MAX, holds)
    assert holds[FLOOR] and FLOOR == min(f for f, ok in holds.items() if ok)


@pytest.mark.parametrize("name", IDS)
def test_conditions_cpu(name):
    c = BY_NAME[name]
    B, N, H, W = c.shape
    z = inputs(name)
    r64 = reference(name, torch.float64)
    rep = REPORT.setdefault(name, {"cols_per_lane": c.cpl, "views": {}})
    weak = strong = 0.0
    for v, s in enumerate(c.views):
        vr = rep["views"].setdefault("%g" % s, {})
        for k, key in enumerate(OUTPUTS):
            assert bool(torch.isfinite(r64[v][k]).all())
            e = e_ref(name, v, k)
            vr["E_ref/" + key] = e
            print("%s s = %+g E_ref %s: %.3e" % (name, s, key, e))
            assert e <= E_REF_MAX, (name, s, key, e)
        cov = r64[v][1]
        vr["weak_share"] = round(weak_share(cov), 4)
        vr["zero_pixels"] = int((cov == 0).sum())
        weak += weak_share(cov) / len(c.views)
        strong += float((cov > STRONG_ABOVE).double().mean()) / len(c.views)
        assert float(cov.min()) >= 0.0 and float(cov.max()) <= 1.0 + 1e-12
    print("%s: share of pixels with 0 < coverage < %g: %.4f, with coverage > %g: %.4f" % (name, WEAK_BELOW, weak, STRONG_ABOVE, strong))
    assert weak >= WEAK_SHARE, (name, weak)
    assert strong >= STRONG_SHARE, (name, strong)
    # the inputs are what the docstring says
    lv, rl, rs = z["lv"], z["rl"], z["rs"]
    last_col, even_int, zero, low = _specials(N)
    if last_col is not None:
        assert bool((lv[:, last_col] == W - 1).all())
    if even_int is not None:
        assert bool(((lv[:, even_int] % 2 == 0) & (lv[:, even_int] >= 2) & (lv[:, even_int] <= W - 1)).all())
    if zero is not None:
        assert bool((lv[:, zero] == 0).all()) and bool((inputs(name, True)["lv"][:, zero] > 0).all())
    if N == 1:
        assert abs(float(lv[0, 0]) % 1 - 0.97) < 1e-5
    others = [i for i in range(N) if i not in (last_col, even_int)]
    if others and N > 1:
        assert float(lv[:, others].max()) <= 0.47 * W * 1.0001
    if low is not None and c.order == "rand" and not c.applied and c.mask == "none":
        p = torch.softmax(rl, 1)[:, low]
        assert float(p.median()) < 1e-3, float(p.median())
    if c.order in ("inc", "dec"):
        d = rl[:, 1:] - rl[:, :-1]
        assert bool((d > 0).all()) if c.order == "inc" else bool((d < 0).all())
    if c.order == "spread":
        assert float((rl.amax(1) - rl.amin(1))[..., 16:-16].min()) > 70.0     # (inside the border window)
    if H * W >= 14 * 64 and c.mix:     # both ends of sigma's clamp, as regions: a share of the elements, not single ones
        lo, hi = (rs <= -12.0, rs >= 30.0) if not c.applied else (rs <= 0.0101, rs == 1.0)
        assert float(lo.double().mean()) >= 0.01 and float(hi.double().mean()) >= 0.01, (float(lo.double().mean()), float(hi.double().mean()))
    if c.form != "plane":
        assert bool((z["drows"][:, others][..., 0] != z["drows"][:, others][..., -1]).any())
        assert 0.05 <= float((z["mrows"] == 0).double().mean()) <= 0.3
    if c.bf16:
        assert torch.equal(rl.to(BF).double(), rl) and torch.equal(rs.to(BF).double(), rs)
    else:
        assert torch.equal(rl.float().double(), rl) and torch.equal(rs.float().double(), rs)


@pytest.mark.parametrize("name", FAR_CASES)
def test_far_reference_cpu(name):
    """The far baselines' fp64 reference: nothing in view for +-1e6 and 3e38 — coverage = rgb = 0, disp the mean of the planes'
    disparities with the mixture (every plane: logit 0, sigma 0.01) and without; 1e-30 is the source camera."""
    c = BY_NAME[name]
    z = inputs(name, True)
    r64 = reference(name, torch.float64, True)
    for v in range(3):
        rgb, cov, disp = r64[v]
        assert not bool(rgb.any()) and not bool(cov.any())
        assert float((disp - z["dl"].mean(1, keepdim=True)).abs().max()) <= 1e-12 * float(z["dl"].max())
    near = _oracle_views(c, z, (0.0,), torch.float64)[0]
    for a, b in zip(r64[3], near):
        assert float((a - b).abs().max()) <= 1e-12
    assert float(r64[3][1].max()) > 0.5
    for k in range(3):
        assert e_ref(name, 3, k, far=True) <= E_REF_MAX


# =====================================================================================================================
# GPU
# =====================================================================================================================
@pytest.fixture(scope="module", autouse=True)
def _parity_report():
    yield
    path = os.environ.get("PD_RENDER_PARITY_JSON")
    if path and REPORT:
        with open(path, "w") as f:
            json.dump(REPORT, f, indent=1, sort_keys=True)


def _operands(name, far=False):
    """Device tensors of a case as ``ops.render_views`` takes them: (rl, rs | None, pm | None, dl, image)."""
    c, z = BY_NAME[name], inputs(name, far)
    B, N, H, W = c.shape
    st = BF if c.bf16 else torch.float32
    rl = z["rl"].to(st).to(DEV)
    rs = z["rs"].to(st).to(DEV) if c.mix else None
    image = z["image"].float().to(DEV)

    def rows(t):
        t = t.float().to(DEV)
        if c.form == "rows_slice":       # the case's rows are the first B images of a larger row view
            return ops.row_view(torch.cat([t, t[:1] * 0.5], 0).contiguous(), W)[:B]
        return ops.row_view(t.contiguous(), W)
    dl = rows(z["drows"]) if c.form != "plane" else z["lv"].float().to(DEV).view(B, N, 1, 1).expand(B, N, H, W)
    pm = rows(z["mrows"]) if c.mask == "rows" else None
    return rl, rs, pm, dl, image


def _render(c, operands, views):
    rl, rs, pm, dl, image = operands
    with torch.no_grad():
        return ops.render_views(rl, rs, pm, dl, image, views, use_mixture_loss=c.mix, tail_applied=c.applied)


@gpu
@pytest.mark.parametrize("name", IDS)
def test_render_views_per_pixel(name):
    c = BY_NAME[name]
    B, N, H, W = c.shape
    r64 = reference(name, torch.float64)
    for V in launches(c):
        assert ops.render_cols_per_lane(W, V) == c.cpl
    res = _render(c, _operands(name), c.views)
    assert res.rgb.shape == (B, len(c.views), 3, H, W) and res.coverage.shape == res.disp.shape == (B, len(c.views), 1, H, W)
    rep = REPORT.setdefault(name, {"cols_per_lane": c.cpl, "views": {}})
    failures = []
    for v, s in enumerate(c.views):
        vr = rep["views"].setdefault("%g" % s, {})
        for k, key in enumerate(OUTPUTS):
            got = res[k][:, v]
            r = px_report(got, r64[v][k], FLOOR)
            e0 = e_ref(name, v, k)
            vr["E_ref/" + key], vr["product/" + key] = e0, r["err"]
            vr["weak_share"], vr["zero_pixels"] = round(weak_share(r64[v][1]), 4), int((r64[v][1] == 0).sum())
            print("%s s = %+g %s: product %.3e  E_ref %.3e  bar %.3e  zero pixels %d (|got| <= %.1e)"
                  % (name, s, key, r["err"], e0, bar(e0), r["zeros"], r["zero_abs"]))
            if not (bool(torch.isfinite(got).all()) and r["zero_ok"] and r["err"] <= bar(e0)):
                failures.append((s, key, r["err"], e0, bar(e0), r["zero_abs"], r["worst"]))
    assert not failures, failures


@gpu
@pytest.mark.parametrize("name", FAR_CASES)
def test_far_baselines(name):
    c = BY_NAME[name]
    r64 = reference(name, torch.float64, True)
    res = _render(c, _operands(name, True), FAR)
    rep = REPORT.setdefault(name, {"cols_per_lane": c.cpl, "views": {}})
    failures = []
    for v, s in enumerate(FAR):
        for t in res:
            assert bool(torch.isfinite(t[:, v]).all()), (s, "not finite")
        if v < 3:    # nothing in view: exact zeros; disp against fp64 with the bar's 1e-4 alone (3e38 * d: the fp32 oracle is NaN)
            assert not bool(res.rgb[:, v].any()) and not bool(res.coverage[:, v].any()), s
            allow = {2: TOL}
        else:
            allow = {k: bar(e_ref(name, v, k, far=True)) for k in range(3)}
        vr = rep["views"].setdefault("far %g" % s, {})
        for k, a in allow.items():
            r = px_report(res[k][:, v], r64[v][k], FLOOR)
            vr["product/" + OUTPUTS[k]] = r["err"]
            print("%s far s = %g %s: product %.3e  allowed %.3e" % (name, s, OUTPUTS[k], r["err"], a))
            if not (r["zero_ok"] and r["err"] <= a):
                failures.append((s, OUTPUTS[k], r["err"], a, r["worst"]))
    assert not failures, failures


def _same_bits(a, b, what):
    for x, y, key in zip(a, b, OUTPUTS):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), (what, key)


@gpu
@pytest.mark.parametrize("name", LAYOUT_CASES)
def test_layouts_bit_for_bit(name):
    """The layouts a model hands over, against the plain contiguous call: the same bits."""
    c = BY_NAME[name]
    B, N, H, W = c.shape
    rl, rs, pm, dl, image = _operands(name)
    plain = _render(c, (rl, rs, pm, dl, image), c.views)
    cl = lambda t: None if t is None else t.contiguous(memory_format=torch.channels_last)   # noqa: E731
    assert not cl(rl).is_contiguous()
    _same_bits(_render(c, (cl(rl), cl(rs), pm, dl, image), c.views), plain, "channels_last conv outputs")
    # logits and sigma as the two channel halves of one conv output: non-contiguous over the batch, sigma at a storage offset
    conv = torch.cat([rl, rs if rs is not None else rl.flip(1)], 1).contiguous()
    lo, hi = conv[:, :N], conv[:, N:]
    assert not lo.is_contiguous() and hi.storage_offset() == N * H * W
    _same_bits(_render(c, (lo, hi if c.mix else None, pm, dl, image), c.views), plain, "channel halves")
    conv_cl = cl(conv)
    _same_bits(_render(c, (conv_cl[:, :N], conv_cl[:, N:] if c.mix else None, pm, dl, image), c.views), plain, "channels_last halves")
    if c.bf16:   # a bf16 conv output at 2 (mod 4)
        def odd(t):
            buf = torch.empty(t.numel() + 1, dtype=BF, device=DEV)
            o = buf[1:].view(t.shape)
            o.copy_(t)
            assert o.data_ptr() % 4 == 2 and o.is_contiguous()
            return o
        _same_bits(_render(c, (odd(rl), None if rs is None else odd(rs), pm, dl, image), c.views), plain, "bf16 at 2 mod 4")
    assert not cl(image).is_contiguous()
    _same_bits(_render(c, (rl, rs, pm, dl, cl(image)), c.views), plain, "channels_last image")
    wide = torch.cat([image, 1.0 - image], 3)
    crop = wide[..., :W]
    assert not crop.is_contiguous()
    _same_bits(_render(c, (rl, rs, pm, dl, crop), c.views), plain, "image: a width crop")
    _same_bits(_render(c, (cl(rl), cl(rs), pm, dl, cl(wide)[..., :W]), c.views), plain, "all of them at once")


@gpu
@pytest.mark.parametrize("mix", [True, False], ids=["mix", "pi"])
@pytest.mark.parametrize("autocast", [False, True], ids=["fp32", "autocast"])
def test_predict_render_channels_last(mix, autocast):
    """predict.render on a channels_last model and channels_last images: the views are, bit for bit, ``ops.render_views`` on
    contiguous copies of what that forward pass kept."""
    import planedepth_amd
    from test_render_views import _Net
    M, H, W = 2, 16, 48
    g = torch.Generator().manual_seed(11)
    images = torch.rand(M, 3, H, W, generator=g).to(DEV)
    baselines = (1.0, -0.5, 0.25)
    net = _Net("keep", mix).to(DEV).to(memory_format=torch.channels_last).eval()
    views, _ = planedepth_amd.predict.render(net, images.contiguous(memory_format=torch.channels_last), baselines, autocast=autocast)
    out = net.outputs
    assert out["raw_logits"].dtype == (BF if autocast else torch.float32)
    with torch.no_grad():
        direct = ops.render_views(out["raw_logits"].contiguous(), out["raw_sigma"].contiguous() if mix else None, out["padding_mask"],
                                  out["disp_layered"], images, baselines, use_mixture_loss=mix)
    _same_bits(views, direct, "predict.render, channels_last")
