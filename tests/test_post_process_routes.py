"""Post-process (trainer.py:421-466): every kernel route of pd_warp_softmax, pd_warp_sum and pd_post_process, per pixel
against the oracle in fp64.

One table (``CASES``) of small shapes.  Each row states, written down by hand from the dispatch conditions, the route the fused
call and the two standalone warps take; ``ops.post_process_route`` / ``ops.warp_route`` — the functions the entry points
themselves switch on — must agree, on the CPU.  ``test_every_reachable_instantiation_is_in_the_table`` walks every (N, W, form)
through the query and proves that the table holds each kernel instantiation a shape can reach at 160 KiB of LDS, and states why
the remaining ones cannot be reached.

Inputs: band-limited logits and sigma (noise at 1/16 resolution, bicubic), because white-noise logits turn the fp32 coordinate
chain's ~W * 6e-8 px into an oracle-fp32 error of up to 1e-4, which would be the bar; an integer disparity, a zero one and one
that lands on column W - 1 per image; shifts up to 300 px; per-row disparities on the last third of the planes under
PD_PP_DISP_ROWS; and a few planes out of view for the image only / for the mirrored image only, which keep the three plane sums
under the clamp ``min(1, .)`` on most pixels — the clamp hides every error where the sum exceeds 1.  ``test_conditions_cpu``
asserts from the references alone that at most 0.30 (and at least 0.02) of the pixels of o_l, o_fr and mask_novel are clamped
and that E_ref <= 1e-4.

The bar (GPU):  err(got, fp64) <= 2 * E_ref + N * 2^-23.
  E_ref   the oracle's own fp32 run against its fp64 run, the largest per-pixel error of that output;
  2       ``cases.three_way``'s factor;
  N 2^-23 two chained N-term fp32 sums of values <= 1 in any order: what the chains' reassociation may cost.
err is the largest per-pixel |got - ref| for the [B,1,H,W] outputs, in units of max(1, max|ref|) (the blend multiplies a mask
error by up to max|disp|; the indicator and ramp fills have scale 1: absolute), and ``slice_report(..., plane_floor=1e-2)["err"]``
(row-scaled) for warp_softmax.  disp_pp is held to it under three disparity fills: the realistic sum(prob * disp_layered); the
indicator disp[:B] = 1, disp[B:] = 0, which makes disp_pp = o_l (1 - o_fr / 2): the masks at full scale; and disp[:B] = 0 with
disp[B:] a ramp distinct in x, y and image, which pins the mirrored read.

Heights: with align_corners=True the reference's row coordinate is y up to one fp32 rounding, and a target row blends two source
rows (NR = 2; under PD_PP_DISP_ROWS also the S maps of the neighbouring rows) only where that round trip is inexact.  H = 14 is
the smallest height with rows rounded both down (1, 2, 3) and up (7): ``test_heights_cover_one_and_two_row_targets``.  The second
row's weight is one ulp (~1e-7): its ARITHMETIC cannot be seen against fp64 at any bar.  What can be seen is whether it reads
only memory that was written: ``test_guards_*`` runs one case per kernel family through the C ABI with the NaN pattern behind
every input, in every output element and in the whole workspace — a read of an unwritten S map or past a plane's end is a NaN
in the output, and the result must equal, bit for bit, the same call on zero-filled buffers.

PD_POST_PROCESS_PARITY_JSON=<file> writes route, E_ref, the product's error and the clamped shares per case: the source of
profiles/post_process_parity.md."""
import ctypes
import functools
import json
import math
import os

import pytest
import torch
import torch.nn.functional as F

from cases import slice_report
from oracle import planedepth_oracle as orc
from planedepth_amd import _capi as C
from planedepth_amd import ops

gpu = pytest.mark.gpu
DEV = "cuda"
LDS = 160 * 1024
EPS = 2.0 ** -23
SHARE_MIN, SHARE_MAX, E_REF_MAX = 0.02, 0.30, 1e-4
CHAIN_VS_STEPWISE = 3e-6      # fused chains against the single warps: fp32 reassociation (the vertical weights leave the plane sum)
REPORT = {}
LOGIT_AMP = 2.0

FLAG = {"plane": 0, "rows": C.PD_PP_DISP_ROWS, "dense": C.PD_PP_DISP_DENSE}
SPLIT, CHAIN, SINGLE = "chain_split", "chain", "single"


class Case:
    """name, B (half the doubled batch), N, H, W, form (plane | rows | dense), the fused route (family, nmax, rows2, alias, LDS
    bytes), the route of warp_softmax (family, nmax) and of warp_sum (family) on an 8-byte aligned output, ``ws4``: the fused
    call gets a workspace that is 4-byte aligned only."""

    def __init__(self, name, B, N, H, W, form, fused, softmax, wsum, ws4=False):
        self.name, self.B, self.N, self.H, self.W, self.form = name, B, N, H, W, form
        self.fused, self.softmax, self.wsum, self.ws4 = fused, softmax, wsum, ws4

    def __repr__(self):
        return self.name


def _lds(N, W, nseg=None):
    """Row buffer N x (W + 4) floats; with nseg: plus one float2 per pixel of the padded row and part (3 parts)."""
    return N * (W + 4) * 4 + (0 if nseg is None else 3 * nseg * 128 * 8)


# The conditions (pd_postprocess.hip, post_process_route / warp_route), by hand:
#   chains      not dense, W even, W <= 1024, N <= 64, N (W + 4) 4 <= LDS, workspace and disp_pp 8-byte aligned
#   split       W <= 640 (3 nseg <= 16 waves, nseg = ceil(W / 128)); NPART 11 (N <= 33), 18 (N <= 54), 22; alias iff
#               N (W + 4) 4 + 3 nseg 1024 > LDS, its LDS then the row buffer alone
#   chain       W >= 642; NMAX 32 (N <= 32), 52 (N <= 52), 64
#   warp seg    not dense, W even, out 8-byte aligned, softmax: N <= 64 with NMAX 32 / 52 / 64; else rows; dense: gather
CASES = [
    # name                B   N   H    W   form     fused (family, nmax, rows2, alias, lds)              softmax        sum
    Case("n1_w2_h2",      2,  1,  2,    2, "plane", (SPLIT, 11, False, False, _lds(1, 2, 1)),            ("seg", 32),   "seg"),
    Case("n11_w128",      2, 11, 14,  128, "rows",  (SPLIT, 11, True, False, _lds(11, 128, 1)),          ("seg", 32),   "seg"),   # parts 1, 2 empty
    Case("n12_w130",      1, 12, 14,  130, "plane", (SPLIT, 11, False, False, _lds(12, 130, 2)),         ("seg", 32),   "seg"),
    Case("n33_w256",      1, 33, 14,  256, "rows",  (SPLIT, 11, True, False, _lds(33, 256, 2)),          ("seg", 52),   "seg"),
    Case("n34_w258",      1, 34, 14,  258, "plane", (SPLIT, 18, False, False, _lds(34, 258, 3)),         ("seg", 52),   "seg"),   # part 2 empty
    Case("n36_w256_h7",   1, 36,  7,  256, "rows",  (SPLIT, 18, True, False, _lds(36, 256, 2)),          ("seg", 52),   "seg"),   # part 2 empty
    Case("n54_w578",      1, 54, 14,  578, "plane", (SPLIT, 18, False, False, _lds(54, 578, 5)),         ("seg", 64),   "seg"),
    Case("n55_w130",      1, 55, 14,  130, "rows",  (SPLIT, 22, True, False, _lds(55, 130, 2)),          ("seg", 64),   "seg"),
    Case("n57_w640",      1, 57, 14,  640, "plane", (SPLIT, 22, False, False, _lds(57, 640, 5)),         ("seg", 64),   "seg"),   # 162192 <= LDS
    Case("n58_w640",      1, 58, 14,  640, "plane", (SPLIT, 22, False, True, _lds(58, 640)),             ("seg", 64),   "seg"),   # 164768 > LDS
    Case("n63_w640_rows", 1, 63, 14,  640, "rows",  (SPLIT, 22, True, True, _lds(63, 640)),              ("seg", 64),   "seg"),   # the reference's 63 planes
    Case("n64_w640",      1, 64, 14,  640, "plane", (SINGLE, 0, False, False, 0),                        ("seg", 64),   "seg"),   # row buffer 164864 > LDS
    Case("n64_w576",      1, 64, 14,  576, "plane", (SPLIT, 22, False, False, LDS),                      ("seg", 64),   "seg"),   # exact fit: 163840
    Case("n64_w578",      1, 64, 14,  578, "rows",  (SPLIT, 22, True, True, _lds(64, 578)),              ("seg", 64),   "seg"),
    Case("n64_w130",      2, 64, 14,  130, "plane", (SPLIT, 22, False, False, _lds(64, 130, 2)),         ("seg", 64),   "seg"),
    Case("n65_w130",      1, 65, 14,  130, "plane", (SINGLE, 0, False, False, 0),                        ("rows", 0),   "seg"),
    Case("n32_w642",      1, 32, 14,  642, "plane", (CHAIN, 32, False, False, _lds(32, 642)),            ("seg", 32),   "seg"),
    Case("n32_w1024",     1, 32, 14, 1024, "rows",  (CHAIN, 32, True, False, _lds(32, 1024)),            ("seg", 32),   "seg"),
    Case("n33_w642",      1, 33, 14,  642, "plane", (CHAIN, 52, False, False, _lds(33, 642)),            ("seg", 52),   "seg"),
    Case("n52_w770",      1, 52, 14,  770, "rows",  (CHAIN, 52, True, False, _lds(52, 770)),             ("seg", 52),   "seg"),
    Case("n53_w642",      1, 53, 14,  642, "plane", (CHAIN, 64, False, False, _lds(53, 642)),            ("seg", 64),   "seg"),
    Case("n63_w642",      1, 63, 14,  642, "rows",  (CHAIN, 64, True, False, _lds(63, 642)),             ("seg", 64),   "seg"),
    Case("n33_w1026",     1, 33, 14, 1026, "plane", (SINGLE, 0, False, False, 0),                        ("seg", 52),   "seg"),
    Case("n5_w63",        2,  5, 14,   63, "plane", (SINGLE, 0, False, False, 0),                        ("rows", 0),   "rows"),
    Case("n9_w129",       1,  9, 14,  129, "rows",  (SINGLE, 0, False, False, 0),                        ("rows", 0),   "rows"),
    Case("n12_w128_dense", 1, 12, 14, 128, "dense", (SINGLE, 0, False, False, 0),                        ("gather", 0), "gather"),
    Case("n12_w128_ws4",  1, 12, 14,  128, "plane", (SINGLE, 0, False, False, 0),                        ("seg", 32),   "seg", ws4=True),
]
BY_NAME = {c.name: c for c in CASES}
IDS = [c.name for c in CASES]


# =====================================================================================================================
# Inputs and references
# =====================================================================================================================
def _band_limited(g, shape, amp):
    """Noise at 1/16 resolution, bicubically upsampled: [M, N, H, W]."""
    M, N, H, W = shape
    low = torch.randn(M, N, max(2, -(-H // 16) + 1), max(2, -(-W // 16) + 1), generator=g, dtype=torch.float64)
    return amp * F.interpolate(low, size=(H, W), mode="bicubic", align_corners=True)


def _border_window(W):
    """1 in the interior, falling over 16 columns to min(1, 64 / W) at the left and right border.  Zero padding makes a step
    of the border logit's size at the edge of view, which the fp32 coordinate chain (~W * 6e-8 px) turns into an error of the
    oracle's own fp32 run in proportion: without this E_ref of warp_softmax is 1.0e-4 .. 1.9e-4 from W = 578 on.  The border
    logits stay far above the bar (|l| ~ 0.3 at W = 640: a dropped border tap moves a probability by a quarter)."""
    x = torch.arange(W, dtype=torch.float64)
    edge = min(1.0, 64.0 / W)
    return (edge + (1.0 - edge) * (torch.minimum(x, W - 1 - x) / 16.0).clamp(max=1.0)).view(1, 1, 1, W)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """fp64 tensors of a case: logits, prob [2B,N,H,W], dl [2B,N,H,W] (the dense disparity map: what the oracle reads),
    lv [2B,N] / rows [2B,N,H] (its compact forms).  Values are fp32-representable, so every precision sees the same inputs."""
    c = BY_NAME[name]
    B, N, H, W = c.B, c.N, c.H, c.W
    g = torch.Generator().manual_seed(7000 + 131 * N + W + H)
    logits = (_band_limited(g, (2 * B, N, H, W), LOGIT_AMP) * _border_window(W)).float().double()
    sigma = torch.sigmoid(_band_limited(g, (2 * B, N, H, W), 1.0)) * 0.9 + 0.05
    w = torch.softmax(logits, 1) / sigma
    prob = (w / w.sum(1, True)).float().double()
    dmax = min(300.0, 0.75 * (W - 1))
    lv = torch.rand(2 * B, N, generator=g, dtype=torch.float64) * dmax
    order = torch.randperm(N, generator=g).tolist()     # which plane gets which special disparity
    special = [("integer", None), ("zero", 0.0), ("last_column", float(W - 1))]
    n_out = N // 8
    for k, n in enumerate(order):
        if N == 1:   # softmax = 1 wherever the plane is: the sums reach 1 at every pixel whose two taps are in view
            lv[:, n] = 0.5 + (torch.arange(2 * B, dtype=torch.float64) % B)     # W = 2: one pixel of four
        elif k == 0:
            lv[:, n] = torch.round(lv[:, n]).clamp(1.0, W - 2.0)
        elif k < 3 and N >= 5:
            lv[:, n] = special[k][1]
        elif k < 3 + n_out:
            lv[:B, n] = float(W + 5)                    # out of view for the image only
        elif k < 3 + 2 * n_out:
            lv[B:, n] = float(W + 5)                    # out of view for the mirrored image only
    lv = lv.float().double()
    rows = lv[:, :, None].expand(-1, -1, H).clone()
    if c.form in ("rows", "dense"):
        third = N - N // 3
        gain = torch.linspace(0.7, 1.3, H, dtype=torch.float64).view(1, 1, H) * (0.8 + 0.4 * torch.rand(2 * B, N - third, 1, generator=g, dtype=torch.float64))
        live = rows[:, third:] < W                       # (the out-of-view planes stay out of view)
        rows[:, third:] = torch.where(live, rows[:, third:] * gain, rows[:, third:])
    rows = rows.float().double()
    dl = rows[..., None].expand(-1, -1, -1, W).clone()
    if c.form == "dense":                                # a true per-pixel map: a gentle slope along x
        dl = (dl * (1.0 + 0.05 * torch.linspace(-1, 1, W, dtype=torch.float64).view(1, 1, 1, W))).float().double()
    return dict(logits=logits, prob=prob, lv=lv, rows=rows, dl=dl)


FILLS = ("real", "indicator", "ramp")


def disp_fill(name, fill):
    c, z = BY_NAME[name], inputs(name)
    B, H, W = c.B, c.H, c.W
    if fill == "real":
        return (z["prob"] * z["dl"]).sum(1, True).float().double()
    d = torch.zeros(2 * B, 1, H, W, dtype=torch.float64)
    if fill == "indicator":
        d[:B] = 1.0
    else:
        d[B:] = ((torch.arange(B * H * W, dtype=torch.float64) + 1.0) / (B * H * W)).view(B, 1, H, W).float().double()
    return d


def _warp(t, dl, sign, flip):
    """[B,N,H,W] sampled at (x + sign * dl, y) through the reference's grid (trainer.py:427-441) and the oracle's grid_sample."""
    Bn, N, H, W = t.shape
    xs = torch.arange(W, dtype=t.dtype).view(1, 1, 1, W).expand(Bn, N, H, W)
    ys = torch.arange(H, dtype=t.dtype).view(1, 1, H, 1).expand(Bn, N, H, W)
    gx = ((xs + sign * dl) / (W - 1) - 0.5) * 2
    gy = (ys / (H - 1) - 0.5) * 2
    grid = torch.stack([gx, gy], -1).reshape(Bn * N, H, W, 2)
    src = t.flip(-1) if flip else t
    return orc.bilinear_sample(src.reshape(Bn * N, 1, H, W), grid, "zeros").reshape(Bn, N, H, W)


def blend(disp, o_l, o_fr):
    """trainer.py:458-461."""
    B = o_l.shape[0]
    mean = disp[:B] * 0.5 + disp[B:].flip(-1) * 0.5
    pp = mean * o_fr + disp[:B] * (1 - o_fr)
    return pp * o_l + disp[B:].flip(-1) * (1 - o_l)


@functools.lru_cache(maxsize=None)
def reference(name, dtype):
    """The post-process of a case in ``dtype`` with its intermediates: the unclamped plane sums ("o_l_raw", ...), the masks and
    disp_pp per fill.  Computed once per process and shared by every test; nobody writes into it."""
    c, z = BY_NAME[name], inputs(name)
    B = c.B
    lg, pr, dl = (z[k].to(dtype) for k in ("logits", "prob", "dl"))
    r = {}
    plr = torch.softmax(_warp(lg[:B], dl[:B], +1.0, False), 1)
    r["o_l_raw"] = _warp(plr, dl[B:], -1.0, False).sum(1, True)
    pfrl = torch.softmax(_warp(lg[B:], dl[B:], -1.0, True), 1)
    r["o_fr_raw"] = _warp(pfrl, dl[:B], +1.0, False).sum(1, True)
    r["mask_novel_raw"] = _warp(pr[:B], dl[:B], +1.0, False).sum(1, True)
    for k in ("o_l", "o_fr", "mask_novel"):
        r[k] = r[k + "_raw"].clamp(max=1)
    for fill in FILLS:
        r["disp_pp/" + fill] = blend(disp_fill(name, fill).to(dtype), r["o_l"], r["o_fr"])
    return r


def pixel_err(got, ref64):
    """Largest per-pixel |got - ref| in units of max(1, max|ref|)."""
    ref64 = ref64.double()
    return float((got.double().cpu() - ref64).abs().max()) / max(1.0, float(ref64.abs().max()))


def bar(e_ref, N):
    return 2.0 * e_ref + N * EPS


OUTPUTS = ["mask_novel"] + ["disp_pp/" + f for f in FILLS]


def e_ref(name, key):
    return pixel_err(reference(name, torch.float32)[key], reference(name, torch.float64)[key])


WARP_COMBOS = [(+1.0, False), (-1.0, False), (-1.0, True), (+1.0, True)]   # (sign, flip_src)
NO_CAP = 1e9


@functools.lru_cache(maxsize=None)
def warp_reference(name, sign, flip, dtype):
    """The standalone warps of a case's image half: softmax over the warped logits; the unclamped plane sum of the warped
    probabilities."""
    c, z = BY_NAME[name], inputs(name)
    lg, pr, dl = (z[k][:c.B].to(dtype) for k in ("logits", "prob", "dl"))
    return dict(softmax=torch.softmax(_warp(lg, dl, sign, flip), 1), sum_raw=_warp(pr, dl, sign, flip).sum(1, True))


# =====================================================================================================================
# CPU: the route table, its coverage, the heights, the inputs' conditions
# =====================================================================================================================
def _fused_route(c, ws_ptr=0, out_ptr=0):
    r = ops.post_process_route(c.B, c.N, c.H, c.W, FLAG[c.form], ws_ptr, out_ptr)
    return (r["family"], r["nmax"], r["rows2"], r["alias"], r["lds_bytes"])


@pytest.mark.parametrize("name", IDS)
def test_route_table_matches_the_query(name):
    c = BY_NAME[name]
    assert _fused_route(c, 4 if c.ws4 else 0) == c.fused
    assert c.B * c.N * c.H * c.W <= 2 * 64 * 14 * 1026 and c.B in (1, 2)
    for flip in (False, True):
        fl = FLAG[c.form] | (C.PD_PP_FLIP_SRC if flip else 0)
        sm, su = ops.warp_route("softmax", c.B, c.N, c.H, c.W, fl), ops.warp_route("sum", c.B, c.N, c.H, c.W, fl)
        assert (sm["family"], sm["nmax"], sm["flip"]) == c.softmax + (flip,)
        assert (su["family"], su["nmax"], su["flip"]) == (c.wsum, 0, flip)
        assert sm["lds_bytes"] == su["lds_bytes"] == 0 and not (sm["rows2"] or sm["alias"] or su["rows2"] or su["alias"])
        # an output that is 4-byte aligned only: the pixel-pair stores of the segment kernels are out
        for kind, fam in (("softmax", c.softmax[0]), ("sum", c.wsum)):
            r4 = ops.warp_route(kind, c.B, c.N, c.H, c.W, fl, 4)
            assert (r4["family"], r4["nmax"]) == (("rows" if fam == "seg" else fam), 0)
    if c.fused[0] != SINGLE:   # either buffer 4-byte aligned only: the single warps
        assert _fused_route(c, 4, 0)[0] == SINGLE and _fused_route(c, 0, 4)[0] == SINGLE and _fused_route(c, 8, 16) == c.fused


def test_single_warps_of_the_unaligned_workspace_take_the_row_kernels():
    """pd_post_process on a workspace at 4 (mod 8): the [B,N,H,W] intermediate sits at the workspace's start and o_l / o_fr
    behind B N H W (even) floats — all at 4 (mod 8), so four of the six warps leave the segment form; mask_novel keeps it."""
    c = BY_NAME["n12_w128_ws4"]
    assert (c.B * c.N * c.H * c.W) % 2 == 0 and (c.B * c.H * c.W) % 2 == 0
    assert ops.warp_route("softmax", c.B, c.N, c.H, c.W, 0, 4)["family"] == "rows"
    assert ops.warp_route("sum", c.B, c.N, c.H, c.W, 0, 4 + 4 * c.B * c.N * c.H * c.W)["family"] == "rows"
    assert ops.warp_route("sum", c.B, c.N, c.H, c.W, 0, 0)["family"] == "seg"


def test_route_queries_validate_like_the_entry_points():
    lib = C.load()
    r = C.PpRoute()
    assert lib.pd_warp_route(0, 1, 4, 8, 1, 0, None, ctypes.byref(r)) == 1 and b"bad shape" in lib.pd_last_error()
    assert lib.pd_warp_route(0, 1, 4, 8, 8, 8, None, ctypes.byref(r)) == 1 and b"unknown flags" in lib.pd_last_error()
    assert lib.pd_warp_route(0, 1, 4, 8, 8, 5, None, ctypes.byref(r)) == 1 and b"exclude" in lib.pd_last_error()
    assert lib.pd_warp_route(2, 1, 4, 8, 8, 0, None, ctypes.byref(r)) == 1 and b"kind" in lib.pd_last_error()
    assert lib.pd_warp_route(0, 1, 4, 8, 8, 0, None, None) == 1
    assert lib.pd_post_process_route(1, 4, 8, 8, C.PD_PP_FLIP_SRC, None, None, ctypes.byref(r)) == 1
    assert lib.pd_post_process_route(0, 4, 8, 8, 0, None, None, ctypes.byref(r)) == 1
    assert lib.pd_post_process_route(1, 4, 8, 8, 0, None, None, None) == 1


def test_every_reachable_instantiation_is_in_the_table():
    """Every (N, W, form) with N <= 70 and W <= 1030 through the query: the kernel instantiations the fused call can reach
    at 160 KiB are exactly the table's, and so are the warps'.  The two that no shape reaches are the NPART = 11 and NPART = 18
    alias forms of pp_chain_split_kernel: alias needs N (W + 4) 4 + 3 nseg 1024 > 163840, and with N <= 54 (NPART <= 18) and
    W <= 640 (the split chains' widths: nseg <= 5) the left side is at most 54 * 644 * 4 + 15360 = 154464.  The library does not
    instantiate these two: a route that asked for one would answer PD_ERR_UNSUPPORTED."""
    assert 54 * (640 + 4) * 4 + 3 * 5 * 1024 == 154464 < LDS < 55 * (640 + 4) * 4 + 3 * 5 * 1024 + 5 * 644 * 4
    lib, r = C.load(), C.PpRoute()
    fused, sm, su = set(), set(), set()
    for form in ("plane", "rows", "dense"):
        for N in range(1, 71):
            for W in range(2, 1031):
                assert lib.pd_post_process_route(1, N, 14, W, FLAG[form], None, None, ctypes.byref(r)) == 0
                fused.add((C.PD_PP_FAMILIES[r.family], r.nmax, bool(r.rows2), bool(r.alias)))
                if r.family != 3:   # the LDS request fits the CU (the exact fit included) and, aliased, holds the 9 maps
                    assert r.lds_bytes <= LDS and (not r.alias or 9 * -(-W // 128) * 1024 <= r.lds_bytes)
                assert lib.pd_warp_route(0, 1, N, 14, W, FLAG[form], None, ctypes.byref(r)) == 0
                sm.add((C.PD_PP_FAMILIES[r.family], r.nmax))
                assert lib.pd_warp_route(1, 1, N, 14, W, FLAG[form], None, ctypes.byref(r)) == 0
                su.add((C.PD_PP_FAMILIES[r.family], r.nmax))
    assert fused == {c.fused[:4] for c in CASES}
    every_split = {(SPLIT, p, r2, al) for p in (11, 18, 22) for r2 in (False, True) for al in (False, True)}
    every_chain = {(CHAIN, m, r2, False) for m in (32, 52, 64) for r2 in (False, True)}
    assert (every_split | every_chain) - fused == {(SPLIT, p, r2, True) for p in (11, 18) for r2 in (False, True)}
    assert sm == {c.softmax for c in CASES} == {("seg", 32), ("seg", 52), ("seg", 64), ("rows", 0), ("gather", 0)}
    assert su == {(c.wsum, 0) for c in CASES} == {("seg", 0), ("rows", 0), ("gather", 0)}
    assert LDS in {c.fused[4] for c in CASES}           # the exact fit
    assert {c.H for c in CASES} == {2, 7, 14} and sum(c.H == 2 for c in CASES) == sum(c.H == 7 for c in CASES) == 1
    assert {c.form for c in CASES} == {"plane", "rows", "dense"} and any(c.ws4 for c in CASES)


def _row_round_trip(H):
    """The reference's fp32 row coordinate of every target row: y -> [-1, 1] (trainer.py:433) -> grid_sample's pixel."""
    y = torch.arange(H, dtype=torch.float32)
    return ((y / (H - 1) - 0.5) * 2 + 1) / 2 * (H - 1), y


def test_heights_cover_one_and_two_row_targets():
    """NR = 1 where the round trip returns y exactly, NR = 2 where it lands below y (rows y - 1, y) or above (rows y, y + 1);
    under rows2 a source row then serves its neighbour above or below through the S maps 1 / 2."""
    iy, y = _row_round_trip(14)
    assert torch.nonzero(iy < y).flatten().tolist() == [1, 2, 3] and torch.nonzero(iy > y).flatten().tolist() == [7]
    assert float((iy - y).abs().max()) < 2e-6
    iy, y = _row_round_trip(7)
    assert int((iy != y).sum()) == 1
    iy, y = _row_round_trip(2)
    assert bool((iy == y).all())
    for r2 in (False, True):   # both directions and one-row targets under each chain family, with and without rows2
        for fam in (SPLIT, CHAIN):
            assert any(c.H == 14 and c.fused[0] == fam and c.fused[2] == r2 for c in CASES)


@pytest.mark.parametrize("name", IDS)
def test_conditions_cpu(name):
    c = BY_NAME[name]
    r64, r32 = reference(name, torch.float64), reference(name, torch.float32)
    z = inputs(name)
    got = orc.post_process_disp(z["logits"], z["prob"], disp_fill(name, "real"), z["dl"])   # the restatement above IS the oracle's
    assert torch.equal(got[0], r64["disp_pp/real"]) and torch.equal(got[1], r64["mask_novel"])
    rep = REPORT.setdefault(name, {})
    for k in ("o_l", "o_fr", "mask_novel"):
        share = float((r64[k + "_raw"] >= 1).double().mean())
        rep["clamped/" + k] = round(share, 4)
        print("%s clamped share of %s: %.3f" % (name, k, share))
        assert share <= SHARE_MAX, (name, k, share)
        assert share >= SHARE_MIN, (name, k, share)
    for k in OUTPUTS:
        e = e_ref(name, k)
        rep["E_ref/" + k] = e
        print("%s E_ref %s: %.3e" % (name, k, e))
        assert e <= E_REF_MAX, (name, k, e)
        assert pixel_err(r32[k], r64[k]) <= bar(e, c.N)
    for sign, flip in WARP_COMBOS:
        w64, w32 = warp_reference(name, sign, flip, torch.float64), warp_reference(name, sign, flip, torch.float32)
        e = slice_report(w32["softmax"], w64["softmax"], plane_floor=1e-2)["err"]
        assert e <= E_REF_MAX, (name, "warp_softmax", sign, flip, e)
        assert pixel_err(w32["sum_raw"], w64["sum_raw"]) <= E_REF_MAX
    lv = z["lv"]
    if c.N >= 5:
        assert bool((lv == 0).any(1).all()) and bool((lv == c.W - 1).any(1).all())
        assert bool(((lv == lv.round()) & (lv > 0) & (lv < c.W - 1)).any(1).all())
    if c.N >= 8:
        assert bool((lv[:c.B] == c.W + 5).any()) and bool((lv[c.B:] == c.W + 5).any())
        assert not bool(((lv[:c.B] == c.W + 5) & (lv[c.B:] == c.W + 5)).any())
    if c.W >= 402:
        assert float(lv[lv < c.W].max()) > 250.0
    if c.form == "rows":
        assert bool((z["rows"][:, c.N - c.N // 3:, 0] != z["rows"][:, c.N - c.N // 3:, -1]).any())
        assert bool((z["rows"][:, :c.N - c.N // 3, 0] == z["rows"][:, :c.N - c.N // 3, -1]).all())


# =====================================================================================================================
# GPU
# =====================================================================================================================
@pytest.fixture(scope="module", autouse=True)
def _parity_report():
    yield
    path = os.environ.get("PD_POST_PROCESS_PARITY_JSON")
    if path and REPORT:
        with open(path, "w") as f:
            json.dump(REPORT, f, indent=1, sort_keys=True)


def _dev(t):
    return t.float().to(DEV).contiguous()


def _operands(name):
    """Device tensors of a case: logits, prob, and the disparities in the form the C ABI reads / in the view ops recognises."""
    c, z = BY_NAME[name], inputs(name)
    if c.form == "plane":
        compact = _dev(z["lv"])
        view = compact.view(2 * c.B, c.N, 1, 1).expand(-1, -1, c.H, c.W)
    elif c.form == "rows":
        compact = _dev(z["rows"])
        view = compact[..., None].expand(-1, -1, -1, c.W)
    else:
        compact = view = _dev(z["dl"])
    return _dev(z["logits"]), _dev(z["prob"]), compact, view


def _fused_abi(c, logits, prob, disp, compact, ws, ws_off=0):
    """pd_post_process through the C ABI on a given workspace (``ws_off`` floats into ``ws``)."""
    lib = C.load()
    disp_pp = torch.empty(c.B, 1, c.H, c.W, device=DEV)
    mask_novel = torch.empty_like(disp_pp)
    wsp = ws.data_ptr() + 4 * ws_off
    got = _fused_route(c, wsp, disp_pp.data_ptr())
    with C.on_device(logits.device):
        C.check(lib.pd_post_process(c.B, c.N, c.H, c.W, FLAG[c.form], C.ptr(logits), C.ptr(prob), C.ptr(disp), C.ptr(compact),
                                    ctypes.c_void_p(wsp), C.ptr(disp_pp), C.ptr(mask_novel), C.stream_handle(logits.device)),
                "pd_post_process")
    return disp_pp, mask_novel, got


def _stepwise_abi(c, logits, prob, disp, compact, ws, ws_off):
    """The six single calls on the workspace layout pd_post_process uses (planes, o_l, o_fr): the same alignments."""
    lib, B, N, H, W = C.load(), c.B, c.N, c.H, c.W
    img, P = N * H * W, H * W
    half = compact.numel() // 2
    base = ws.data_ptr() + 4 * ws_off
    planes, o_l, o_fr = (ctypes.c_void_p(base + 4 * o) for o in (0, B * img, B * img + B * P))
    dl_r, dl_l = ctypes.c_void_p(compact.data_ptr()), ctypes.c_void_p(compact.data_ptr() + 4 * half)
    lg_l = ctypes.c_void_p(logits.data_ptr() + 4 * B * img)
    disp_pp = torch.empty(B, 1, H, W, device=DEV)
    mask_novel = torch.empty_like(disp_pp)
    fl, st = FLAG[c.form], C.stream_handle(logits.device)
    with C.on_device(logits.device):
        C.check(lib.pd_warp_softmax(B, N, H, W, 1.0, fl, C.ptr(logits), dl_r, planes, st), "pd_warp_softmax")
        C.check(lib.pd_warp_sum(B, N, H, W, -1.0, fl, planes, dl_l, 1.0, o_l, st), "pd_warp_sum")
        C.check(lib.pd_warp_softmax(B, N, H, W, -1.0, fl | C.PD_PP_FLIP_SRC, lg_l, dl_l, planes, st), "pd_warp_softmax")
        C.check(lib.pd_warp_sum(B, N, H, W, 1.0, fl, planes, dl_r, 1.0, o_fr, st), "pd_warp_sum")
        C.check(lib.pd_pp_combine(B, H, W, C.ptr(disp), o_fr, o_l, C.ptr(disp_pp), st), "pd_pp_combine")
        C.check(lib.pd_warp_sum(B, N, H, W, 1.0, fl, C.ptr(prob), dl_r, 1.0, C.ptr(mask_novel), st), "pd_warp_sum")
    return disp_pp, mask_novel


def _bits(t):
    return t.contiguous().view(torch.int32)


@gpu
@pytest.mark.parametrize("name", IDS)
def test_fused_post_process_per_pixel(name):
    c = BY_NAME[name]
    r64 = reference(name, torch.float64)
    logits, prob, compact, view = _operands(name)
    ws = torch.empty(C.load().pd_post_process_workspace_floats(c.B, c.N, c.H, c.W) + 2, device=DEV)
    off = (1 if c.ws4 else 0) + (0 if ws.data_ptr() % 8 == 0 else 1)     # 8-byte aligned, or 4 (mod 8)
    rep = REPORT.setdefault(name, {})
    failures = []
    for fill in FILLS:
        disp = _dev(disp_fill(name, fill))
        disp_pp, mask_novel, route = _fused_abi(c, logits, prob, disp, compact, ws, off)
        assert route == c.fused, (route, c.fused)
        rep["route"] = list(route)
        for key, got in (("disp_pp/" + fill, disp_pp), ("mask_novel", mask_novel)):
            assert bool(torch.isfinite(got).all()), key
            e, e0 = pixel_err(got, r64[key]), e_ref(name, key)
            rep["product/" + key] = max(e, rep.get("product/" + key, 0.0))
            rep["E_ref/" + key] = e0
            print("%s %s: product %.3e  E_ref %.3e  bar %.3e" % (name, key, e, e0, bar(e0, c.N)))
            if not e <= bar(e0, c.N):
                failures.append((key, e, e0, bar(e0, c.N)))
        # two runs, the same bits (no atomics in the file)
        again = _fused_abi(c, logits, prob, disp, compact, ws, off)
        assert torch.equal(_bits(again[0]), _bits(disp_pp)) and torch.equal(_bits(again[1]), _bits(mask_novel)), fill
        # against the single warps, per pixel
        if c.ws4:
            step = _stepwise_abi(c, logits, prob, disp, compact, torch.empty_like(ws), off)
        else:
            step = ops.post_process_disp_stepwise(logits, prob, disp, view, row_uniform=c.form == "rows")
            via_ops = ops.post_process_disp(logits, prob, disp, view, row_uniform=c.form == "rows")   # the Python path: the same call
            assert torch.equal(_bits(via_ops[0]), _bits(disp_pp)) and torch.equal(_bits(via_ops[1]), _bits(mask_novel)), fill
        for got, want in zip((disp_pp, mask_novel), step):
            d, allow = float((got - want).abs().max()), CHAIN_VS_STEPWISE * max(1.0, float(want.abs().max()))
            if c.fused[0] == SINGLE and not torch.equal(_bits(got), _bits(want)):
                failures.append(("single warps, not the stepwise bits", fill, d))
            elif not d <= allow:
                failures.append(("fused vs stepwise", fill, d, allow))
    assert not failures, failures


@gpu
@pytest.mark.parametrize("name", IDS)
def test_standalone_warps_per_pixel(name):
    c = BY_NAME[name]
    logits, prob, compact, view = _operands(name)
    B = c.B
    rep = REPORT.setdefault(name, {})
    failures = []
    ru = dict(row_uniform=c.form == "rows")
    for sign, flip in WARP_COMBOS:
        w64, w32 = warp_reference(name, sign, flip, torch.float64), warp_reference(name, sign, flip, torch.float32)
        got = ops.warp_softmax(logits[:B], view[:B], sign, flip_src=flip, **ru)
        again = ops.warp_softmax(logits[:B], view[:B], sign, flip_src=flip, **ru)
        assert torch.equal(_bits(got), _bits(again))
        rep_g = slice_report(got, w64["softmax"], plane_floor=1e-2)
        e0 = slice_report(w32["softmax"], w64["softmax"], plane_floor=1e-2)["err"]
        assert rep_g["zero_ok"] and math.isfinite(rep_g["err"])
        print("%s warp_softmax %+d flip %d: product %.3e  E_ref %.3e" % (name, sign, flip, rep_g["err"], e0))
        rep["product/warp_softmax"] = max(rep_g["err"], rep.get("product/warp_softmax", 0.0))
        rep["E_ref/warp_softmax"] = max(e0, rep.get("E_ref/warp_softmax", 0.0))
        if not rep_g["err"] <= bar(e0, c.N):
            failures.append(("warp_softmax", sign, flip, rep_g["err"], e0))
        for cap in (1.0, NO_CAP):
            got = ops.warp_sum(prob[:B], view[:B], sign, cap=cap, flip_src=flip, **ru)
            again = ops.warp_sum(prob[:B], view[:B], sign, cap=cap, flip_src=flip, **ru)
            assert torch.equal(_bits(got), _bits(again))
            ref = w64["sum_raw"].clamp(max=cap)
            assert cap == 1.0 or float(w64["sum_raw"].max()) < cap / 2      # nothing hidden
            e, e0 = pixel_err(got, ref), pixel_err(w32["sum_raw"].clamp(max=cap), ref)
            print("%s warp_sum %+d flip %d cap %g: product %.3e  E_ref %.3e" % (name, sign, flip, cap, e, e0))
            rep["product/warp_sum"] = max(e, rep.get("product/warp_sum", 0.0))
            rep["E_ref/warp_sum"] = max(e0, rep.get("E_ref/warp_sum", 0.0))
            if not e <= bar(e0, c.N):
                failures.append(("warp_sum", sign, flip, cap, e, e0))
    assert not failures, failures


# =====================================================================================================================
# Reads and writes stay inside what was handed over (one case per kernel family, through the C ABI)
# =====================================================================================================================
def _guard_tools():
    import test_operator_sweeps as T
    return T.Guarded, T._inp, T._call


@gpu
@pytest.mark.parametrize("name", ["n12_w128_dense", "n9_w129", "n55_w130"], ids=["gather", "rows", "seg"])
def test_guards_warps(name):
    Guarded, _inp, _call = _guard_tools()
    c, z = BY_NAME[name], inputs(name)
    B, N, H, W = c.B, c.N, c.H, c.W
    half = {"plane": z["lv"], "rows": z["rows"], "dense": z["dl"]}[c.form][:B]
    planes, prob, disp = _inp(z["logits"][:B]), _inp(z["prob"][:B]), _inp(half)
    for flip in (0, C.PD_PP_FLIP_SRC):
        fl = FLAG[c.form] | flip
        assert ops.warp_route("softmax", B, N, H, W, fl)["family"] == c.softmax[0] and ops.warp_route("sum", B, N, H, W, fl)["family"] == c.wsum
        for sign in (1.0, -1.0):
            res = []
            for zero in (False, True):
                sm, su = Guarded(B * N * H * W), Guarded(B * H * W)
                if zero:
                    sm.floats().zero_(), su.floats().zero_()
                assert sm.buf.data_ptr() % 8 == 0 and su.buf.data_ptr() % 8 == 0
                _call("pd_warp_softmax", B, N, H, W, sign, fl, planes.ptr, disp.ptr, sm.ptr)
                _call("pd_warp_sum", B, N, H, W, sign, fl, prob.ptr, disp.ptr, ctypes.c_float(NO_CAP), su.ptr)
                if not zero:
                    sm.check("pd_warp_softmax out"), su.check("pd_warp_sum out")
                assert bool(torch.isfinite(sm.floats()).all()) and bool(torch.isfinite(su.floats()).all()), "a NaN: read past an input's end"
                res.append((sm.buf.clone(), su.buf.clone()))
            assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    planes.check("planes", written=0), prob.check("probability", written=0), disp.check("disp", written=0)


@gpu
@pytest.mark.parametrize("name", ["n52_w770", "n34_w258", "n63_w640_rows", "n11_w128"], ids=["chain_rows2", "split", "split_alias_rows2", "split_rows2"])
def test_guards_fused(name):
    Guarded, _inp, _call = _guard_tools()
    c, z = BY_NAME[name], inputs(name)
    B, N, H, W = c.B, c.N, c.H, c.W
    compact = {"plane": z["lv"], "rows": z["rows"], "dense": z["dl"]}[c.form]
    logits, prob, disp, dl = _inp(z["logits"]), _inp(z["prob"]), _inp(disp_fill(name, "real")), _inp(compact)
    nws = C.load().pd_post_process_workspace_floats(B, N, H, W)
    res = []
    for zero in (False, True):
        ws, disp_pp, mask_novel = Guarded(nws), Guarded(B * H * W), Guarded(B * H * W)
        if zero:
            ws.floats().zero_(), disp_pp.floats().zero_(), mask_novel.floats().zero_()
        assert _fused_route(c, ws.buf.data_ptr(), disp_pp.buf.data_ptr()) == c.fused
        _call("pd_post_process", B, N, H, W, FLAG[c.form], logits.ptr, prob.ptr, disp.ptr, dl.ptr, ws.ptr, disp_pp.ptr, mask_novel.ptr)
        ws.check("workspace", written=0)
        if not zero:
            disp_pp.check("disp_pp"), mask_novel.check("mask_novel")
        else:
            disp_pp.check("disp_pp", written=0), mask_novel.check("mask_novel", written=0)
        assert bool(torch.isfinite(disp_pp.floats()).all()), "a NaN in disp_pp: an S map or an input read where nothing was written"
        assert bool(torch.isfinite(mask_novel.floats()).all())
        res.append((disp_pp.buf.clone(), mask_novel.buf.clone()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    for t, what in ((logits, "logits"), (prob, "probability"), (disp, "disp"), (dl, "disp_layered")):
        t.check(what, written=0)
