"""Decoder tails: every launch shape of the ten tail kernels against the fp64 oracle, measured per ELEMENT against the terms that
make the element (cases.term_report) instead of per tensor.

Why.  The tail kernels share one per-plane step, so the equalities the suite asserts between routes (rows = dense, bf16 = fp32
rounded once, inference = training) pass for an error all routes share, and ``rel_err`` (max|a-b| / max|b| of the tensor) gives a
low-probability plane thousands of times the budget: a backward that scales ``gD (d_n - disp) P_n`` by 1.001 where P_n < 1e-3 moves
the tensor norm by 1e-7.  Here an element's budget is its ALLOWANCE, the sum of the absolute values of the terms of the backward's own
formula (pd_decoder_tail.hip), from the fp64 oracle's tensors:

    g_raw_logits          (|g_logits| + |gD| (|d_n| + |disp|) P_n) m
    g_raw_sigma           (|g_sigma| + |gD| (|d_n| + |disp|) P_n / sigma_n) s (1 - s)   where the clamp gate is open, else 0
    g_disp_layered        |gD| P_n, summed over x (rows) or over y and x (per plane)
    |gD| = |g_disp| + |g_depth| c / disp^2;  every forward tensor: |ref| (plain relative error per element)

The bar, per tensor against the fp64 run: err <= 2 E_ref + 1e-4 (E_ref: the oracle's fp32 run under the same metric) AND err < 1e-4
outright; where the allowance is 0 the result is exactly 0.

The table CASES holds one small case per branch of the launch arithmetic of tail_launch / tail_px / pd_decoder_tail_bwd;
``test_the_table_covers_the_launch_arithmetic`` restates those rules and proves the coverage without a GPU.  Inputs are kink-free
(``test_conditions``): raw_sigma in [-9, 6] and never within 0.02 of logit(0.01), so that fp32 and fp64 take the same side of the
clamp and 1 - s >= 2.5e-3; no pixel of a mixture case has every plane masked.

Every case runs three backward passes — upstream on disp / depth only ("geom": g_raw_logits is then purely gD (d_n - disp) P_n, a
low-probability plane has nothing to hide behind), on logits / sigma only ("conv"), and jointly ("all") — and the two partial results
add up to the joint one within LINEAR_TOL of the joint allowance.

PD_TAIL_PARITY_JSON=<file> writes every figure (err, E_ref, rel_err per case and tensor; the launch shapes): the source of
profiles/tail_form_parity.md."""
import functools
import json
import math
import os
import re
import zlib
from typing import NamedTuple, Optional

import pytest
import torch

from cases import rel_err, term_report
from oracle import planedepth_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
BF = torch.bfloat16
gpu = pytest.mark.gpu

TOL = 1e-4                 # the project's bar
E_REF_CAP = 5e-5           # the oracle's own fp32 run per element: measured <= 4.6e-5 (profiles/tail_form_parity.md)
SIGMA_LO, SIGMA_HI = -9.0, 6.0
KINK = math.log(0.01 / 0.99)   # logit(0.01) = -4.59512: where sigma's lower clamp bound opens
KINK_MARGIN = 0.02
# g(geom) + g(conv) against g(all): the fp64 formula is linear in its upstream gradients and the joint allowance is the sum of the
# two partial ones, so the three fp32 results differ by roundings of terms the allowance bounds: gl + t once (2^-24), gs - t / sg and
# its two products by s and 1 - s, on each side — under ten roundings in all, 6e-7; 1e-6 is 16 of them.
LINEAR_TOL = 1e-6
PLADE_FLOOR = 0.1          # PladeNet tail: an element of a [B,N,H,W] tensor against max(|ref|, 0.1 max_n |ref| at its pixel)
PLADE_E_REF_CAP = 2e-4     # the oracle's own fp32 run under that floor, where test_plade_conditions asks for it: measured <= 9.4e-5
COMBOS = ("geom", "conv", "all")
REPORT = {}                # "family/case/mode" -> {tensor: {err, e_ref, rel_err}}


class Case(NamedTuple):
    name: str
    shape: tuple                 # (B, N, H, W)
    disp: str                    # plane | dense | rows
    mask: Optional[str]          # None | dense | rows
    disp_grad: bool = True       # False: the disparities take no gradient (the row-owned backward then has no LDS, g_dl == NULL)
    offset: bool = False         # the conv outputs start one element into their storage: 1 pixel per lane at H*W % 4 == 0
    spread: float = 2.5          # standard deviation of the raw logits (6: the online softmax moves its reference often)


CASES = [
    # pixel-linear kernels (forward, layers, tail_bwd_kernel)
    Case("px4_two_blocks", (2, 3, 7, 148), "plane", None),                # H*W = 1036: 259 lanes of 4, second block has 3
    Case("px1_two_blocks", (2, 3, 3, 87), "dense", "dense"),              # H*W = 261: 1 pixel per lane, second block has 5
    Case("full_block", (2, 3, 4, 256), "dense", None),                    # 256 lanes of 4: exactly one full block
    Case("planes300", (2, 300, 7, 148), "plane", "dense"),                # two blocks, two strides of the zero / store loops
    Case("one_plane", (2, 1, 3, 87), "plane", None),
    Case("two_planes", (2, 2, 7, 148), "plane", None),
    Case("misaligned", (2, 3, 4, 16), "plane", "dense", offset=True),
    Case("dense_row_mask", (2, 5, 4, 66), "dense", "rows"),               # H*W % 4 == 0, W % 4 != 0: kRowMask at 1 pixel per lane
    Case("plane_row_mask", (2, 5, 7, 148), "plane", "rows"),              # kRowMask with the per-plane reduction, 4 pixels per lane
    # row-owned backward (tail_bwd_rows_kernel)
    Case("rows_4x66", (2, 5, 4, 66), "rows", "rows"),                     # H*W % 4 == 0 but W % 4 != 0; 2 waves
    Case("rows_2x6", (2, 5, 2, 6), "rows", "rows"),
    Case("rows_w260", (2, 5, 2, 260), "rows", "rows"),                    # px 4: 2 waves, one live lane in the second
    Case("rows_w260_nograd", (2, 5, 2, 260), "rows", None, disp_grad=False),
    Case("rows_w516", (1, 5, 5, 516), "rows", None),                      # px 4: 3 waves
    Case("rows_w1028_n70", (1, 70, 2, 1028), "rows", "rows", spread=6.0),  # px 4: 4 waves, 2 trips, one live lane in the second
    Case("rows_w65_dense_mask", (2, 5, 2, 65), "rows", "dense"),          # px 1: 2 waves; row disparities with a dense mask
    Case("rows_w193_n300", (1, 300, 2, 193), "rows", "rows"),             # px 1: 4 waves, 300 planes
    Case("rows_w193_n4096", (1, 4096, 1, 193), "rows", None),             # the 64 KiB of LDS the entry point allows
    Case("rows_w257", (2, 5, 5, 257), "rows", "rows"),                    # px 1: 2 trips
    Case("rows_w257_nograd", (1, 5, 2, 257), "rows", "rows", disp_grad=False),
    Case("rows_w513", (1, 5, 2, 513), "rows", None),                      # px 1: 3 trips
    Case("rows_w44_n70", (2, 70, 5, 44), "rows", "rows"),                 # one wave, 70 planes: the final loop takes a second step
]
BY_NAME = {c.name: c for c in CASES}
IDS = [c.name for c in CASES]
# the PladeNet tail has no row form: the pixel-linear entries, N = 300 and the N = 2 minimum (its mask entry is not used)
PLADE_CASES = ["px4_two_blocks", "px1_two_blocks", "full_block", "planes300", "two_planes", "misaligned"]
# the entries that introduce a px, wave count or trip count the route equalities of the suite have not seen
NEW_ROW_SHAPES = ["rows_4x66", "rows_w260", "rows_w516", "rows_w1028_n70", "rows_w65_dense_mask", "rows_w193_n300", "rows_w257",
                  "rows_w513", "rows_w44_n70"]
NEW_SHAPES = ["px4_two_blocks", "px1_two_blocks", "planes300", "misaligned", "dense_row_mask", "plane_row_mask"] + NEW_ROW_SHAPES


def _kernel_constants():
    text = open(os.path.join(ROOT, "planedepth_amd", "csrc", "pd_common.h")).read()
    return tuple(int(re.search(r"constexpr int %s = (\d+);" % k, text).group(1)) for k in ("kBlock", "kWave"))


def ceil_div(a, b):
    return -(-a // b)


def launch_shape(case, kBlock, kWave):
    """tail_px / tail_launch / pd_decoder_tail_bwd restated: what the entry points launch for a case."""
    B, N, H, W = case.shape
    row_form = case.disp == "rows" or case.mask == "rows"
    px = 4 if (H * W) % 4 == 0 and not case.offset and (not row_form or W % 4 == 0) else 1
    lanes = ceil_div(H * W, px)
    grid = ceil_div(lanes, kBlock)
    s = dict(px=px, lanes=lanes, grid=grid, last_block=lanes - (grid - 1) * kBlock, waves=None, trips=None, shmem=None,
             strides=ceil_div(N, kBlock))
    if case.disp == "rows":
        row_lanes = ceil_div(W, px)
        waves = min(kBlock // kWave, ceil_div(row_lanes, kWave))
        trips = ceil_div(W, kWave * waves * px)
        last_trip_lanes = row_lanes - (trips - 1) * kWave * waves
        s.update(waves=waves, trips=trips, shmem=waves * N * 4 if case.disp_grad else 0, last_trip_lanes=last_trip_lanes,
                 last_wave_lanes=last_trip_lanes - (ceil_div(last_trip_lanes, kWave) - 1) * kWave,
                 final_steps=ceil_div(N, kWave * waves))
    elif case.disp == "plane" and case.disp_grad:
        s["shmem"] = N * 4
    return s


def test_the_table_covers_the_launch_arithmetic():
    """A later edit that drops a branch of the launch arithmetic from the table fails here, without a GPU."""
    kBlock, kWave = _kernel_constants()
    assert (kBlock, kWave) == (256, 64)     # the widths below are chosen for these
    L = {c.name: launch_shape(c, kBlock, kWave) for c in CASES}
    assert len(BY_NAME) == len(CASES)

    def some(pred):
        return any(pred(c, L[c.name]) for c in CASES)

    pixel = lambda c: c.disp != "rows"  # noqa: E731
    # pixel-linear kernels
    assert some(lambda c, s: pixel(c) and c.shape[2] * c.shape[3] == 1036 and s["px"] == 4 and s["grid"] == 2 and s["last_block"] == 3
                and c.shape[0] >= 2)
    assert some(lambda c, s: pixel(c) and c.shape[2] * c.shape[3] == 261 and s["px"] == 1 and s["grid"] == 2 and c.shape[0] >= 2)
    assert some(lambda c, s: pixel(c) and s["grid"] == 1 and s["last_block"] == kBlock and c.shape[0] >= 2)
    for hw in ((4, 66), (2, 6)):        # a row form with H*W % 4 == 0 but W % 4 != 0 takes one pixel per lane
        assert some(lambda c, s: c.shape[2:] == hw and "rows" in (c.disp, c.mask) and s["px"] == 1 and c.shape[0] >= 2)
    # per-plane disparity gradient: [B,N,1,1] leaf, workspace reduction
    assert some(lambda c, s: c.disp == "plane" and c.disp_grad and c.shape[1] == 300 and s["grid"] == 2 and s["strides"] == 2
                and c.shape[2] * c.shape[3] == 1036)
    for n in (1, 2):
        assert some(lambda c, s: c.disp == "plane" and c.disp_grad and c.shape[1] == n)
    # row-owned backward: every width with the rows' gradient, and the form without it
    rows = {(s["px"], c.shape[3]): dict(s, N=c.shape[1]) for c, s in ((c, L[c.name]) for c in CASES)
            if c.disp == "rows" and c.disp_grad}
    want = {(4, 260): (2, 1), (4, 516): (3, 1), (4, 1028): (4, 2), (1, 65): (2, 1), (1, 193): (4, 1), (1, 257): (4, 2), (1, 513): (4, 3)}
    for key, (waves, trips) in want.items():
        assert key in rows, key
        assert (rows[key]["waves"], rows[key]["trips"]) == (waves, trips), (key, rows[key])
        assert rows[key]["shmem"] == waves * rows[key]["N"] * 4
    assert rows[(4, 260)]["last_wave_lanes"] == 1            # one live lane in the second wave
    assert rows[(4, 1028)]["last_trip_lanes"] == 1           # one live lane in the second trip
    assert rows[(1, 257)]["last_trip_lanes"] == 1
    assert some(lambda c, s: c.disp == "rows" and not c.disp_grad and s["shmem"] == 0 and s["waves"] >= 2)
    assert some(lambda c, s: c.disp == "rows" and not c.disp_grad and s["trips"] >= 2)
    # plane counts of the row-owned backward
    assert some(lambda c, s: c.disp == "rows" and c.disp_grad and c.shape[1] == 70 and c.shape[3] == 44 and s["waves"] == 1
                and s["final_steps"] == 2)
    assert some(lambda c, s: c.disp == "rows" and c.disp_grad and c.shape[1] == 300 and s["waves"] == 4 and s["final_steps"] == 2)
    assert some(lambda c, s: c.disp == "rows" and c.disp_grad and c.shape == (1, 4096, 1, 193) and s["waves"] == 4
                and s["shmem"] == 64 * 1024)
    assert {c.shape[2] for c in CASES if c.disp == "rows"} >= {1, 2, 5}
    # mixed forms, the misaligned case, the logits that move the softmax reference
    assert some(lambda c, s: c.disp == "rows" and c.mask == "dense")
    assert some(lambda c, s: c.disp == "dense" and c.mask == "rows")
    assert some(lambda c, s: c.disp == "plane" and c.mask == "rows" and c.disp_grad)
    assert some(lambda c, s: c.offset and (c.shape[2] * c.shape[3]) % 4 == 0 and s["px"] == 1)
    assert some(lambda c, s: c.spread == 6.0 and c.disp == "rows" and c.mask == "rows")
    # the PladeNet tail: pixel-linear entries, N = 300, N = 2
    plade = [BY_NAME[n] for n in PLADE_CASES]
    assert all(c.disp != "rows" for c in plade) and {300, 2} <= {c.shape[1] for c in plade} and min(c.shape[1] for c in plade) == 2
    assert {(L[c.name]["px"], L[c.name]["grid"]) for c in plade} >= {(4, 2), (1, 2), (4, 1), (1, 1)}
    assert set(NEW_SHAPES) <= set(BY_NAME) and all(BY_NAME[n].disp == "rows" and BY_NAME[n].disp_grad for n in NEW_ROW_SHAPES)
    assert max(math.prod(c.shape) for c in CASES) < 1 << 20


# =====================================================================================================================
# inputs, the oracle's runs and the allowances
# =====================================================================================================================
def _seed(case):
    return zlib.crc32(case.name.encode()) % 100000


def _levels(B, N, W, g):
    lv = torch.arange(N, dtype=torch.float32)[None, :, None, None] + 0.5 * (torch.rand(B, N, 1, 1, generator=g) - 0.5)
    return 300.0 * (W / 640.0) * (2.0 / 300.0) ** (lv / max(N - 1, 1))


def _raw_sigma_interior(shape, g):
    rs = (torch.randn(*shape, generator=g) * 3.0 - 1.0).clamp(SIGMA_LO, SIGMA_HI)   # the suite's raw_sigma, kept inside [-9, 6]
    return torch.where((rs - KINK).abs() < 1.5 * KINK_MARGIN, torch.full_like(rs, KINK + 2.0 * KINK_MARGIN), rs)


def make_inputs(case, channels=None):
    """CPU fp32 inputs of a case: conv outputs, the disparities in the case's own form ([B,N,1,1] / [B,N,H] / [B,N,H,W]; decreasing
    with the plane index, as the decoders space them), the mask in its form and the four upstream gradients.  ``channels``: the
    PladeNet tail's N - 1 logit channels (and a fifth upstream gradient, of dists)."""
    B, N, H, W = case.shape
    g = torch.Generator().manual_seed(_seed(case))
    inp = dict(rl=torch.randn(B, channels or N, H, W, generator=g) * (case.spread if channels is None else 1.5),
               rs=_raw_sigma_interior(case.shape, g))
    lv = _levels(B, N, W, g)
    if case.disp == "plane":
        inp["plane"] = lv.contiguous()
    elif case.disp == "rows":
        inp["plane"] = (lv[..., 0] * (1.0 + 0.2 * torch.rand(B, 1, H, generator=g))).contiguous()
    else:
        inp["plane"] = (lv * (1.0 + 0.2 * torch.rand(B, 1, H, W, generator=g))).contiguous()
    inp["mask"] = None
    if case.mask is not None and channels is None:
        m = (torch.rand(*((B, N, H) if case.mask == "rows" else (B, N, H, W)), generator=g) > 0.3).float()
        m[:, 0] = 1.0      # plane 0 stays in view: no pixel loses every plane
        inp["mask"] = m
    inp["ups"] = dict(gl=torch.randn(B, N, H, W, generator=g), gs=torch.randn(B, N, H, W, generator=g),
                      gd=torch.randn(B, 1, H, W, generator=g), gz=torch.randn(B, 1, H, W, generator=g) * 0.1)
    if channels is not None:
        inp["ups"]["gt"] = torch.randn(B, channels, H, W, generator=g) * 0.05
    return inp


def expand_form(t, form, shape):
    B, N, H, W = shape
    if form == "plane":
        return t.expand(B, N, H, W)
    if form == "rows":
        return t.unsqueeze(-1).expand(B, N, H, W)
    return t


def _grads(outs, ups, leaves):
    """The three backward passes of one graph: {combo: [gradient per leaf]} (a leaf no pass reaches gets zeros)."""
    res = {}
    for combo in COMBOS:
        sel = [(o, u) for kind, o, u in zip(("conv", "geom", "geom", "conv"), outs, ups)
               if o is not None and (combo == "all" or kind == combo)]
        gs = torch.autograd.grad([o for o, _ in sel], [l for l in leaves if l is not None], [u for _, u in sel],
                                 retain_graph=True, allow_unused=True)
        it = iter(gs)
        res[combo] = [None if l is None else (lambda x: torch.zeros_like(l) if x is None else x)(next(it)) for l in leaves]
    return res


def oracle_tail(case, inp, mix, dtype):
    """oracle.decoder_tail and its three backward passes in ``dtype`` on the CPU."""
    B, N, H, W = case.shape
    cast = lambda t: t.to(dtype).clone()  # noqa: E731
    rl = cast(inp["rl"]).requires_grad_(True)
    rs = cast(inp["rs"]).requires_grad_(True) if mix else None
    pl = cast(inp["plane"]).requires_grad_(True)
    m = torch.ones(B, N, H, W, dtype=dtype) if inp["mask"] is None else expand_form(cast(inp["mask"]), case.mask, case.shape)
    o = orc.decoder_tail(rl, rs, m, expand_form(pl, case.disp, case.shape), W, use_mixture_loss=mix)
    u = {k: cast(v) for k, v in inp["ups"].items()}
    gr = _grads([o["logits"], o["disp"], o["depth"], o.get("sigma")], [u["gl"], u["gd"], u["gz"], u["gs"]], [rl, rs, pl])
    res = dict(logits=o["logits"], disp=o["disp"], depth=o["depth"], pi=o.get("pi", o["probability"]), probability=o["probability"])
    if mix:
        res["sigma"] = o["sigma"]
    for combo in COMBOS:
        res["g_raw_logits/" + combo], g_rs, res["g_disp_layered/" + combo] = gr[combo]
        if mix:
            res["g_raw_sigma/" + combo] = g_rs
    return {k: v.detach() for k, v in res.items()}


def allowances(case, inp, mix, ref64):
    """An element's allowance: the sum of the absolute values of the terms the fp64 formula adds to produce it (module docstring)."""
    B, N, H, W = case.shape
    d = expand_form(inp["plane"].double(), case.disp, case.shape)
    m = torch.ones(B, N, H, W, dtype=torch.float64) if inp["mask"] is None else expand_form(inp["mask"].double(), case.mask, case.shape)
    u = {k: v.double() for k, v in inp["ups"].items()}
    P, disp = ref64["probability"], ref64["disp"]
    c = 0.1 * 0.58 * W
    a = {k: ref64[k].abs() for k in ("logits", "disp", "depth", "pi", "probability") + (("sigma",) if mix else ())}
    for combo in COMBOS:
        geom, conv = combo in ("geom", "all"), combo in ("conv", "all")
        gD = (u["gd"].abs() + u["gz"].abs() * c / disp ** 2) if geom else torch.zeros_like(disp)
        t = gD * (d.abs() + disp.abs()) * P
        a["g_raw_logits/" + combo] = ((u["gl"].abs() if conv else 0.0) + t) * m
        if mix:
            s = torch.sigmoid(inp["rs"].double())
            gate = (s >= 0.01) & (s <= 1.0)
            a["g_raw_sigma/" + combo] = torch.where(gate, ((u["gs"].abs() if conv else 0.0) + t / ref64["sigma"]) * s * (1.0 - s),
                                                    torch.zeros_like(s))
        per_pixel = gD * P
        a["g_disp_layered/" + combo] = (per_pixel if case.disp == "dense" else per_pixel.sum(3) if case.disp == "rows"
                                        else per_pixel.sum((2, 3), keepdim=True))
    return a


@functools.lru_cache(maxsize=2)
def reference(name, mix):
    """(inputs, fp64 run, allowances, E_ref per tensor, old rel_err of the fp32 oracle per tensor) of a case, computed once."""
    case = BY_NAME[name] if name in BY_NAME else BOUND_CASES[name]
    inp = make_inputs(case)
    ref64, ref32 = oracle_tail(case, inp, mix, torch.float64), oracle_tail(case, inp, mix, torch.float32)
    allow = allowances(case, inp, mix, ref64)
    e_ref = {k: term_report(ref32[k], ref64[k], allow[k]) for k in ref64}
    return inp, ref64, allow, e_ref, {k: rel_err(ref32[k], ref64[k]) for k in ref64}


def _record(family, case, mode, figures):
    REPORT["%s/%s/%s" % (family, case, mode)] = figures
    path = os.environ.get("PD_TAIL_PARITY_JSON")
    if path:
        kBlock, kWave = _kernel_constants()
        shapes = {c.name: dict(shape=list(c.shape), disp=c.disp, mask=c.mask, disp_grad=c.disp_grad, offset=c.offset,
                               **launch_shape(c, kBlock, kWave)) for c in CASES}
        with open(path, "w") as f:
            json.dump(dict(launch=shapes, figures=REPORT), f, indent=1, sort_keys=True)


@pytest.mark.parametrize("mix", [True, False], ids=["mix", "l1"])
@pytest.mark.parametrize("name", IDS)
def test_conditions(name, mix):
    """Kink-free and fair, proven on the oracle alone: the clamp decision is the same in fp32 and fp64, no pixel has every plane
    masked, the formula's exact zeros are exact in the fp32 oracle, and the oracle's fp32 run is within E_REF_CAP of its fp64 run on
    every tensor under the element-wise metric."""
    case = BY_NAME[name]
    inp, ref64, allow, e_ref, _ = reference(name, mix)
    rs = inp["rs"]
    assert float(rs.min()) >= SIGMA_LO and float(rs.max()) <= SIGMA_HI
    assert float((rs.double() - KINK).abs().min()) >= KINK_MARGIN
    s32, s64 = torch.sigmoid(rs), torch.sigmoid(rs.double())
    assert torch.equal(s32 >= 0.01, s64 >= 0.01) and bool((s32 < 1.0).all()) and float((1.0 - s64).min()) >= 2.4e-3
    assert bool((s64 < 0.01).any()) and bool((s64 > 0.5).any())       # both sides of the gate are there
    if inp["mask"] is not None:
        m = expand_form(inp["mask"], case.mask, case.shape)
        assert float(m.sum(1).min()) >= 1.0 and (case.shape[1] == 1 or bool((m == 0).any()))
    d = expand_form(inp["plane"], case.disp, case.shape)
    assert bool((d > 0).all()) and (case.shape[1] == 1 or bool((d[:, 1:] < d[:, :-1]).all()))
    for k, r in e_ref.items():
        print("%-24s E_ref %.3g  zeros %d" % (k, r["err"], r["zeros"]))
        assert r["zero_abs"] == 0.0, (k, r)
        assert r["err"] <= E_REF_CAP, (k, r)
    # pass "geom" leaves g_raw_logits purely gD (d_n - disp) P_n: planes of low probability are in it, and measured
    low = (ref64["probability"] < 1e-3) & (allow["g_raw_logits/geom"] > 0)
    assert case.shape[1] < 5 or math.prod(case.shape) < 2000 or bool(low.any())


# =====================================================================================================================
# the product
# =====================================================================================================================
def _offset_view(t):
    """``t`` on the device as a contiguous view that starts one element into its storage (tests/test_bf16_tails._bf16_leafable's
    construction, for any dtype): breaks the alignment of the four-pixel access."""
    buf = torch.empty(t.numel() + 1, device=DEV, dtype=t.dtype)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 8 != 0
    return v


def _device_operands(case, inp, dtype=torch.float32):
    """(raw_logits leaf, raw_sigma leaf, disparity leaf, disp_layered as the operator takes it, padding_mask as it takes it)"""
    from planedepth_amd import ops
    B, N, H, W = case.shape
    put = (lambda t: _offset_view(t.to(dtype))) if case.offset else (lambda t: t.to(DEV).to(dtype))
    rl, rs = put(inp["rl"]).requires_grad_(True), put(inp["rs"]).requires_grad_(True)
    leaf = inp["plane"].to(DEV).requires_grad_(case.disp_grad)
    dl = leaf.expand(-1, -1, H, W) if case.disp == "plane" else ops.row_view(leaf, W) if case.disp == "rows" else leaf
    pm = inp["mask"]
    if pm is not None:
        pm = ops.row_view(pm.to(DEV), W) if case.mask == "rows" else pm.to(DEV)
    return rl, rs, leaf, dl, pm


def product_tail(case, inp, mix):
    """ops.decoder_tail, layers() and the three backward passes, keyed as oracle_tail keys them."""
    from planedepth_amd import _capi as C
    from planedepth_amd import ops, planeform as PF, tails
    rl, rs, leaf, dl, pm = _device_operands(case, inp)
    flags, form, _, _, _ = tails._decoder_operands(rl, rs if mix else None, pm, dl, mix)
    assert form == dict(plane=PF.PER_PLANE, rows=PF.ROWS, dense=PF.DENSE)[case.disp]       # the form the table claims is taken
    assert bool(flags & C.PD_TAIL_MASK_ROWS) == (case.mask == "rows")
    assert (rl.data_ptr() % 16 != 0) == case.offset
    logits, sigma, disp, depth, layers = ops.decoder_tail(rl, rs if mix else None, pm, dl, use_mixture_loss=mix)
    pi, prob = layers(True, True)
    u = {k: v.to(DEV) for k, v in inp["ups"].items()}
    gr = _grads([logits, disp, depth, sigma], [u["gl"], u["gd"], u["gz"], u["gs"]],
                [rl, rs if mix else None, leaf if case.disp_grad else None])
    res = dict(logits=logits, disp=disp, depth=depth, pi=pi, probability=prob)
    if mix:
        res["sigma"] = sigma
    for combo in COMBOS:
        res["g_raw_logits/" + combo], g_rs, g_dl = gr[combo]
        if mix:
            res["g_raw_sigma/" + combo] = g_rs
        if case.disp_grad:
            res["g_disp_layered/" + combo] = g_dl
    return {k: v.detach().float().cpu() for k, v in res.items()}


def _hold_to_the_bar(family, case_name, mode, got, ref64, allow, e_ref, old):
    figures, bad = {}, []
    for k in sorted(got):
        assert tuple(got[k].shape) == tuple(ref64[k].shape), (k, tuple(got[k].shape), tuple(ref64[k].shape))
        assert bool(torch.isfinite(got[k]).all()), k
        r = term_report(got[k], ref64[k], allow[k])
        figures[k] = dict(err=r["err"], zero_abs=r["zero_abs"], e_ref=e_ref[k]["err"], rel_err=rel_err(got[k], ref64[k]),
                          rel_err_oracle_fp32=old[k])
        print("%-24s err %.3g  E_ref %.3g  rel_err %.3g  zeros %d  worst at %s" % (k, r["err"], e_ref[k]["err"], figures[k]["rel_err"],
                                                                                   r["zeros"], r["worst"]))
        if r["zero_abs"] != 0.0 or not (r["err"] <= 2.0 * e_ref[k]["err"] + TOL and r["err"] < TOL):
            bad.append((k, r, e_ref[k]["err"]))
    _record(family, case_name, mode, figures)
    assert not bad, bad
    return figures


def _hold_linearity(got, allow):
    for k in ("g_raw_logits", "g_raw_sigma", "g_disp_layered"):
        if k + "/all" not in got:
            continue
        r = term_report(got[k + "/geom"] + got[k + "/conv"], got[k + "/all"].double(), allow[k + "/all"])
        assert r["zero_abs"] == 0.0 and r["err"] <= LINEAR_TOL, (k, r)


@gpu
@pytest.mark.parametrize("mix", [True, False], ids=["mix", "l1"])
@pytest.mark.parametrize("name", IDS)
def test_decoder_tail_vs_fp64_per_element(name, mix):
    """Forward, layers() and the three backward passes of ops.decoder_tail in fp32 at every launch shape of the table.  A row-form
    case's g_disp_layered is [B,N,H] against the fp64 row sums."""
    case = BY_NAME[name]
    inp, ref64, allow, e_ref, old = reference(name, mix)
    got = product_tail(case, inp, mix)
    assert set(got) == {k for k in ref64 if case.disp_grad or not k.startswith("g_disp_layered")}
    if case.disp == "rows" and case.disp_grad:
        assert tuple(got["g_disp_layered/all"].shape) == case.shape[:3]
    _hold_to_the_bar("decoder", name, "mix" if mix else "l1", got, ref64, allow, e_ref, old)
    _hold_linearity(got, allow)


# =====================================================================================================================
# the equalities the suite asserts between routes, at the launch shapes it has not seen
# =====================================================================================================================
def _route_inputs(case, bf16):
    """Device inputs for tests/test_plane_geometry.tail_run: conv outputs (bf16: rounded), dense and row forms of the same map and
    mask, and upstream gradients whose logits / sigma parts are exact in bf16 (both routes then see the same gradient)."""
    from planedepth_amd import ops
    B, N, H, W = case.shape
    inp = make_inputs(case)
    st = BF if bf16 else torch.float32
    conv = (lambda t: _offset_view(t.to(st))) if case.offset else (lambda t: t.to(DEV).to(st))
    u = inp["ups"]
    gw = dict(l=u["gl"].to(BF).float().to(DEV), s=u["gs"].to(BF).float().to(DEV), d=u["gd"].to(DEV), z=u["gz"].to(DEV))
    dense_d = expand_form(inp["plane"], case.disp, case.shape).contiguous().to(DEV)
    dense_m = None if inp["mask"] is None else expand_form(inp["mask"], case.mask, case.shape).contiguous().to(DEV)
    view_d = ops.row_view(inp["plane"].to(DEV).requires_grad_(True), W) if case.disp == "rows" else None
    view_m = ops.row_view(inp["mask"].to(DEV), W) if case.mask == "rows" else dense_m
    return conv(inp["rl"]), conv(inp["rs"]), gw, dense_d, dense_m, view_d, view_m


@gpu
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("mix", [True, False], ids=["mix", "l1"])
@pytest.mark.parametrize("name", NEW_ROW_SHAPES + ["dense_row_mask"])
def test_row_form_has_the_dense_forms_bits_at_the_new_launch_shapes(name, mix, bf16):
    """tests/test_plane_geometry.py::test_row_form_has_the_dense_forms_bits' comparison where the row-owned backward takes two to
    four waves, a ragged last wave, several trips, or more planes than lanes."""
    from test_plane_geometry import tail_run
    case = BY_NAME[name]
    rl, rs, gw, dense_d, dense_m, view_d, view_m = _route_inputs(case, bf16)
    want = tail_run(rl, rs, dense_m, dense_d, mix, gw)
    got = tail_run(rl, rs, view_m, view_d if view_d is not None else dense_d, mix, gw)
    for k in ("logits", "sigma", "disp", "depth", "pi", "prob", "g_l", "g_s"):
        if want[k] is not None:
            assert got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]), k
    if view_d is not None:
        g_rows = view_d._pd_rows.grad
        assert tuple(g_rows.shape) == case.shape[:3]
        # per element against the fp64 sum of the dense route's own fp32 addends: W roundings of a running sum at the most
        dense = want["g_dl"].double()
        r = term_report(g_rows, dense.sum(-1), dense.abs().sum(-1))
        assert r["zero_abs"] == 0.0 and r["err"] <= case.shape[3] * 2.0 ** -24, r
    else:
        assert torch.equal(got["g_dl"], want["g_dl"])


@gpu
@pytest.mark.parametrize("mix", [True, False], ids=["mix", "l1"])
@pytest.mark.parametrize("name", NEW_SHAPES)
def test_bf16_equals_fp32_route_rounded_once_at_the_new_launch_shapes(name, mix):
    """tests/test_bf16_tails.py::test_decoder_tail_bf16_equals_fp32_route_rounded_once' comparison, in the row forms too."""
    from test_bf16_tails import _close_f32, _rounded_once
    from test_plane_geometry import tail_run
    case = BY_NAME[name]
    rl, rs, gw, dense_d, dense_m, view_d, view_m = _route_inputs(case, True)
    dl = view_d if view_d is not None else dense_d if case.disp == "dense" else \
        make_inputs(case)["plane"].to(DEV).requires_grad_(True).expand(-1, -1, *case.shape[2:])
    leaf_grad = lambda r: view_d._pd_rows.grad if view_d is not None else r["g_dl"] if case.disp == "dense" else dl._base.grad  # noqa: E731
    runs = []
    for widen in (False, True):
        if view_d is not None:
            view_d._pd_rows.grad = None
        if case.disp == "plane":
            dl._base.grad = None
        r = tail_run(rl.float() if widen else rl, rs.float() if widen else rs, view_m, dl, mix, gw)
        r["g_leaf"] = leaf_grad(r).clone()
        runs.append(r)
    got, want = runs
    assert want["logits"].dtype == torch.float32 and want["g_l"].dtype == torch.float32
    for k in ("disp", "depth", "prob"):
        _close_f32(k, got[k], want[k], 1e-6)
    assert got["logits"].dtype == BF
    if view_m is not None:
        assert torch.equal(got["logits"].float(), rl.float() * view_m)
    _rounded_once("g_raw_logits", got["g_l"], want["g_l"])
    if mix:
        _close_f32("pi", got["pi"], want["pi"], 1e-6)
        _rounded_once("sigma", got["sigma"], want["sigma"])
        assert float(got["sigma"].float().min()) >= 0.01
        _rounded_once("g_raw_sigma", got["g_s"], want["g_s"])
        closed = torch.sigmoid(rs.float()) < 0.01
        assert int(closed.sum()) > 0 and bool((got["g_s"][closed] == 0).all()) and bool((want["g_s"][closed] == 0).all())
    _close_f32("g_disp_layered", got["g_leaf"], want["g_leaf"], 1e-5)


@gpu
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("mix", [True, False], ids=["mix", "l1"])
@pytest.mark.parametrize("name", [n for n in NEW_SHAPES if n != "misaligned"])   # (that helper builds aligned inputs only)
def test_inference_tail_has_the_training_bits_at_the_new_launch_shapes(name, mix, bf16):
    """tests/test_infer_tail.py's whole check (disp / depth / stash bit for bit, confidence = max_n probability_n, the best plane)
    on the table's shapes and forms."""
    from test_infer_tail import _run_decoder
    case = BY_NAME[name]
    _run_decoder(case.shape, case.disp, case.mask, mix, bf16, seed=_seed(case))


# =====================================================================================================================
# exact edges
# =====================================================================================================================
@gpu
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_exact_edges(bf16):
    """Hand-placed raw_sigma at -12, 12 and 30 and masked planes: sigma exactly on its bounds with an exactly zero gradient behind
    the closed gate; logits, their gradient and the disparity gradient exactly 0 at a masked plane; an absurd finite disparity under
    a masked plane changes nothing."""
    from planedepth_amd import ops
    from test_bf16_tails import _raw_sigma
    B, N, H, W = shape = (2, 6, 3, 20)
    g = torch.Generator().manual_seed(11)
    st = BF if bf16 else torch.float32
    rl0 = (torch.randn(*shape, generator=g) * 2.5).to(DEV).to(st)
    rs0 = _raw_sigma(shape, g).to(DEV).to(st)
    pm = (torch.rand(*shape, generator=g) > 0.3).float()
    pm[:, 0] = 1.0
    pm = pm.to(DEV)
    d0 = (_levels(B, N, W, g) * (1.0 + 0.2 * torch.rand(B, 1, H, W, generator=g))).to(DEV)
    ups = [torch.randn(*shape, generator=g).to(DEV).to(st), torch.randn(*shape, generator=g).to(DEV).to(st),
           torch.randn(B, 1, H, W, generator=g).to(DEV), (torch.randn(B, 1, H, W, generator=g) * 0.1).to(DEV)]
    masked = pm == 0
    assert int(masked.sum()) > 0

    def run(dense):
        rl, rs = rl0.clone().requires_grad_(True), rs0.clone().requires_grad_(True)
        dl = dense.clone().requires_grad_(True)
        logits, sigma, disp, depth, layers = ops.decoder_tail(rl, rs, pm, dl)
        torch.autograd.backward([logits, sigma, disp, depth], ups)
        pi, prob = layers(True, True)
        return dict(logits=logits.detach(), sigma=sigma.detach(), disp=disp.detach(), depth=depth.detach(), pi=pi, prob=prob,
                    g_rl=rl.grad, g_rs=rs.grad, g_dl=dl.grad)

    got = run(d0)
    lo, hi, open12 = rs0.float() == -12.0, rs0.float() == 30.0, rs0.float() == 12.0
    assert int(lo.sum()) > 0 and int(hi.sum()) > 0 and int(open12.sum()) > 0
    assert bool((got["sigma"][lo] == torch.tensor(0.01, dtype=torch.float32).to(st)).all())
    assert bool((got["sigma"][hi] == 1.0).all())
    assert bool((got["g_rs"][lo] == 0).all()) and bool((got["g_rs"][hi] == 0).all())
    assert bool((got["g_rs"][open12] != 0).any())           # 12 is just inside: its gate is open
    assert bool((got["logits"][masked] == 0).all()) and bool((got["g_rl"][masked] == 0).all())
    assert bool((got["g_dl"][masked] == 0).all()) and bool((got["prob"][masked] == 0).all())
    assert bool((got["g_rl"][~masked] != 0).any()) and bool((got["g_dl"][~masked] != 0).any())
    absurd = torch.where(masked, torch.full_like(d0, 1e30), d0)
    again = run(absurd)
    for k in got:
        assert bool(torch.isfinite(again[k].float()).all()), k
        assert torch.equal(again[k], got[k]), k


# =====================================================================================================================
# the plane-count bound, through the C entry points
# =====================================================================================================================
BOUND_CASES = {c.name: c for c in [Case("bound_n16384", (1, 16384, 2, 2), "plane", None),
                                   Case("bound_rows_n4096", (1, 4096, 2, 2), "rows", None)]}


def _c_tail(case, inp, mix=True):
    """pd_decoder_tail_fwd / _layers / _bwd called directly on a case's tensors (fp32, no mask).  Returns (rc of the backward, its
    error text, results keyed as oracle_tail keys them for the joint pass)."""
    from planedepth_amd import _capi as C
    lib = C.load()
    B, N, H, W = case.shape
    flags = (C.PD_TAIL_MIXTURE if mix else 0) | (C.PD_TAIL_DISP_ROWS if case.disp == "rows" else 0)
    dev = torch.device(DEV, torch.cuda.current_device())
    new = lambda *s: torch.empty(*s, device=dev)  # noqa: E731
    rl, rs = inp["rl"].to(dev), inp["rs"].to(dev)
    plane = inp["plane"].to(dev).reshape((B, N, H) if case.disp == "rows" else (B, N)).contiguous()
    u = {k: v.to(dev) for k, v in inp["ups"].items()}
    sigma, disp, depth, stash = new(B, N, H, W), new(B, 1, H, W), new(B, 1, H, W), new(B, 2, H, W)
    pi, prob = new(B, N, H, W), new(B, N, H, W)
    g_rl, g_rs, g_dl = torch.empty_like(rl), torch.empty_like(rs), torch.empty_like(plane)
    ws = new(max(1, lib.pd_decoder_tail_bwd_workspace_floats(B, N, H, W)))
    st = C.stream_handle(dev)
    with C.on_device(dev):
        C.check(lib.pd_decoder_tail_fwd(B, N, H, W, flags, C.ptr(rl), C.ptr(rs), None, C.ptr(plane), None, C.ptr(sigma), C.ptr(disp),
                                        C.ptr(depth), C.ptr(stash), st), "pd_decoder_tail_fwd")
        C.check(lib.pd_decoder_tail_layers(B, N, H, W, flags, C.ptr(rl), C.ptr(rs), None, C.ptr(stash), C.ptr(pi), C.ptr(prob), st),
                "pd_decoder_tail_layers")
        rc = lib.pd_decoder_tail_bwd(B, N, H, W, flags, C.ptr(rl), C.ptr(rs), None, C.ptr(plane), C.ptr(stash), C.ptr(disp),
                                     C.ptr(u["gl"]), C.ptr(u["gs"]), C.ptr(u["gd"]), C.ptr(u["gz"]), C.ptr(g_rl), C.ptr(g_rs),
                                     C.ptr(g_dl), C.ptr(ws), st)
    text = lib.pd_last_error().decode(errors="replace") if rc else ""
    torch.cuda.synchronize()
    res = {"logits": rl, "sigma": sigma, "disp": disp, "depth": depth, "pi": pi, "probability": prob, "g_raw_logits/all": g_rl,
           "g_raw_sigma/all": g_rs, "g_disp_layered/all": g_dl.reshape(inp["plane"].shape)}
    return rc, text, {k: v.float().cpu() for k, v in res.items()}


@pytest.mark.parametrize("name", list(BOUND_CASES))
def test_conditions_of_the_bound_cases(name):
    _, _, _, e_ref, _ = reference(name, True)
    for k, r in e_ref.items():
        assert r["zero_abs"] == 0.0 and r["err"] <= E_REF_CAP, (k, r)


@gpu
@pytest.mark.parametrize("name", list(BOUND_CASES))
def test_plane_count_bound(name):
    """The largest plane count each backward form accepts runs and meets the bar (16384: the per-plane reduction's 64 KiB of LDS;
    4096 in the row-owned form); one plane more is refused by the entry point's argument check, with its text."""
    case = BOUND_CASES[name]
    inp, ref64, allow, e_ref, old = reference(name, True)
    rc, text, got = _c_tail(case, inp)
    assert rc == 0, (rc, text)
    _hold_to_the_bar("bound", name, "mix", got, {k: ref64[k] for k in got}, allow, e_ref, old)
    B, N, H, W = case.shape
    over = case._replace(name=name + "_plus_one", shape=(B, N + 1, H, W))
    rc, text, _ = _c_tail(over, make_inputs(over))
    assert rc != 0 and "too many planes" in text, (rc, text)


# =====================================================================================================================
# the PladeNet tail
# =====================================================================================================================
def _plade_run(case, inp, mix, dtype, device):
    """ops.plade_tail (device = the GPU, fp32) or oracle.plade_tail (the CPU, ``dtype``) with one joint backward pass."""
    B, N, H, W = case.shape
    fused = device != "cpu"
    put = (lambda t: _offset_view(t.to(dtype))) if (fused and case.offset) else (lambda t: t.to(device).to(dtype).clone())
    rl = put(inp["rl"]).requires_grad_(True)
    rs = put(inp["rs"]).requires_grad_(True) if mix else None
    leaf = inp["plane"].to(device).to(dtype).clone().requires_grad_(True)
    dl = expand_form(leaf, case.disp, case.shape)
    if fused:
        from planedepth_amd import ops
        logits, dists, sigma, disp, depth, layers = ops.plade_tail(rl, rs, dl, use_mixture_loss=mix)
        pi, prob = layers(True, True)
        o = dict(logits=logits, dists=dists, sigma=sigma, disp=disp, depth=depth, pi=pi, probability=prob)
    else:
        o = orc.plade_tail(rl, rs, dl, W, orc.camera_ray_norm(H, W, dtype), mix)
        o.setdefault("pi", o["probability"])
    u = {k: v.to(device).to(dtype) for k, v in inp["ups"].items()}
    outs, grads = [o["logits"], o["dists"], o["disp"], o["depth"]], [u["gl"], u["gt"], u["gd"], u["gz"]]
    if mix:
        outs.append(o["sigma"])
        grads.append(u["gs"])
    torch.autograd.backward(outs, grads)
    res = {k: o[k] for k in ("dists", "disp", "depth", "pi", "probability") + (("sigma",) if mix else ())}
    res.update(g_raw_logits=rl.grad, g_disp_layered=leaf.grad)
    if mix:
        res["g_raw_sigma"] = rs.grad
    return {k: v.detach().double().cpu() for k, v in res.items()}


def _plade_allowance(k, ref):
    """disp, depth, sigma: |ref|.  dists: max(|ref|, 0.1 of the tensor's largest entry).  Every other tensor has a plane axis: an
    element against max(|ref|, 0.1 max_n |ref| at its pixel) — alpha compositing (cumprod of 1 - alpha + 1e-10) is ill-conditioned
    per element, the fp32 oracle itself is 5e-3 .. 8e-2 off fp64 there without the floor."""
    a = ref.abs()
    if k in ("disp", "depth", "sigma"):
        return a
    if k == "dists":
        return torch.maximum(a, PLADE_FLOOR * a.max())
    return torch.maximum(a, PLADE_FLOOR * a.amax(1, keepdim=True))


@functools.lru_cache(maxsize=2)
def plade_reference(name, mix):
    case = BY_NAME[name]
    inp = make_inputs(case, channels=case.shape[1] - 1)
    ref64, ref32 = _plade_run(case, inp, mix, torch.float64, "cpu"), _plade_run(case, inp, mix, torch.float32, "cpu")
    allow = {k: _plade_allowance(k, v) for k, v in ref64.items()}
    return inp, ref64, allow, {k: term_report(ref32[k], ref64[k], allow[k]) for k in ref64}, {k: rel_err(ref32[k], ref64[k]) for k in ref64}


@pytest.mark.parametrize("mix", [True, False], ids=["mix", "l1"])
@pytest.mark.parametrize("name", PLADE_CASES)
def test_plade_conditions(name, mix):
    """The oracle's own fp32 run under the floored metric: every forward tensor within PLADE_E_REF_CAP at every plane count; the
    gradients from 49 planes on.  With two or three planes the per-pixel floor has nothing to stand on (one plane holds the
    probability, d_n - disp cancels in it and the others are small): the fp32 oracle is up to 4e-2 away there, and the three-way bar
    is as wide (profiles/tail_form_parity.md states E_ref per case)."""
    case = BY_NAME[name]
    _, ref64, _, e_ref, _ = plade_reference(name, mix)
    assert bool((ref64["dists"] > 0).all())
    for k, r in e_ref.items():
        print("%-24s E_ref %.3g" % (k, r["err"]))
        if not k.startswith("g_") or case.shape[1] >= 49:
            assert r["err"] <= PLADE_E_REF_CAP, (k, r)


@gpu
@pytest.mark.parametrize("mix", [True, False], ids=["mix", "l1"])
@pytest.mark.parametrize("name", PLADE_CASES)
def test_plade_tail_vs_fp64_per_element(name, mix):
    """The PladeNet tail at the pixel-linear launch shapes, N = 300 and N = 2, under the floored element-wise metric; the bar is
    the three-way one only: err <= 2 E_ref + 1e-4."""
    case = BY_NAME[name]
    inp, ref64, allow, e_ref, old = plade_reference(name, mix)
    got = _plade_run(case, inp, mix, torch.float32, DEV)
    figures, bad = {}, []
    for k in sorted(ref64):
        assert bool(torch.isfinite(got[k]).all()), k
        r = term_report(got[k], ref64[k], allow[k])
        figures[k] = dict(err=r["err"], e_ref=e_ref[k]["err"], rel_err=rel_err(got[k], ref64[k]), rel_err_oracle_fp32=old[k])
        print("%-24s err %.3g  E_ref %.3g  rel_err %.3g" % (k, r["err"], e_ref[k]["err"], figures[k]["rel_err"]))
        if not r["err"] <= 2.0 * e_ref[k]["err"] + TOL:
            bad.append((k, r, e_ref[k]["err"]))
    _record("plade", name, "mix" if mix else "l1", figures)
    assert not bad, bad
