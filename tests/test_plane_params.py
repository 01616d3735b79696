"""The kernels that MAKE the plane set and the pose algebra — pd_plane_geometry_fwd/_bwd, pd_homography_matrices_fwd/_bwd (three
modes), pd_plane_levels_fwd/_bwd, pd_crop_grid, pd_cat_flip — against a plain fp64 evaluation on the CPU, per ELEMENT, at every
launch shape their loops and grids can take.

Why.  One tensor of these kernels spans many decades (ground-plane disparities 3e-6 .. 3e2 px, g_distance ~ 1/d^2), so the tensor
norm ``rel_err`` lets the small rows and the far planes be wrong by 100 %; and the suite ran them at one shape each, which is one
trip of every ``+= kWave`` loop.  Here the sizes come from kBlock = 256 and kWave = 64 (``test_*_table_covers_*`` prove it without a
GPU), and every element is measured against itself or against its ALLOWANCE (cases.term_report: the sum of the absolute values of
the terms that make it).

Plane geometry / plane levels (fp32 kernels in the reference's operation order).  Reference: synthetic.decoder_plane_geometry in
fp64 on the fp32 inputs; yardstick: the same code in fp32 (E_ref).
    disp_rows, distance, norm   |got - ref| / |ref| <= 2 E_ref + FWD_TOL; an element whose reference is exactly 0 or 1 by
                                construction (norm of xy planes, the x component) has those bits
    mask_rows                   equal, no exclusions (no fp32 value lies between the double 1e-7 and 1e-7f)
    g_residual                  term_report under  xy: sum_y |g_y| |d disp / d level| + |g_dist| |d distance / d level|
                                                   xz: sum_y |g_y disp_y| / h * span / (nx - 1) + |g_dist| inv span / (nx - 1)
                                err <= 2 E_ref + BWD_TOL, in three passes (rows only, distance only, both) that add up.
Homography matrices (fp64 inside, rounded once).  Reference: the stock torch chain in fp64 (ops.homography_matrices).
    every element               |got - ref| <= 2^-23 |ref| + 1e-12 A:  one fp32 ulp plus fp64 evaluation noise; A = the largest
                                |entry| of the element's matrix / vector, for g_T the sum over planes of |per-plane contribution|,
                                for g_distance / g_norm |ref|.  test_homography_conditions_cpu evaluates the chain in two orders
                                (torch.inverse, adjugate / determinant) and holds their difference to 1e-12 A.
    stereo-row mask             the fp64 oracle's mask, away from its own knife edges (<= 1 % of the rows, from the reference alone)

PD_PLANE_PARAM_PARITY_JSON=<file> writes every figure: the source of profiles/plane_param_parity.md."""
import functools
import itertools
import json
import math
import os
import re
import types
import zlib
from typing import NamedTuple

import numpy as np
import pytest
import torch

from cases import term_report
from conftest import GOLDEN
from oracle import planedepth_oracle as orc
from planedepth_amd import _capi as C
from planedepth_amd import synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
gpu = pytest.mark.gpu
F64 = torch.float64

# --- bars.  None of them is taken from a product run.
# Forward of the fp32 kernels: a chain of at most eight rounded operations (8 * 2^-24 = 4.8e-7) plus powf, whose argument error is
# amplified by |ln(disp_min / disp_max)| ~ 5 (another ~3e-7): 1e-6, about sixteen half-ulps.
FWD_TOL = 1e-6
# Backward of the fp32 kernels: it reads the STORED fp32 disparities, so it inherits the forward's allowance on them (1e-6), and adds
# its own roundings of terms the allowance bounds: the wave's sum (at most 3 adds per lane and 6 butterfly steps), the products by disp,
# ln(base) (logf: 1 ulp) and the two quotients — under sixteen half-ulps, 1e-6.  Together 2e-6.
BWD_TOL = 2e-6
# g(rows) + g(distance) against g(both): linear in the upstream gradients, so they differ by roundings of terms the joint allowance
# bounds — the subtraction and three products / quotients on each of the three results, the final add: under sixteen, 1e-6.
LINEAR_TOL = 1e-6
# The fp32 restatement's own error per element over the tables below (measured on the CPU, profiles/plane_param_parity.md: forward
# <= 4.4e-7, g_residual and g_levels <= 5.0e-7 of their allowances): the caps leave a factor of 2, so that 2 E_ref + tol stays below 4e-6.
E_REF_CAP = 1e-6
E_REF_CAP_BWD = 1e-6
ULP = 2.0 ** -23          # one fp32 ulp, relative
NOISE = 1e-12             # fp64 evaluation noise, in units of A
MASK_EXCLUDED_CAP = 0.01  # share of stereo-row mask entries on the fp64 reference's own knife edges
COMBOS = ("rows", "dist", "both")
CFG = dict(disp_min=2.0, disp_max=300.0, xz_min=0.1852, xz_max=0.3704)
REPORT = {}


def _kernel_constants():
    text = open(os.path.join(ROOT, "planedepth_amd", "csrc", "pd_common.h")).read()
    return tuple(int(re.search(r"constexpr int %s = (\d+);" % k, text).group(1)) for k in ("kBlock", "kWave"))


def ceil_div(a, b):
    return -(-a // b)


def _seed(name):
    return zlib.crc32(name.encode()) % 100000


def _record(key, figures):
    REPORT[key] = figures
    path = os.environ.get("PD_PLANE_PARAM_PARITY_JSON")
    if path:
        with open(path, "w") as f:
            json.dump(REPORT, f, indent=1, sort_keys=True)


def rel_report(got, ref64):
    """Per-element relative error where the reference is not 0; ``exact``: the other elements have the reference's bits."""
    g, r = got.detach().double().cpu(), ref64.detach().double().cpu()
    assert g.shape == r.shape, (tuple(g.shape), tuple(r.shape))
    live = r != 0
    q = torch.where(live, (g - r).abs() / r.abs().clamp_min(1e-300), torch.zeros_like(r))
    q = torch.where(torch.isnan(q), torch.full_like(q, float("inf")), q)
    return dict(err=float(q.max()) if q.numel() else 0.0, exact=bool((g[~live] == 0).all()), zeros=int((~live).sum()))


def ulp_report(got, ref64, A):
    """|got - ref| against ULP |ref| + NOISE A per element: the worst element in units of its allowance, and in fp32 ulps of itself."""
    g, r, a = got.detach().double().cpu(), ref64.detach().double().cpu(), A.detach().double().cpu().expand_as(ref64)
    assert g.shape == r.shape, (tuple(g.shape), tuple(r.shape))
    diff = (g - r).abs()
    diff = torch.where(torch.isnan(diff), torch.full_like(diff, float("inf")), diff)
    allow = ULP * r.abs() + NOISE * a
    over = torch.where(allow > 0, diff / allow.clamp_min(1e-300), torch.where(diff > 0, torch.full_like(diff, float("inf")), diff))
    ulps = torch.where(r != 0, diff / (ULP * r.abs()).clamp_min(1e-300), torch.zeros_like(diff))
    return dict(worst=float(over.max()) if over.numel() else 0.0, ulps=float(ulps.max()) if ulps.numel() else 0.0)


# =====================================================================================================================
# 1. plane geometry
# =====================================================================================================================
class GeoCase(NamedTuple):
    name: str
    B: int
    nl: int            # no_levels (xy planes)
    nx: int            # xz_levels (ground planes)
    H: int
    W: int
    grid: str          # resize | crop (horizon inside) | above | below (the crop lies wholly above / below the horizon)
    edge_rows: bool = False   # hand-written y rows around the mask's threshold


GEO_CASES = [
    GeoCase("h1", 1, 2, 2, 1, 2, "resize"),
    GeoCase("h7_row_at_zero", 2, 3, 2, 7, 9, "resize"),              # the odd H puts a grid row at y = 0 (fp32 linspace: -3e-8)
    GeoCase("fixture_shape", 2, 4, 3, 64, 64, "crop"),
    GeoCase("h65_edge_rows", 2, 3, 2, 65, 33, "crop", edge_rows=True),
    GeoCase("xy_only", 3, 5, 0, 7, 9, "resize"),
    GeoCase("n70_h130", 2, 60, 10, 130, 66, "crop"),
    GeoCase("headline_h192", 1, 49, 14, 192, 40, "crop"),
    GeoCase("above_horizon", 1, 49, 14, 63, 24, "above"),            # everything masked; the gradient still flows to h
    GeoCase("below_horizon", 1, 4, 3, 63, 24, "below"),
]
GEO = {c.name: c for c in GEO_CASES}
GEO_IDS = [c.name for c in GEO_CASES]
ONE_E7 = float(np.float32(1e-7))
EDGE_Y = [0.0, -0.0, ONE_E7, float(np.nextafter(np.float32(1e-7), np.float32(0.0))), 1e-6, -1e-3]   # rows 1..6 of image 0
EDGE_MASK = [0.0, 0.0, 1.0, 0.0, 1.0, 0.0]


def test_geometry_table_covers_the_launch_arithmetic():
    """plane_geometry_fwd_kernel: one thread per (b, n, y), kBlock per block; plane_geometry_bwd_kernel: one wave per (b, n),
    kBlock / kWave of them per block, lanes striding the rows by kWave."""
    kBlock, kWave = _kernel_constants()
    assert (kBlock, kWave) == (256, 64)
    assert len(GEO) == len(GEO_CASES)
    trips = {c.H: (ceil_div(c.H, kWave), c.H % kWave) for c in GEO_CASES}
    assert {1, 63, 64, 65, 130, 192} <= set(trips)
    assert trips[1] == (1, 1) and trips[63] == (1, 63) and trips[64] == (1, 0)            # one trip: one lane, ragged, exact
    assert trips[65] == (2, 1) and trips[130] == (3, 2) and trips[192] == (3, 0)          # ragged two, two-plus, three exact
    total = [c.B * (c.nl + c.nx) * c.H for c in GEO_CASES]
    assert any(t < kBlock for t in total) and any(t > kBlock and t % kBlock for t in total)
    waves = [c.B * (c.nl + c.nx) for c in GEO_CASES]
    per_block = kBlock // kWave
    assert any(w % per_block == 0 for w in waves) and any(w % per_block for w in waves) and any(w > per_block for w in waves)
    assert any(c.nl + c.nx > kWave for c in GEO_CASES)
    assert {0, 2, 14} <= {c.nx for c in GEO_CASES}
    assert {"resize", "crop", "above", "below"} <= {c.grid for c in GEO_CASES}
    assert any(c.edge_rows and c.nx and c.H > len(EDGE_Y) + 1 for c in GEO_CASES)
    assert any(c.grid == "resize" and c.H % 2 and c.H > 1 and c.nx for c in GEO_CASES)
    assert [(c.B, c.nl, c.nx, c.H, c.W) for c in GEO_CASES] == [
        (1, 2, 2, 1, 2), (2, 3, 2, 7, 9), (2, 4, 3, 64, 64), (2, 3, 2, 65, 33), (3, 5, 0, 7, 9), (2, 60, 10, 130, 66),
        (1, 49, 14, 192, 40), (1, 49, 14, 63, 24), (1, 4, 3, 63, 24)]
    assert max(t for t in total) < 1 << 16


def geo_crop(case, b):
    """(full_h, full_w, h0, w0) of image b: a different resize factor and window per image."""
    H, W = case.H, case.W
    if case.grid == "resize":
        return H, W, 0, 0
    full_h, full_w = 2 * H + 11 + 6 * b, 3 * W + 5 + 4 * b
    mid = (full_h - 1) // 2                       # linspace(-1, 1, full_h) changes sign between rows mid and mid + 1 (or is 0 at mid)
    h0 = {"crop": mid - H // 3 - b, "above": mid - H - 1 - b, "below": mid + 2 + b}[case.grid]
    assert 0 <= h0 and h0 + H <= full_h
    return full_h, full_w, h0, 3 + 2 * b


def geo_inputs(case):
    g = torch.Generator().manual_seed(_seed("geo/" + case.name))
    N = case.nl + case.nx
    grid = torch.stack([synthetic.crop_grid(case.H, case.W, *geo_crop(case, b)) for b in range(case.B)], 0)
    if case.edge_rows:
        grid[0, 1, 1:1 + len(EDGE_Y), :] = torch.tensor(EDGE_Y, dtype=torch.float32)[:, None]
    return dict(grid=grid, residual=torch.rand(case.B, N, generator=g) - 0.5,
                g_rows=torch.randn(case.B, N, case.H, generator=g), g_dist=torch.randn(case.B, N, generator=g))


def geo_kw(case):
    return dict(no_levels=case.nl, xz_levels=case.nx, **CFG)


def geo_restatement(case, inp, dtype, residual=True):
    """synthetic.decoder_plane_geometry(rows=True) in ``dtype`` on the fp32 inputs, and its three backward passes."""
    N = case.nl + case.nx
    res = (inp["residual"].to(dtype).clone().requires_grad_(True) if residual else torch.zeros(case.B, N, dtype=dtype))
    o = synthetic.decoder_plane_geometry(inp["grid"].to(dtype), res, rows=True, **geo_kw(case))
    rows = o["disp_layered"][..., 0]
    out = dict(disp_rows=rows, mask_rows=o["padding_mask"][..., 0], distance=o["distance"], norm=o["norm"])
    if residual:
        ups = dict(rows=([rows], [inp["g_rows"].to(dtype)]), dist=([o["distance"]], [inp["g_dist"].to(dtype)]))
        ups["both"] = (ups["rows"][0] + ups["dist"][0], ups["rows"][1] + ups["dist"][1])
        for combo in COMBOS:
            out["g_residual/" + combo], = torch.autograd.grad(ups[combo][0], [res], ups[combo][1], retain_graph=True)
    return {k: v.detach() for k, v in out.items()}


def geo_allowance(case, inp, ref64):
    """The absolute terms of g_residual from the fp64 tensors (module docstring)."""
    nl, nx = case.nl, case.nx
    d, dist = ref64["disp_rows"], ref64["distance"]
    gr, gd = inp["g_rows"].double().abs(), inp["g_dist"].double().abs()
    ln = abs(math.log(CFG["disp_min"] / CFG["disp_max"])) / (nl - 1)
    a_rows = (gr * d).sum(-1) * ln                 # xy: |d disp / d level| = disp |ln base| / (nl - 1) on every row
    a_dist = gd * dist * ln                        #     |d distance / d level| = distance |ln base| / (nl - 1)
    if nx:
        span = (CFG["xz_max"] - CFG["xz_min"]) / (nx - 1)
        h = CFG["xz_min"] + span * (torch.arange(nx, dtype=F64)[None] + inp["residual"].double()[:, nl:])
        a_rows[:, nl:] = (gr[:, nl:] * d[:, nl:]).sum(-1) / h * span
        a_dist[:, nl:] = gd[:, nl:] * (dist[:, nl:] / h) * span
    return dict(rows=a_rows, dist=a_dist, both=a_rows + a_dist)


@functools.lru_cache(maxsize=None)
def geo_reference(name, residual=True):
    case = GEO[name]
    inp = geo_inputs(case)
    ref64, ref32 = geo_restatement(case, inp, F64, residual), geo_restatement(case, inp, torch.float32, residual)
    allow = geo_allowance(case, inp, ref64) if residual else {}
    e_ref = {k: rel_report(ref32[k], ref64[k])["err"] for k in ("disp_rows", "distance", "norm")}
    for combo in allow:
        e_ref["g_residual/" + combo] = term_report(ref32["g_residual/" + combo], ref64["g_residual/" + combo], allow[combo])["err"]
    return inp, ref64, ref32, allow, e_ref


def check_geo_forward(tag, got, ref64, e_ref, case):
    figures = {}
    for k in ("disp_rows", "distance", "norm"):
        r = rel_report(got[k], ref64[k])
        figures[k] = dict(err=r["err"], e_ref=e_ref[k])
        print(tag, k, "err %.2e E_ref %.2e" % (r["err"], e_ref[k]))
        assert r["exact"], (tag, k)
        assert r["err"] <= 2.0 * e_ref[k] + FWD_TOL, (tag, k, r["err"], e_ref[k])
    norm = got["norm"].detach().cpu()
    assert bool((norm[..., 0] == 0).all())                                              # no plane of this set has an x component
    assert bool((norm[:, :case.nl, 1] == 0).all()) and bool((norm[:, :case.nl, 2] == 1).all())
    assert torch.equal(got["mask_rows"].detach().cpu().double(), ref64["mask_rows"]), (tag, "mask_rows")
    return figures


def check_geo_backward(tag, got, ref64, allow, e_ref):
    figures = {}
    for combo in COMBOS:
        k = "g_residual/" + combo
        r = term_report(got[k], ref64[k], allow[combo])
        figures[k] = dict(err=r["err"], e_ref=e_ref[k], worst=r["worst"])
        print(tag, k, "err %.2e E_ref %.2e at %s" % (r["err"], e_ref[k], r["worst"]))
        assert r["zero_abs"] == 0.0, (tag, k)
        assert r["err"] <= 2.0 * e_ref[k] + BWD_TOL, (tag, k, r["err"], e_ref[k], r["worst"])
    lin = term_report(got["g_residual/rows"].double() + got["g_residual/dist"].double(), got["g_residual/both"], allow["both"])
    figures["linear"] = lin["err"]
    assert lin["err"] <= LINEAR_TOL and lin["zero_abs"] == 0.0, (tag, "rows + dist != both", lin)
    return figures


def masked_rows(case, inp):
    """(rows below the horizon, rows above it, rows at y = 0: closer to it than the mask's threshold) of the y channel's first
    column, summed over the images."""
    y = inp["grid"][:, 1, :, 0]
    return int((y >= ONE_E7).sum()), int((y <= -ONE_E7).sum()), int((y.abs() < ONE_E7).sum())


@pytest.mark.parametrize("name", GEO_IDS)
def test_geometry_conditions_cpu(name):
    """The fp32 restatement meets the bars, E_ref stays under its caps, and the cases have the rows they claim."""
    case = GEO[name]
    inp, ref64, ref32, allow, e_ref = geo_reference(name)
    figures = check_geo_forward("restatement/" + name, ref32, ref64, e_ref, case)
    figures.update(check_geo_backward("restatement/" + name, ref32, ref64, allow, e_ref))
    _record("plane_geometry/%s/restatement" % name, figures)
    assert all(e_ref[k] <= E_REF_CAP for k in ("disp_rows", "distance", "norm")), e_ref
    assert all(e_ref["g_residual/" + c] <= E_REF_CAP_BWD for c in COMBOS), e_ref
    assert bool((allow["both"] > 0).all())                    # every plane's gradient has terms: nothing passes by being 0
    y = inp["grid"][:, 1]
    assert bool((y == y[..., :1]).all())                      # the kernel's contract: the y channel is constant along x
    below, above, at_zero = masked_rows(case, inp)
    want = {"crop": below > 0 and above > 0, "above": below == 0 and at_zero == 0 and above == case.B * case.H,
            "below": above == 0 and at_zero == 0 and below == case.B * case.H, "resize": True}[case.grid]
    assert want, (below, above, at_zero)
    if case.grid == "resize" and case.H % 2 and case.H > 1:
        assert at_zero == case.B and bool((ref64["mask_rows"][:, case.nl:, case.H // 2] == 0).all())
    if case.nx:
        m = ref64["mask_rows"][:, case.nl:]
        assert torch.equal(m, (y[:, None, :, 0] >= ONE_E7).double().expand_as(m))
        if case.grid == "above":       # every ground row is masked and clamped, and h still takes a gradient from it
            assert float(m.sum()) == 0.0 and bool((ref64["g_residual/rows"][:, case.nl:].abs() > 0).all())
    if case.edge_rows:
        rows = slice(1, 1 + len(EDGE_Y))
        assert ref64["mask_rows"][0, case.nl:, rows].tolist() == [EDGE_MASK] * case.nx
        assert ref32["mask_rows"][0, case.nl:, rows].tolist() == [EDGE_MASK] * case.nx
        d = ref32["disp_rows"][0, case.nl:, rows]
        clamped = [i for i, m in enumerate(EDGE_MASK) if m == 0.0]
        assert torch.equal(d[:, clamped], d[:, 2:3].expand(-1, len(clamped)))      # a masked row has the disparity of y = 1e-7f


@pytest.mark.parametrize("residual", [True, False], ids=["res", "nores"])
def test_restatement_matches_the_reference_fixture_per_element(residual):
    """synthetic.decoder_plane_geometry(rows=True) in fp32 against every tensor the reference decoder wrote into
    tests/golden/plane_geometry.npz, per element: two fp32 evaluations of one formula, each within E_REF_CAP of the exact value."""
    z = np.load(os.path.join(GOLDEN, "plane_geometry.npz"))
    meta = json.loads(str(z["meta"]))
    for tag, kw in meta["cases"].items():
        if bool(kw["plane_residual"]) != residual:
            continue
        grid = torch.from_numpy(z["%s/grid" % kw["inputs_of"]])
        N = kw["no_levels"] + kw["xz_levels"]
        res = torch.from_numpy(z[tag + "/residual"]) if residual else torch.zeros(kw["B"], N)
        o = synthetic.decoder_plane_geometry(grid, res, no_levels=kw["no_levels"], xz_levels=kw["xz_levels"], rows=True, **meta["cfg"])
        got = dict(disp_rows=o["disp_layered"][..., 0], distance=o["distance"], norm=o["norm"])
        for k, v in got.items():
            r = rel_report(v, torch.from_numpy(z["%s/%s" % (tag, k)]).double())
            print(tag, k, r["err"])
            assert r["exact"] and r["err"] <= 2.0 * E_REF_CAP, (tag, k, r)
        assert torch.equal(o["padding_mask"][..., 0], torch.from_numpy(z[tag + "/mask_rows"])), tag


def geo_product(case, inp, residual=True):
    from planedepth_amd import ops
    res = inp["residual"].to(DEV).requires_grad_(True) if residual else None
    dl, pm, distance, norm = ops.plane_geometry(inp["grid"].to(DEV), res, **geo_kw(case))
    rows = dl._pd_rows
    N = case.nl + case.nx
    assert tuple(dl.shape) == tuple(pm.shape) == (case.B, N, case.H, case.W) and tuple(rows.shape) == (case.B, N, case.H)
    out = dict(disp_rows=rows, mask_rows=pm._pd_rows, distance=distance, norm=norm)
    if residual:
        ups = dict(rows=([rows], [inp["g_rows"].to(DEV)]), dist=([distance], [inp["g_dist"].to(DEV)]))
        ups["both"] = (ups["rows"][0] + ups["dist"][0], ups["rows"][1] + ups["dist"][1])
        for combo in COMBOS:
            out["g_residual/" + combo], = torch.autograd.grad(ups[combo][0], [res], ups[combo][1], retain_graph=True)
    return {k: v.detach().cpu() for k, v in out.items()}


@gpu
@pytest.mark.parametrize("name", GEO_IDS)
def test_plane_geometry_per_element(name):
    case = GEO[name]
    inp, ref64, _, allow, e_ref = geo_reference(name)
    got = geo_product(case, inp)
    figures = check_geo_forward(name, got, ref64, e_ref, case)
    figures.update(check_geo_backward(name, got, ref64, allow, e_ref))
    _record("plane_geometry/%s/product" % name, figures)
    again = geo_product(case, inp)
    for k in got:
        assert torch.equal(got[k].view(torch.int32), again[k].view(torch.int32)), (name, k)       # two runs, the same bits
    if case.edge_rows:
        rows = slice(1, 1 + len(EDGE_Y))
        assert got["mask_rows"][0, case.nl:, rows].tolist() == [EDGE_MASK] * case.nx
        d = got["disp_rows"][0, case.nl:, rows]
        clamped = [i for i, m in enumerate(EDGE_MASK) if m == 0.0]
        assert torch.equal(d[:, clamped], d[:, 2:3].expand(-1, len(clamped)))


@gpu
@pytest.mark.parametrize("name", GEO_IDS)
def test_plane_geometry_forward_without_residual(name):
    case = GEO[name]
    inp, ref64, _, _, e_ref = geo_reference(name, False)
    got = geo_product(case, inp, residual=False)
    _record("plane_geometry/%s/product_nores" % name, check_geo_forward(name + "/nores", got, ref64, e_ref, case))


@gpu
@pytest.mark.parametrize("name", GEO_IDS)
def test_xy_only_geometry_has_the_plane_levels_bits(name):
    """xz_levels == 0 is what pd_plane_levels gives, on every row, at the new shapes."""
    from planedepth_amd import ops
    case = GEO[name]
    inp = geo_inputs(case)
    res = inp["residual"][:, :case.nl].contiguous().to(DEV)
    dl, pm, distance, norm = ops.plane_geometry(inp["grid"].to(DEV), res, no_levels=case.nl, xz_levels=0, **CFG)
    d0, dist0 = ops.plane_disparities(torch.arange(case.nl, device=DEV, dtype=torch.float32)[None] + res, CFG["disp_min"],
                                      CFG["disp_max"], case.W)
    assert torch.equal(dl._pd_rows, d0.reshape(case.B, case.nl, 1).expand(-1, -1, case.H))
    assert torch.equal(distance, dist0) and bool((pm._pd_rows == 1).all())


# =====================================================================================================================
# 2. homography matrices
# =====================================================================================================================
class HCase(NamedTuple):
    name: str
    mode: str          # planes | uniform | stereo_rows
    B: int
    N: int
    rows: int = 0


H_CASES = [
    HCase("planes_n1", "planes", 1, 1), HCase("planes_n11", "planes", 3, 11), HCase("planes_n63", "planes", 1, 63),
    HCase("planes_n64", "planes", 3, 64), HCase("planes_n65", "planes", 1, 65), HCase("planes_n130", "planes", 3, 130),
    HCase("uniform_n1", "uniform", 1, 1), HCase("uniform_n2", "uniform", 3, 2), HCase("uniform_n5", "uniform", 1, 5),
    HCase("uniform_n70", "uniform", 3, 70),
    HCase("stereo_n1_r1", "stereo_rows", 1, 1, 1), HCase("stereo_n5_r63", "stereo_rows", 2, 5, 63),
    HCase("stereo_n5_r64", "stereo_rows", 1, 5, 64), HCase("stereo_n3_r65", "stereo_rows", 2, 3, 65),
    HCase("stereo_n70_r130", "stereo_rows", 1, 70, 130), HCase("stereo_n7_r192", "stereo_rows", 2, 7, 192),
]
HC = {c.name: c for c in H_CASES}
H_IDS = [c.name for c in H_CASES]
MODES = {"planes": C.PD_HMAT_PLANES, "uniform": C.PD_HMAT_UNIFORM, "stereo_rows": C.PD_HMAT_STEREO_ROWS}
HW_PLANES = (37, 120)      # the image the intrinsics of the planes / uniform cases belong to
W_STEREO = 40
D_MIN, D_MAX = 0.05, 50.0


def test_homography_table_covers_the_launch_arithmetic():
    """homography_matrices_fwd/bwd_kernel: one wave per image, lanes striding max(N, NH) / NH slots by kWave (NH = 4 in uniform
    mode); stereo_rows_fwd/bwd_kernel: one wave per (plane, image), lanes striding the rows by kWave."""
    kBlock, kWave = _kernel_constants()
    assert (kBlock, kWave) == (256, 64) and len(HC) == len(H_CASES)
    by = lambda mode: [c for c in H_CASES if c.mode == mode]  # noqa: E731
    assert {c.N for c in by("planes")} == {1, 11, kWave - 1, kWave, kWave + 1, 2 * kWave + 2}
    assert {c.B for c in by("planes")} == {1, 3}
    assert {c.N for c in by("uniform")} == {1, 2, 5, kWave + 6} and {c.B for c in by("uniform")} == {1, 3}
    assert sum(c.N < 4 for c in by("uniform")) >= 2            # fewer planes than homography slots
    assert {(c.N, c.rows) for c in by("stereo_rows")} == {(1, 1), (5, kWave - 1), (5, kWave), (3, kWave + 1),
                                                          (kWave + 6, 2 * kWave + 2), (7, 3 * kWave)}
    assert {c.B for c in by("stereo_rows")} == {1, 2}
    assert max(c.B * c.N * max(c.rows, 9) for c in H_CASES) < 1 << 16


def f8_pose(B, seed, rot):
    """A pose as Trainer.predict_poses leaves it for a novel frame without COLMAP: a rotation conjugated by a crop matrix, ZERO
    translation, Rt[3,3] = 0."""
    g = torch.Generator().manual_seed(seed)
    R = synthetic.small_pose(g, B, rot=rot, trans=0.0)[:, :3, :3]
    Rc = torch.eye(3)[None].repeat(B, 1, 1)
    Rc[:, 0, 2] = torch.randn(B, generator=g) * 0.05
    Rc[:, 1, 2] = torch.randn(B, generator=g) * 0.05
    Rc[:, 2, 2] = 0.7 + 0.3 * torch.rand(B, generator=g)
    Rt = torch.zeros(B, 4, 4)
    Rt[:, :3, :3] = Rc @ R @ torch.inverse(Rc)
    return Rt


def hmat_inputs(case):
    """fp32 CPU inputs: distances spread log-uniformly (stratified, shuffled) over 0.05 .. 50, so that g_distance ~ 1/d^2 covers
    decades inside one tensor."""
    B, N = case.B, case.N
    g = torch.Generator().manual_seed(_seed("hmat/" + case.name))
    u = torch.stack([(torch.randperm(N, generator=g) + torch.rand(N, generator=g)) / N for _ in range(B)], 0)
    distance = D_MIN * (D_MAX / D_MIN) ** u
    norm = torch.nn.functional.normalize(torch.randn(B, N, 3, generator=g) * 0.4 + torch.tensor([0.0, 0.0, 1.0]), dim=-1)
    if case.mode == "stereo_rows":
        H = case.rows
        K, inv_K = synthetic.intrinsics(B, H, W_STEREO)
        T = synthetic.small_pose(None, B, stereo=True)
        norm[..., 0] = 0.0
        # the ground-like half: [0, 1, t], facing away above the row y0 = k + 0.37 somewhere in the middle 60 % of the image
        y0 = torch.floor((0.2 + 0.6 * torch.rand(B, N - N // 2, generator=g)) * H) + 0.37
        norm[:, N // 2:, 1] = 1.0
        norm[:, N // 2:, 2] = (H / 2.0 - y0) / (1.92 * H)
        norm = torch.nn.functional.normalize(norm, dim=-1)
        g_first = torch.randn(B, N, H, generator=g)
    else:
        K, inv_K = synthetic.intrinsics(B, *HW_PLANES)
        T = f8_pose(B, _seed(case.name), 0.05) if case.mode == "uniform" else synthetic.small_pose(g, B, rot=0.05, trans=0.01)
        g_first = torch.randn(B, 4 if case.mode == "uniform" else N, 3, 3, generator=g)
    return dict(distance=distance, norm=norm.contiguous(), T=T, K=K, inv_K=inv_K, g_first=g_first,
                g_H=torch.randn(B, N, 3, 3, generator=g))


def adjugate_inverse(A):
    """The second evaluation order: adjugate / determinant."""
    r0, r1, r2 = A[..., 0, :], A[..., 1, :], A[..., 2, :]
    c0, c1, c2 = torch.linalg.cross(r1, r2), torch.linalg.cross(r2, r0), torch.linalg.cross(r0, r1)
    return torch.stack([c0, c1, c2], -1) / (r0 * c0).sum(-1)[..., None, None]


def chain_planes(d, n, Tx, K, Ki, stock):
    """layers.py:206-219, 223 for a per-plane pose Tx [B,N,4,4]: (H_t2s [B,N,3,3], Rn [B,N,3]).  ``stock``: the package's stock torch
    statement of it (torch.inverse); otherwise the same products with the adjugate inverse."""
    B, N = d.shape
    if stock:
        from planedepth_amd import ops
        ex = lambda M: M[:, None].expand(-1, N, -1, -1).reshape(B * N, 4, 4)  # noqa: E731
        Hm, Rn = ops.homography_matrices(d, n, Tx.reshape(B * N, 4, 4), ex(K), ex(Ki))
        return Hm.reshape(B, N, 3, 3), Rn.reshape(B, N, 3)
    Rm, t = Tx[..., :3, :3], Tx[..., :3, 3:4]
    M = Rm + torch.matmul(t, n[..., None, :]) / d[..., None, None]
    Hm = adjugate_inverse(torch.matmul(K[:, None, :3, :3], torch.matmul(M, Ki[:, None, :3, :3])))
    return Hm, torch.matmul(Rm, n[..., None])[..., 0]


def chain_uniform(d, n, Tx, K, Ki, stock):
    """The four slots of PD_HMAT_UNIFORM for a per-slot pose Tx [B,4,4,4]: slot 0 is plane 0 with the translation detached, slots
    1..3 the virtual planes n / d = e_j with the rotation detached; Rn of every real plane from slot 0's pose."""
    B, N = d.shape
    Rm, t = Tx[..., :3, :3], Tx[..., :3, 3:4]
    eye = torch.eye(3, dtype=d.dtype)
    first = Rm[:, :1] + torch.matmul(t[:, :1].detach(), n[:, :1, None, :]) / d[:, :1, None, None]
    rest = Rm[:, 1:].detach() + t[:, 1:] * eye.reshape(1, 3, 1, 3)
    A = torch.matmul(K[:, None, :3, :3], torch.matmul(torch.cat([first, rest], 1), Ki[:, None, :3, :3]))
    Hm = torch.inverse(A) if stock else adjugate_inverse(A)
    return Hm, torch.matmul(Rm[:, :1], n[..., None])[..., 0]


def hmat_reference_run(case, inp, stock=True, with_g_H=False):
    """The fp64 chain of a case and its gradients under the case's upstream gradient: forward tensors, g_distance, g_norm, g_T
    (summed over the per-plane / per-slot pose copies) and the allowance of every gradient."""
    B, N = case.B, case.N
    d, n, T = (inp[k].double().clone().requires_grad_(True) for k in ("distance", "norm", "T"))
    K, Ki = inp["K"].double(), inp["inv_K"].double()
    slots = 4 if case.mode == "uniform" else N
    Tx = T.detach()[:, None].expand(B, slots, 4, 4).clone().requires_grad_(True)
    out = {}
    if case.mode == "uniform":
        Hm, Rn = chain_uniform(d, n, Tx, K, Ki, stock)
        first = Hm
    else:
        Hm, Rn = chain_planes(d, n, Tx, K, Ki, stock)
        first = Hm
        if case.mode == "stereo_rows":
            y = torch.arange(case.rows, dtype=F64).reshape(1, 1, -1)
            first = out["shift"] = Hm[:, :, 0, 1, None] * y + Hm[:, :, 0, 2, None]
    out.update(H_t2s=Hm, Rn=Rn)
    obj = (first * inp["g_first"].double()).sum()
    if with_g_H:
        obj = obj + (Hm * inp["g_H"].double()).sum()
    gd, gn, gT = torch.autograd.grad(obj, [d, n, Tx], allow_unused=True)
    zeros = lambda g, like: torch.zeros_like(like) if g is None else g  # noqa: E731
    gd, gn, gT = zeros(gd, d), zeros(gn, n), zeros(gT, Tx)
    out.update(g_distance=gd, g_norm=gn, g_T=gT.sum(1)[:, :3], A_g_T=gT.abs().sum(1)[:, :3])
    return {k: v.detach() for k, v in out.items()}


def hmat_allowances(ref):
    a = dict(H_t2s=ref["H_t2s"].abs().amax((-2, -1), keepdim=True), Rn=ref["Rn"].abs().amax(-1, keepdim=True),
             g_distance=ref["g_distance"].abs(), g_norm=ref["g_norm"].abs(), g_T=ref["A_g_T"])
    if "shift" in ref:
        a["shift"] = ref["shift"].abs().amax(-1, keepdim=True)
    return a


def stereo_mask_reference(case, inp):
    """(mask [B,N,rows] of oracle.homography_grid in fp64, sure [B,N,rows]: the rows away from the reference's own knife edges,
    facing [B,N,rows])."""
    B, N, H = case.B, case.N, case.rows
    ex = lambda M: M.double()[:, None].expand(-1, N, -1, -1).reshape(B * N, 4, 4)  # noqa: E731
    d, n = inp["distance"].double(), inp["norm"].double()
    _, mask = orc.homography_grid(d, n, ex(inp["T"]), ex(inp["K"]), ex(inp["inv_K"]), H, 5)
    mask = mask.reshape(B, N, H, 5)
    assert bool((mask == mask[..., :1]).all())                 # constant along x: the row form exists
    Hm, Rn = orc.homography_matrices(d, n, ex(inp["T"]), ex(inp["K"]), ex(inp["inv_K"]))
    y = torch.arange(H, dtype=F64).reshape(1, 1, H)
    Ki = inp["inv_K"].double()
    ray = Ki[:, None, :3, 1, None] * y[..., None, :] + Ki[:, None, :3, 2, None]           # [B,1,3,H]: the rays at x = 0
    facing = (ray * Rn.reshape(B, N, 3, 1)).sum(2)
    Hm = Hm.reshape(B, N, 3, 3)
    z = Hm[:, :, 2, 1, None] * y + Hm[:, :, 2, 2, None]
    sure = (facing.abs() > 1e-5 * facing.abs().amax(-1, keepdim=True)) & ((z - 1e-7).abs() > 1e-9)
    return mask[..., 0].double(), sure, facing


@functools.lru_cache(maxsize=None)
def hmat_reference(name):
    case = HC[name]
    inp = hmat_inputs(case)
    ref = hmat_reference_run(case, inp)
    return inp, ref, hmat_allowances(ref)


HMAT_FWD = {"planes": ("H_t2s", "Rn"), "uniform": ("H_t2s", "Rn"), "stereo_rows": ("shift", "Rn")}


@pytest.mark.parametrize("name", H_IDS)
def test_homography_conditions_cpu(name):
    case = HC[name]
    inp, ref, allow = hmat_reference(name)
    other = hmat_reference_run(case, inp, stock=False)
    figures = {}
    for k in ("H_t2s", "Rn", "g_distance", "g_norm", "g_T") + (("shift",) if case.mode == "stereo_rows" else ()):
        a = allow[k].expand_as(ref[k])
        diff = (other[k] - ref[k]).abs()
        live = a > 0
        figures[k] = float((diff[live] / a[live]).max()) if bool(live.any()) else 0.0
        assert bool((diff <= NOISE * a).all()), (name, k, figures[k])     # the two orders agree: NOISE A is noise, not a margin
    figures["cond_H"] = float(torch.linalg.cond(ref["H_t2s"]).max())
    _record("homography_matrices/%s/two_orders" % name, figures)
    assert figures["cond_H"] < 1e5
    d = inp["distance"]
    assert float(d.min()) >= D_MIN and float(d.max()) <= D_MAX
    if case.N >= 5:
        assert float(d.max() / d.min()) > 10 ** (3.0 * (case.N - 2) / case.N)        # stratified over three decades
    if case.mode == "uniform":
        assert float(inp["T"][:, :3, 3].abs().max()) == 0.0
        assert float(ref["g_distance"].abs().max()) == 0.0 and float(ref["g_norm"].abs().max()) == 0.0
        assert float(ref["g_T"][:, :, 3].abs().min()) > 0                 # the translation column takes its gradient from slots 1..3
    elif case.N >= 5:
        gd = ref["g_distance"].abs()
        assert float(gd.max() / gd.min()) > 1e3, float(gd.max() / gd.min())             # decades inside one tensor
    if case.mode == "stereo_rows":
        assert float(inp["norm"][..., 0].abs().max()) == 0.0
        mask, sure, facing = stereo_mask_reference(case, inp)
        excluded = 1.0 - float(sure.double().mean())
        figures["mask_excluded"] = excluded
        assert excluded <= MASK_EXCLUDED_CAP, excluded
        assert torch.equal(mask[sure], (facing > 0).double()[sure])
        if case.rows >= 2:     # (a one-row image has no inside for the sign to change in)
            flips = ((facing[..., 1:] > 0) != (facing[..., :-1] > 0)).any(-1)
            assert bool(flips.any(-1).all()), "the facing test changes sign inside the image on some plane of every image"
            assert 0.0 < float(mask.mean()) < 1.0


def hmat_product(case, inp, grads=("distance", "norm", "T"), norm=None):
    """ops.homography_matrices_fused and its backward under the case's upstream gradient, for the leaves in ``grads``."""
    from planedepth_amd import ops
    leaf = lambda k, t: t.to(DEV).requires_grad_(k in grads)  # noqa: E731
    d, n, T = leaf("distance", inp["distance"]), leaf("norm", inp["norm"] if norm is None else norm), leaf("T", inp["T"])
    res = ops.homography_matrices_fused(d, n, T, inp["K"].to(DEV), inp["inv_K"].to(DEV), MODES[case.mode], rows=case.rows)
    out = {}
    if case.mode == "stereo_rows":
        out["shift"], out["mask"], out["Rn"] = res
        assert not res[1].requires_grad
    else:
        out["H_t2s"], out["Rn"] = res
    assert not out["Rn"].requires_grad
    if grads:
        (res[0] * inp["g_first"].to(DEV)).sum().backward()
    for k, t in (("g_distance", d), ("g_norm", n), ("g_T", T)):
        out[k] = t.grad
    return {k: (None if v is None else v.detach().cpu()) for k, v in out.items()}


def check_hmat(tag, got, ref, allow, keys):
    figures = {}
    for k in keys:
        g = got[k][:, :3] if k == "g_T" else got[k]
        r = ulp_report(g, ref[k], allow[k])
        figures[k] = r
        print(tag, k, "worst %.3f of the allowance, %.3f ulp" % (r["worst"], r["ulps"]))
        assert r["worst"] <= 1.0, (tag, k, r)
    return figures


@gpu
@pytest.mark.parametrize("name", H_IDS)
def test_homography_matrices_per_element(name):
    case = HC[name]
    inp, ref, allow = hmat_reference(name)
    grads = ("distance",) if case.mode == "stereo_rows" else ("distance", "norm", "T")
    got = hmat_product(case, inp, grads)
    keys = HMAT_FWD[case.mode] + (("g_distance",) if case.mode == "stereo_rows" else ("g_distance", "g_norm", "g_T"))
    _record("homography_matrices/%s/product" % name, check_hmat(name, got, ref, allow, keys))
    if case.mode == "stereo_rows":
        mask, sure, _ = stereo_mask_reference(case, inp)
        assert torch.equal(got["mask"].double()[sure], mask[sure])
        assert bool(((got["mask"] == 0) | (got["mask"] == 1)).all())
    else:
        assert float(got["g_T"][:, 3].abs().max()) == 0.0                  # the last row of the pose is never read
    if case.mode == "uniform":
        assert float(got["g_distance"].abs().max()) == 0.0 and float(got["g_norm"].abs().max()) == 0.0
    again = hmat_product(case, inp, grads)
    for k, v in got.items():
        assert v is None or torch.equal(v.view(torch.int32), again[k].view(torch.int32)), (name, k)


SUBSET_CASES = ["planes_n1", "planes_n65", "uniform_n2", "uniform_n70", "stereo_n3_r65"]


@gpu
@pytest.mark.parametrize("name", SUBSET_CASES)
def test_homography_operator_gradient_subsets(name):
    """Every subset of {distance, norm, T} the mode carries: the requested gradients meet the bar, the others are not produced."""
    case = HC[name]
    inp, ref, allow = hmat_reference(name)
    leaves = ("distance",) if case.mode == "stereo_rows" else ("distance", "norm", "T")
    for r in range(1, len(leaves) + 1):
        for grads in itertools.combinations(leaves, r):
            got = hmat_product(case, inp, grads)
            check_hmat("%s/%s" % (name, "+".join(grads)), got, ref, allow, tuple("g_" + k for k in grads))
            for k in leaves:
                assert (got["g_" + k] is None) == (k not in grads), (name, grads, k)
    got = hmat_product(case, inp, ())                                      # no leaf: forward only
    check_hmat(name + "/forward", got, ref, allow, HMAT_FWD[case.mode])
    if case.mode == "stereo_rows":
        for k in ("norm", "T"):
            with pytest.raises(RuntimeError, match="distance"):
                hmat_product(case, inp, ("distance", k))


@gpu
def test_homography_operator_without_upstream_gradient_and_broadcast_norm():
    from planedepth_amd import ops
    case = HC["planes_n11"]
    inp, ref, allow = hmat_reference(case.name)
    # g_first is None: the matrices took no part in the loss, no gradient and no launch
    ctx = types.SimpleNamespace(saved_tensors=tuple(inp[k].to(DEV) for k in ("distance", "norm", "T", "K", "inv_K")),
                                needs_input_grad=(True, True, True, False, False, False, False), mode=C.PD_HMAT_PLANES, rows=0)
    assert ops._HomographyMatrices.backward(ctx, None, None) == (None,) * 7
    d = inp["distance"].to(DEV).requires_grad_(True)
    Hm, Rn = ops.homography_matrices_fused(d, inp["norm"].to(DEV), inp["T"].to(DEV), inp["K"].to(DEV), inp["inv_K"].to(DEV))
    (Rn.sum() + d.sum()).backward()
    assert torch.equal(d.grad, torch.ones_like(d))
    # a broadcast normal gives the expanded result
    one = inp["norm"][:1, :1].contiguous()
    for mode in ("planes", "uniform"):
        c = case._replace(mode=mode)
        inp_m = dict(inp, T=f8_pose(c.B, 5, 0.05), g_first=inp["g_first"][:, :4]) if mode == "uniform" else inp
        want = hmat_product(c, inp_m, ("distance", "T"), norm=one.expand(c.B, c.N, 3).contiguous())
        for shape in ((1, 1, 3), (c.B, 1, 3), (3,)):
            b = one.reshape(-1)[:3].reshape(shape) if len(shape) == 1 else one.expand(*shape).contiguous()
            got = hmat_product(c, inp_m, ("distance", "T"), norm=b)
            for k, v in want.items():
                if v is not None:
                    assert torch.equal(got[k], v), (mode, shape, k)


def _hmat_fwd(lib, case, t, mode, Hm, Rn, shift, mask):
    B, N = case.B, case.N
    for buf, n in ((Hm, B * (4 if mode == C.PD_HMAT_UNIFORM else N) * 9), (Rn, B * N * 3), (shift, B * N * case.rows),
                   (mask, B * N * case.rows)):
        assert buf is None or (buf.numel() == n and buf.is_contiguous() and buf.dtype == torch.float32)
    C.check(lib.pd_homography_matrices_fwd(B, N, mode, case.rows, C.ptr(t["distance"]), C.ptr(t["norm"]), C.ptr(t["T"]),
                                           C.ptr(t["K"]), C.ptr(t["inv_K"]), C.ptr(Hm), C.ptr(Rn), C.ptr(shift), C.ptr(mask),
                                           C.stream_handle(t["T"].device)), "pd_homography_matrices_fwd")


def _stereo_bwd(lib, case, t, g_H, g_shift):
    B, N = case.B, case.N
    assert g_H is None or (g_H.numel() == B * N * 9 and g_H.is_contiguous())
    assert g_shift is None or (g_shift.numel() == B * N * case.rows and g_shift.is_contiguous())
    gd = torch.empty(B, N, device=DEV)
    C.check(lib.pd_homography_matrices_bwd(B, N, C.PD_HMAT_STEREO_ROWS, case.rows, C.ptr(t["distance"]), C.ptr(t["norm"]),
                                           C.ptr(t["T"]), C.ptr(t["K"]), C.ptr(t["inv_K"]), C.ptr(g_H), C.ptr(g_shift), C.ptr(gd),
                                           None, None, C.stream_handle(gd.device)), "pd_homography_matrices_bwd")
    return gd.cpu()


@gpu
@pytest.mark.parametrize("name", ["stereo_n3_r65", "stereo_n70_r130"])
def test_homography_c_entry_points(name):
    """What the C entry points accept and Python never passes: H_t2s in PD_HMAT_STEREO_ROWS, g_H together with g_shift, Rn = NULL."""
    lib = C.load()
    case = HC[name]
    inp, ref, allow = hmat_reference(name)
    B, N, rows = case.B, case.N, case.rows
    t = {k: inp[k].to(DEV).contiguous() for k in ("distance", "norm", "T", "K", "inv_K")}
    new = lambda *s: torch.full(s, float("nan"), device=DEV)  # noqa: E731
    H_planes, Rn_planes = new(B, N, 3, 3), new(B, N, 3)
    _hmat_fwd(lib, case, t, C.PD_HMAT_PLANES, H_planes, Rn_planes, None, None)
    H_rows, Rn_rows, shift, mask = new(B, N, 3, 3), new(B, N, 3), new(B, N, rows), new(B, N, rows)
    _hmat_fwd(lib, case, t, C.PD_HMAT_STEREO_ROWS, H_rows, Rn_rows, shift, mask)
    assert torch.equal(H_rows.view(torch.int32), H_planes.view(torch.int32))           # the same matrices, bit for bit
    assert torch.equal(Rn_rows.view(torch.int32), Rn_planes.view(torch.int32))
    check_hmat(name + "/c", dict(H_t2s=H_rows.cpu(), Rn=Rn_rows.cpu(), shift=shift.cpu()), ref, allow, ("H_t2s", "Rn", "shift"))
    for mode in (C.PD_HMAT_PLANES, C.PD_HMAT_STEREO_ROWS):                             # Rn = NULL: everything else unchanged
        H2 = new(B, N, 3, 3)
        s2, m2 = (new(B, N, rows), new(B, N, rows)) if mode == C.PD_HMAT_STEREO_ROWS else (None, None)
        _hmat_fwd(lib, case, t, mode, H2, None, s2, m2)
        assert torch.equal(H2.view(torch.int32), H_planes.view(torch.int32))
        if s2 is not None:
            assert torch.equal(s2.view(torch.int32), shift.view(torch.int32)) and torch.equal(m2, mask)
    # the stereo backward with both upstream gradients
    g_H, g_shift = inp["g_H"].to(DEV).contiguous(), inp["g_first"].to(DEV).contiguous()
    both, only_H, only_s = _stereo_bwd(lib, case, t, g_H, g_shift), _stereo_bwd(lib, case, t, g_H, None), _stereo_bwd(lib, case, t, None, g_shift)
    total = only_H.double() + only_s.double()
    # three values rounded once each from fp64: half an ulp of each
    assert bool(((both.double() - total).abs() <= 0.5 * ULP * (both.abs() + only_H.abs() + only_s.abs()).double() * 1.0001).all())
    ref_both = hmat_reference_run(case, inp, with_g_H=True)
    r = ulp_report(both, ref_both["g_distance"], ref_both["g_distance"].abs())
    _record("homography_matrices/%s/c_entry_both" % name, dict(g_distance=r))
    assert r["worst"] <= 1.0, r
    r = ulp_report(only_s, ref["g_distance"], allow["g_distance"])
    assert r["worst"] <= 1.0, r


# ---------------------------------------------------------------------------------------------------------------------
# composition: distance has two consumers
# ---------------------------------------------------------------------------------------------------------------------
COMPOSE = GeoCase("compose", 2, 3, 4, 65, 33, "crop")


def compose_inputs():
    case = COMPOSE
    inp = geo_inputs(case)
    K, inv_K = synthetic.intrinsics(case.B, case.H, case.W)
    g = torch.Generator().manual_seed(_seed("compose"))
    inp.update(T=synthetic.small_pose(None, case.B, stereo=True), K=K, inv_K=inv_K,
               g_shift=torch.randn(case.B, case.nl + case.nx, case.H, generator=g) * 3e-3)     # (1/d^2: else it drowns g_dist)
    return inp


def compose_chain(inp, dtype):
    """plane geometry (in ``dtype``) -> the stereo-row shift (fp64 on the geometry's rounded distance and normals, as the kernel
    evaluates it) -> sum(shift g_shift) + sum(disp_rows g_rows) + sum(distance g_dist); g_residual and the pieces of its allowance."""
    case = COMPOSE
    B, N, H = case.B, case.nl + case.nx, case.H
    res = inp["residual"].to(dtype).clone().requires_grad_(True)
    o = synthetic.decoder_plane_geometry(inp["grid"].to(dtype), res, rows=True, **geo_kw(case))
    rows, distance = o["disp_layered"][..., 0], o["distance"]
    d64 = distance.double()
    d_leaf = d64.detach().clone().requires_grad_(True)
    Tx = inp["T"].double()[:, None].expand(B, N, 4, 4)
    y = torch.arange(H, dtype=F64).reshape(1, 1, H)
    shift_of = lambda d: (lambda Hm: (Hm[:, :, 0, 1], Hm[:, :, 0, 2]))(  # noqa: E731
        chain_planes(d, o["norm"].detach().double(), Tx, inp["K"].double(), inp["inv_K"].double(), True)[0])
    h01, h02 = shift_of(d64)
    shift = h01[..., None] * y + h02[..., None]
    obj = (shift * inp["g_shift"].double()).sum() + (rows.double() * inp["g_rows"].double()).sum() + (d64 * inp["g_dist"].double()).sum()
    g_res, = torch.autograd.grad(obj, [res])
    a1, b1 = shift_of(d_leaf)
    da, = torch.autograd.grad(a1.sum(), [d_leaf], retain_graph=True)          # every plane's matrix depends on its own distance only
    db, = torch.autograd.grad(b1.sum(), [d_leaf])
    a_hmat = (inp["g_shift"].double() * (da[..., None] * y + db[..., None])).abs().sum(-1)      # sum_y |g_y d shift_y / d distance|
    return dict(g_residual=g_res.detach().double(), shift=shift.detach(), rows=rows.detach(), distance=distance.detach(),
                norm=o["norm"].detach(), a_hmat=a_hmat.detach())


@functools.lru_cache(maxsize=None)
def compose_reference():
    inp = compose_inputs()
    ref64, ref32 = compose_chain(inp, F64), compose_chain(inp, torch.float32)
    geo64 = dict(disp_rows=ref64["rows"], distance=ref64["distance"])
    # the geometry's allowance with |g_dist| + sum_y |g_y d shift_y / d distance| for the distance's upstream gradient
    allow = geo_allowance(COMPOSE, dict(inp, g_dist=inp["g_dist"].double().abs() + ref64["a_hmat"]), geo64)["both"]
    e_ref = term_report(ref32["g_residual"], ref64["g_residual"], allow)["err"]
    return inp, ref64, allow, e_ref


def test_composition_conditions_cpu():
    inp, ref64, allow, e_ref = compose_reference()
    print("composition E_ref %.2e" % e_ref)
    _record("composition/restatement", dict(e_ref=e_ref))
    assert e_ref <= E_REF_CAP_BWD
    assert float(ref64["norm"][..., 0].abs().max()) == 0.0
    gd_direct = inp["g_dist"].double().abs()
    assert bool((ref64["a_hmat"] > 0.05 * gd_direct).any()) and bool((gd_direct > 0.05 * ref64["a_hmat"]).any())   # both consumers count


@gpu
def test_geometry_into_stereo_rows_composition():
    from planedepth_amd import ops
    case = COMPOSE
    inp, ref64, allow, e_ref = compose_reference()
    res = inp["residual"].to(DEV).requires_grad_(True)
    dl, pm, distance, norm = ops.plane_geometry(inp["grid"].to(DEV), res, **geo_kw(case))
    shift, mask, _ = ops.homography_matrices_fused(distance, norm, inp["T"].to(DEV), inp["K"].to(DEV), inp["inv_K"].to(DEV),
                                                   C.PD_HMAT_STEREO_ROWS, rows=case.H)
    ((shift * inp["g_shift"].to(DEV)).sum() + (dl._pd_rows * inp["g_rows"].to(DEV)).sum()
     + (distance * inp["g_dist"].to(DEV)).sum()).backward()
    r = term_report(res.grad, ref64["g_residual"], allow)
    print("composition g_residual err %.2e E_ref %.2e at %s" % (r["err"], e_ref, r["worst"]))
    _record("composition/product", dict(err=r["err"], e_ref=e_ref))
    assert r["err"] <= 2.0 * e_ref + BWD_TOL and r["zero_abs"] == 0.0, (r, e_ref)
    fwd = ulp_report(shift, ref64["shift"], ref64["shift"].abs().amax(-1, keepdim=True))
    print("composition shift (on the fp64 geometry's distance): %.1f ulp" % fwd["ulps"])


# =====================================================================================================================
# 3. plane levels, crop grid, cat flip
# =====================================================================================================================
LEVEL_SHAPES = [(1, 1), (1, 255), (1, 256), (1, 257), (3, 70)]        # M = B * N: one thread, a ragged block, one block, two, 210
LEVELS_NL, LEVELS_W = 49, 40


def test_small_kernel_tables_cover_the_launch_arithmetic():
    kBlock, kWave = _kernel_constants()
    assert {b * n for b, n in LEVEL_SHAPES} == {1, kBlock - 1, kBlock, kBlock + 1, 3 * (kWave + 6)}
    hw = {c[0] * c[1] for c in CROP_CASES}
    assert {1, kBlock - 1, kBlock + 1} <= hw
    steps = {s for c in CROP_CASES for p in c[2] for s in p[:2]}
    assert {1, 2} <= steps and any(s % 2 for s in steps if s > 2) and any(s % 2 == 0 for s in steps if s > 2)
    assert all(len(set(c[2])) == len(c[2]) >= 2 for c in CROP_CASES)                   # different parameters per image
    assert all(p[2] + c[1] <= p[0] and p[3] + c[0] <= p[1] for c in CROP_CASES for p in c[2])      # the window lies in the frame
    chw = {c * h * w for _, c, h, w in FLIP_SHAPES}
    assert {1, 2, 37} <= {s[3] for s in FLIP_SHAPES} and any(v < kBlock for v in chw) and kBlock + 1 in chw
    assert any(c >= 2 and h * w < kBlock < c * h * w for _, c, h, w in FLIP_SHAPES)     # the channel-0 boundary inside a block


def levels_inputs(B, N):
    g = torch.Generator().manual_seed(1000 * B + N)
    levels = (torch.arange(B * N, dtype=torch.float32).reshape(B, N) % LEVELS_NL) + torch.rand(B, N, generator=g) - 0.5
    return dict(levels=levels, g_disp=torch.randn(B, N, generator=g), g_dist=torch.randn(B, N, generator=g))


def levels_restatement(inp, dtype):
    """networks/depth_decoder.py:150-154 as synthetic.decoder_plane_geometry states it."""
    lv = inp["levels"].to(dtype).clone().requires_grad_(True)
    disp = CFG["disp_max"] * (CFG["disp_min"] / CFG["disp_max"]) ** (lv / (LEVELS_NL - 1))
    distance = 0.1 * 0.58 * LEVELS_W / disp
    out = dict(disp=disp, distance=distance)
    ups = dict(rows=([disp], [inp["g_disp"].to(dtype)]), dist=([distance], [inp["g_dist"].to(dtype)]))
    ups["both"] = (ups["rows"][0] + ups["dist"][0], ups["rows"][1] + ups["dist"][1])
    for combo in COMBOS:
        out["g_levels/" + combo], = torch.autograd.grad(ups[combo][0], [lv], ups[combo][1], retain_graph=True)
    return {k: v.detach() for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def levels_reference(B, N):
    inp = levels_inputs(B, N)
    ref64, ref32 = levels_restatement(inp, F64), levels_restatement(inp, torch.float32)
    ln = abs(math.log(CFG["disp_min"] / CFG["disp_max"])) / (LEVELS_NL - 1)
    a_rows, a_dist = inp["g_disp"].double().abs() * ref64["disp"] * ln, inp["g_dist"].double().abs() * ref64["distance"] * ln
    allow = dict(rows=a_rows, dist=a_dist, both=a_rows + a_dist)
    e_ref = {k: rel_report(ref32[k], ref64[k])["err"] for k in ("disp", "distance")}
    for combo in COMBOS:
        e_ref["g_levels/" + combo] = term_report(ref32["g_levels/" + combo], ref64["g_levels/" + combo], allow[combo])["err"]
    return inp, ref64, allow, e_ref


@pytest.mark.parametrize("B,N", LEVEL_SHAPES)
def test_plane_levels_conditions_cpu(B, N):
    _, _, allow, e_ref = levels_reference(B, N)
    _record("plane_levels/%dx%d/restatement" % (B, N), e_ref)
    assert all(v <= (E_REF_CAP_BWD if k.startswith("g_") else E_REF_CAP) for k, v in e_ref.items()), e_ref
    assert bool((allow["rows"] > 0).all()) and bool((allow["dist"] > 0).all())


@gpu
@pytest.mark.parametrize("B,N", LEVEL_SHAPES)
def test_plane_levels_per_element(B, N):
    from planedepth_amd import ops
    inp, ref64, allow, e_ref = levels_reference(B, N)
    lv = inp["levels"].to(DEV).requires_grad_(True)
    disp, distance = ops.plane_disparities(lv, CFG["disp_min"], CFG["disp_max"], LEVELS_W, no_levels=LEVELS_NL)
    assert tuple(disp.shape) == (B, N, 1, 1) and tuple(distance.shape) == (B, N)
    figures = {}
    for k, v in (("disp", disp.reshape(B, N)), ("distance", distance)):
        r = rel_report(v, ref64[k])
        figures[k] = dict(err=r["err"], e_ref=e_ref[k])
        assert r["err"] <= 2.0 * e_ref[k] + FWD_TOL, (k, r, e_ref[k])
    ups = dict(rows=([disp], [inp["g_disp"].to(DEV).reshape(B, N, 1, 1)]), dist=([distance], [inp["g_dist"].to(DEV)]))
    ups["both"] = (ups["rows"][0] + ups["dist"][0], ups["rows"][1] + ups["dist"][1])
    got = {}
    for combo in COMBOS:
        k = "g_levels/" + combo
        got[combo], = torch.autograd.grad(ups[combo][0], [lv], ups[combo][1], retain_graph=True)
        r = term_report(got[combo], ref64[k], allow[combo])
        figures[k] = dict(err=r["err"], e_ref=e_ref[k])
        print(B, N, k, "err %.2e E_ref %.2e" % (r["err"], e_ref[k]))
        assert r["err"] <= 2.0 * e_ref[k] + BWD_TOL, (k, r, e_ref[k])
    lin = term_report(got["rows"].double() + got["dist"].double(), got["both"], allow["both"])
    assert lin["err"] <= LINEAR_TOL, lin
    _record("plane_levels/%dx%d/product" % (B, N), figures)


# (H, W, per-image (full_w, full_h, w0, h0)): steps of 1 and 2, odd and even, windows on both sides of the midpoint
CROP_CASES = [
    (1, 1, ((1, 1, 0, 0), (2, 2, 1, 0), (2, 3, 0, 1), (5, 4, 4, 3))),
    (15, 17, ((17, 15, 0, 0), (18, 16, 1, 1), (40, 33, 5, 7), (101, 64, 84, 49))),
    (1, 257, ((257, 1, 0, 0), (258, 2, 1, 1), (300, 5, 43, 2))),
    (2, 2, ((2, 2, 0, 0), (3, 3, 1, 1), (3, 2, 0, 0))),
]


def linspace_scalar(i, steps):
    """torch.linspace(-1, 1, steps)'s scalar formula in numpy fp32 (ATen RangeFactories)."""
    if steps <= 1:
        return np.float32(-1.0)
    step = np.float32(2.0) / np.float32(steps - 1)
    if i < steps // 2:
        return np.float32(-1.0) + step * np.float32(i)
    return np.float32(1.0) - step * np.float32(steps - i - 1)


@gpu
@pytest.mark.parametrize("H,W,params", CROP_CASES, ids=["%dx%d" % c[:2] for c in CROP_CASES])
def test_crop_grid_bits(H, W, params):
    from planedepth_amd import ops
    got = ops.crop_grid(torch.tensor(params, dtype=torch.int32, device=DEV), H, W).cpu()
    assert tuple(got.shape) == (len(params), 2, H, W)
    for b, (full_w, full_h, w0, h0) in enumerate(params):
        xs = np.array([linspace_scalar(w0 + x, full_w) for x in range(W)], dtype=np.float32)
        ys = np.array([linspace_scalar(h0 + y, full_h) for y in range(H)], dtype=np.float32)
        want = np.stack([np.broadcast_to(xs[None, :], (H, W)), np.broadcast_to(ys[:, None], (H, W))], 0)
        assert np.array_equal(got[b].numpy().view(np.int32), want.view(np.int32)), (b, params[b])
        lin = synthetic.crop_grid(H, W, full_h, full_w, h0, w0)
        assert float((got[b] - lin).abs().max()) <= ULP, (b, float((got[b] - lin).abs().max()))       # one ulp of the coordinate range


FLIP_SHAPES = [(2, 2, 3, 37), (1, 3, 5, 2), (2, 1, 257, 1), (2, 2, 4, 37), (1, 1, 1, 1)]


@gpu
@pytest.mark.parametrize("negate", [False, True], ids=["plain", "negate_c0"])
@pytest.mark.parametrize("B,Cn,H,W", FLIP_SHAPES)
def test_cat_flip_bits(B, Cn, H, W, negate):
    from planedepth_amd import ops
    g = torch.Generator().manual_seed(B + 10 * Cn + 100 * H + 1000 * W)
    own, other = torch.randn(B, Cn, H, W, generator=g), torch.randn(B, Cn, H, W, generator=g)
    other.view(-1)[0] = 0.0                                        # a zero that the mirror negates into -0
    got = ops.cat_flip(own.to(DEV), other.to(DEV), negate_c0=negate).cpu()
    if negate:      # the oracle's statement for the grid tensor (add_flip_right_inputs)
        flipped = other.clone()
        flipped[:, 0] *= -1.0
        want = torch.cat([own, flipped.flip(-1)], 0)
    else:
        want = torch.cat([own, other.flip(-1)], 0)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    sign = -1.0 if negate else 1.0
    for b in range(B):                                            # the channel-0 boundary, element by element
        for c in range(Cn):
            for y in (0, H - 1):
                for x in (0, W - 1):
                    v = float(other[b, c, y, W - 1 - x]) * (sign if c == 0 else 1.0)
                    assert float(got[B + b, c, y, x]) == v and float(got[b, c, y, x]) == float(own[b, c, y, x])
    if negate and Cn >= 2:
        assert torch.equal(got[B:, 1:], other[:, 1:].flip(-1)) and torch.equal(got[B:, 0], -other[:, 0].flip(-1))


@gpu
def test_cat_flip_matches_the_oracle_batch_doubling():
    from planedepth_amd import ops
    inputs = synthetic.kitti_like_inputs(2, 3, 37, seed=3)
    want = orc.add_flip_right_inputs(inputs)
    dev = {k: v.to(DEV) for k, v in inputs.items()}
    got_l = ops.cat_flip(dev[("color", "l")], dev[("color", "r")])
    got_g = ops.cat_flip(dev["grid"], dev["grid"], negate_c0=True)
    assert torch.equal(got_l.cpu().view(torch.int32), want[("color", "l")].view(torch.int32))
    assert torch.equal(got_g.cpu().view(torch.int32), want["grid"].view(torch.int32))
