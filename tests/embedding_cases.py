"""Helpers of tests/test_grid_embedding.py: a plain fp64 restatement of the grid embedding pyramid (the checker, not the product),
torch's own fp32 formulation of the reference's statements, the input builders and the reader of tests/golden/grid_embedding.npz.

The restatement follows networks/depth_decoder.py:66-71, 123-139 (``epconv``, then ``F.interpolate`` bilinear with
``align_corners=True``), layers.py:308-354 (``Embedder``) and ATen's upsample_bilinear2d: embed at the four taps, blend along x, then
along y.  The source coordinate y (H - 1) / (h - 1) is split into floor and fraction by an integer division; ELU uses ``torch.expm1``.
"""
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

from conftest import GOLDEN

FIXTURE = os.path.join(GOLDEN, "grid_embedding.npz")
HIDDEN = 16
KINDS = ("neural", "frequency", "identity")
LEVELS = ((1, 1), (1, 5), (4, 1), (7, 13), (23, 41), (30, 50), (12, 21))   # of a 23 x 41 grid: degenerate, down, equal, up
SMALL = (3, 23, 41)
WORKLOAD = (8, 192, 640)
DECODER_LEVELS = ((6, 20), (12, 40), (24, 80), (48, 160), (96, 320))


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
def crop_grids(B, H, W):
    """[B,2,H,W] fp32: per sample a window of linspace(-1, 1, full) with its own (full_w, full_h, w0, h0), as RandomResizeCrop leaves
    inputs["grid"]; odd samples flipped as trainer.py:258-260 flips them (x negated, columns reversed)."""
    grid = torch.empty(B, 2, H, W)
    for b in range(B):
        full_w, full_h = W + 3 + 7 * b, H + 2 + 5 * b
        w0, h0 = (3 * b + 1) % (full_w - W + 1), (2 * b + 1) % (full_h - H + 1)
        grid[b, 0] = torch.linspace(-1, 1, full_w)[w0:w0 + W][None, :]
        grid[b, 1] = torch.linspace(-1, 1, full_h)[h0:h0 + H][:, None]
        if b % 2:
            grid[b, 0] = -grid[b, 0].flip(-1)
    return grid


def make_weights(E, seed=0):
    """(w1 [16,2], b1 [16], w2 [E,16], b2 [E]) fp32, scaled so that both branches of both ELUs are live on a crop grid."""
    g = torch.Generator().manual_seed(1000 + 17 * E + seed)
    return (1.5 * torch.randn(HIDDEN, 2, generator=g), 0.5 * torch.randn(HIDDEN, generator=g),
            0.6 * torch.randn(E, HIDDEN, generator=g), 0.5 * torch.randn(E, generator=g))


def level_gradients(B, E, sizes, seed=0):
    """g_out ~ randn per level."""
    g = torch.Generator().manual_seed(77 + seed)
    return [torch.randn(B, E, h, w, generator=g) for h, w in sizes]


def negative_shares(grid, weights):
    """The shares of z1 and of z2 that are negative (fp64)."""
    w1, b1, w2, b2 = (t.double() for t in weights)
    z1 = torch.einsum("jc,bchw->bjhw", w1, grid.double()) + b1[None, :, None, None]
    z2 = torch.einsum("ej,bjhw->behw", w2, elu(z1)) + b2[None, :, None, None]
    return float((z1 < 0).double().mean()), float((z2 < 0).double().mean())


# ---------------------------------------------------------------------------------------------------------------------
# the fp64 restatement
# ---------------------------------------------------------------------------------------------------------------------
def elu(z):
    return torch.where(z > 0, z, torch.expm1(z))


def embed(grid, kind, weights=None, multires=0):
    """[B,E,H,W] in grid's dtype: the embedding at every grid point."""
    if kind == "identity":
        return grid
    if kind == "frequency":
        return torch.cat([grid] + [fn(grid * 2.0 ** k) for k in range(multires) for fn in (torch.sin, torch.cos)], 1)
    w1, b1, w2, b2 = (t.to(grid.dtype).reshape(t.shape[0], -1) if t.dim() > 1 else t.to(grid.dtype) for t in weights)
    e1 = elu(torch.einsum("jc,bchw->bjhw", w1, grid) + b1[None, :, None, None])
    return elu(torch.einsum("ej,bjhw->behw", w2, e1) + b2[None, :, None, None])


def axis_taps(n_out, n_in):
    """(first tap, second tap, fraction fp64) of the n_out positions of an axis of n_in under align_corners=True, split exactly."""
    num, den = torch.arange(n_out) * (n_in - 1), max(n_out - 1, 1)
    i0 = torch.div(num, den, rounding_mode="floor")
    return i0, (i0 + 1).clamp(max=n_in - 1), (num - i0 * den).double() / den


def resample(emb, size):
    """ATen's upsample_bilinear2d (align_corners=True) of [B,E,H,W] to ``size``: along x, then along y."""
    y0, y1, ty = axis_taps(size[0], emb.shape[2])
    x0, x1, tx = axis_taps(size[1], emb.shape[3])
    tx, ty = tx.to(emb.dtype), ty.to(emb.dtype)[:, None]

    def along_x(rows):
        return rows[..., x0] * (1 - tx) + rows[..., x1] * tx
    return along_x(emb[:, :, y0]) * (1 - ty) + along_x(emb[:, :, y1]) * ty


def pyramid_fp64(grid, sizes, kind, weights=None, multires=0):
    """The levels in fp64, list of [B,E,h,w]."""
    emb = embed(grid.double(), kind, weights, multires)
    return [resample(emb, s) for s in sizes]


def pyramid_and_gradients_fp64(grid, sizes, weights, g_levels):
    """(levels, (g_w1, g_b1, g_w2, g_b2)) in fp64 for the neural kind: the gradients of sum_l <g_l, level_l> by autograd in fp64."""
    leaves = [t.double().clone().requires_grad_(True) for t in weights]
    levels = pyramid_fp64(grid, sizes, "neural", leaves)
    loss = sum((lv * g.double()).sum() for lv, g in zip(levels, g_levels))
    grads = torch.autograd.grad(loss, leaves)
    return [lv.detach() for lv in levels], grads


# ---------------------------------------------------------------------------------------------------------------------
# torch's formulation in fp32: the reference's statements
# ---------------------------------------------------------------------------------------------------------------------
def epconv_module(weights):
    """The reference's ``epconv`` (networks/depth_decoder.py:66-71) holding ``weights``."""
    w1, b1, w2, b2 = weights
    m = torch.nn.Sequential(torch.nn.Conv2d(2, HIDDEN, kernel_size=1, stride=1, padding=0, bias=True), torch.nn.ELU(inplace=True),
                            torch.nn.Conv2d(HIDDEN, w2.shape[0], kernel_size=1, stride=1, padding=0, bias=True),
                            torch.nn.ELU(inplace=True))
    with torch.no_grad():
        m[0].weight.copy_(w1.reshape(HIDDEN, 2, 1, 1))
        m[0].bias.copy_(b1)
        m[2].weight.copy_(w2.reshape(-1, HIDDEN, 1, 1))
        m[2].bias.copy_(b2)
    return m


def torch_pyramid(module, grid, sizes):
    """``epconv`` on the full grid, then one F.interpolate per level, as the decoders' forward does (module None: the raw grid)."""
    emb = grid if module is None else module(grid)
    return [F.interpolate(emb, size=tuple(s), align_corners=True, mode="bilinear") for s in sizes]


def allowance(want, rel, floor):
    """rel |want| + floor max|want| per element."""
    return rel * want.abs() + floor * float(want.abs().max())


_fixture = {}


def load_fixture():
    """(meta dict, arrays) of tests/golden/grid_embedding.npz (made by tests/golden/make_embedding_golden.py from the reference)."""
    if not _fixture:
        z = np.load(FIXTURE)
        _fixture["meta"] = json.loads(str(z["meta"]))
        _fixture["arrays"] = {k: z[k] for k in z.files if k != "meta"}
    return _fixture["meta"], _fixture["arrays"]


def fixture_weights(arrays, tag):
    return tuple(torch.from_numpy(arrays["%s/%s" % (tag, n)]) for n in ("w1", "b1", "w2", "b2"))
