"""The inference tails on the GPU (ops.decoder_tail_inference / ops.plade_tail_inference: pd_decoder_tail_infer /
pd_plade_tail_infer) against the training tails under no_grad (disp, depth and the stash bit for bit), against ``layers()``'s
probability and against the fp64 oracle on the exactly widened inputs; the memory the operator allocates.

Bounds.  ``confidence`` against ``layers()``'s ``probability.amax(1)``: 5e-6 absolute, the project's bound for a fused value
against its unfused form (a probability is at most 1).  Against the fp64 oracle: 1e-4 relative, the bound of the fp32 outputs in
tests/test_gpu_parity.py.  ``plane_index``: the oracle's probability there is within 5e-6 of the oracle's maximum (fp32 cannot
order two planes closer than its own error), and equals the oracle's argmax wherever the oracle's top two differ by more than
1e-5 (twice that error)."""
import itertools

import pytest
import torch

from oracle import planedepth_oracle as oracle
from planedepth_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
ALL = ("depth", "confidence", "plane_index", "disp_best", "layers")

# (B,N,H,W): 4 pixels per lane; odd H*W, 1 pixel per lane; H*W % 4 == 0 but W % 4 != 0 (a row form then takes 1 pixel per lane);
# two workgroups of 4-pixel lanes, the second partial; five workgroups of 1-pixel lanes
SHAPES = [(2, 5, 8, 16), (1, 3, 3, 5), (2, 4, 2, 6), (1, 2, 5, 300), (1, 2, 7, 150)]
N1 = (2, 1, 4, 8)
DISP_FORMS = ("plane", "dense", "rows")
MASK_FORMS = (None, "dense", "rows")


def _levels(B, N, W, g):
    """Per-plane disparities as the decoders space them (decreasing with the plane index), jittered per image."""
    lv = torch.arange(N, dtype=torch.float32)[None, :, None, None] + 0.5 * (torch.rand(B, N, 1, 1, generator=g) - 0.5)
    return 300.0 * (W / 640.0) * (2.0 / 300.0) ** (lv / max(N - 1, 1))


def _disp(form, shape, g):
    """(what the operator gets, the dense fp32 [B,N,H,W] map it stands for)"""
    B, N, H, W = shape
    lv = _levels(B, N, W, g).to(DEV)
    if form == "plane":
        dl = lv.expand(B, N, H, W)
        return dl, dl.contiguous()
    if form == "rows":
        rows = (lv[..., 0] * (1.0 + 0.2 * torch.rand(B, 1, H, generator=g).to(DEV))).contiguous()
        return ops.row_view(rows, W), rows.unsqueeze(-1).expand(B, N, H, W).contiguous()
    dense = (lv * (1.0 + 0.2 * torch.rand(B, 1, H, W, generator=g).to(DEV))).contiguous()
    return dense, dense


def _mask(form, shape, g):
    """0/1 mask; plane 0 stays in view everywhere (the xy planes of the reference always are), so no pixel loses every weight"""
    B, N, H, W = shape
    if form is None:
        return None, torch.ones(B, N, H, W, device=DEV)
    if form == "rows":
        rows = (torch.rand(B, N, H, generator=g) > 0.4).float().to(DEV)
        rows[:, 0] = 1.0
        return ops.row_view(rows, W), rows.unsqueeze(-1).expand(B, N, H, W).contiguous()
    dense = (torch.rand(B, N, H, W, generator=g) > 0.4).float().to(DEV)
    dense[:, 0] = 1.0
    return dense, dense


def _conv_outputs(shape, g, bf16, channels=None):
    B, N, H, W = shape
    rl = (torch.randn(B, channels or N, H, W, generator=g) * 2.5).to(DEV)
    rs = (torch.randn(B, N, H, W, generator=g) * 3 - 1).to(DEV)
    rs.view(-1)[0::7] = -12.0    # sigmoid = 6e-6: clamped to 0.01
    rs.view(-1)[2::11] = 30.0    # sigmoid = 1.0 exactly: on the upper bound
    return (rl.to(BF), rs.to(BF)) if bf16 else (rl, rs)


def _check(res, train_disp, train_depth, train_stash, prob, prob64, dense_dl):
    """Everything the issue asks of one case.  ``prob``: layers()'s probability (device, fp32); ``prob64``: the oracle's (CPU)."""
    assert torch.equal(res.disp, train_disp)
    assert torch.equal(res.depth, train_depth)
    assert torch.equal(res.layers.stash, train_stash)
    assert not torch.isnan(res.disp).any()
    assert res.confidence.dtype == torch.float32 and res.plane_index.dtype == torch.int32
    assert res.confidence.shape == res.plane_index.shape == res.disp_best.shape == res.disp.shape
    conf, idx = res.confidence.cpu().double(), res.plane_index.cpu().long()
    err_layers = float((res.confidence - prob.amax(1, keepdim=True)).abs().max())
    want = prob64.amax(1, keepdim=True)
    err_oracle = float(((conf - want).abs() / want).max())
    print("confidence: |vs layers| %.3g  rel vs fp64 %.3g" % (err_layers, err_oracle))
    assert err_layers <= 5e-6
    assert err_oracle <= 1e-4
    assert int(idx.min()) >= 0 and int(idx.max()) < prob64.shape[1]
    at_idx = prob64.gather(1, idx)
    assert bool((at_idx >= want - 5e-6).all()), float((want - at_idx).max())
    top2 = prob64.topk(2, dim=1).values if prob64.shape[1] > 1 else None
    clear = (top2[:, :1] - top2[:, 1:2]) > 1e-5 if top2 is not None else torch.ones_like(idx, dtype=torch.bool)
    assert torch.equal(idx[clear], prob64.argmax(1, keepdim=True)[clear])
    assert torch.equal(res.disp_best, dense_dl.gather(1, res.plane_index.long()))
    # layers() of the inference operator is the training tail's, from the same stash
    assert torch.equal(res.layers(False, True)[1], prob)


def _run_decoder(shape, disp_form, mask_form, mix, bf16, seed=0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    rl, rs = _conv_outputs(shape, g, bf16)
    dl, dense_dl = _disp(disp_form, shape, g)
    pm, dense_pm = _mask(mask_form, shape, g)
    with torch.no_grad():
        _, _, disp, depth, layers = ops.decoder_tail(rl, rs if mix else None, pm, dl, use_mixture_loss=mix)
        res = ops.decoder_tail_inference(rl, rs if mix else None, pm, dl, use_mixture_loss=mix, want=ALL)
    want = oracle.decoder_tail(rl.double().cpu(), rs.double().cpu(), dense_pm.double().cpu(), dense_dl.double().cpu(), shape[3],
                               use_mixture_loss=mix)
    _check(res, disp, depth, layers.stash, layers(False, True)[1], want["probability"], dense_dl)
    return res


def _decoder_variants():
    for shape in SHAPES + [N1]:
        for disp_form, mask_form, mix, bf16 in itertools.product(DISP_FORMS, MASK_FORMS, (True, False), (False, True)):
            yield pytest.param(shape, disp_form, mask_form, mix, bf16,
                               id="%s-%s-%s-%s-%s" % ("x".join(map(str, shape)), disp_form, mask_form or "nomask",
                                                      "mix" if mix else "pi", "bf16" if bf16 else "fp32"))


@pytest.mark.parametrize("shape,disp_form,mask_form,mix,bf16", list(_decoder_variants()))
def test_decoder_tail_inference(shape, disp_form, mask_form, mix, bf16):
    res = _run_decoder(shape, disp_form, mask_form, mix, bf16)
    if shape[1] == 1:   # one plane: it holds all the probability
        assert bool((res.confidence == 1.0).all()) and bool((res.plane_index == 0).all())


@pytest.mark.parametrize("mix", [True, False])
@pytest.mark.parametrize("bf16", [False, True])
def test_decoder_tail_inference_on_the_reference_plane_set(mix, bf16):
    """49 xy + 14 xz planes through ops.plane_geometry (row views of disparities and mask); the y-grid crosses zero, so the upper
    rows mask every xz plane (logit 0 in the softmax, weight 0)."""
    B, N, H, W = shape = (1, 63, 4, 32)
    g = torch.Generator().manual_seed(63)
    grid = torch.stack(torch.meshgrid(torch.linspace(-1, 1, W), torch.linspace(-1, 1, H), indexing="xy"), 0)[None].to(DEV)
    residual = (torch.rand(B, N, generator=g) - 0.5).to(DEV)
    with torch.no_grad():
        dl, pm, _, _ = ops.plane_geometry(grid, residual, no_levels=49, xz_levels=14, disp_min=2.0, disp_max=300.0,
                                          xz_min=0.1852, xz_max=0.3704)
        assert dl.stride(3) == 0 and pm.stride(3) == 0
        assert bool((pm[:, 49:, :2] == 0).all()) and bool((pm[:, 49:, 2:] == 1).all())
        rl, rs = _conv_outputs(shape, g, bf16)
        _, _, disp, depth, layers = ops.decoder_tail(rl, rs if mix else None, pm, dl, use_mixture_loss=mix)
        res = ops.decoder_tail_inference(rl, rs if mix else None, pm, dl, use_mixture_loss=mix, want=ALL)
    dense_dl, dense_pm = dl.contiguous(), pm.contiguous()
    want = oracle.decoder_tail(rl.double().cpu(), rs.double().cpu(), dense_pm.double().cpu(), dense_dl.double().cpu(), W,
                               use_mixture_loss=mix)
    _check(res, disp, depth, layers.stash, layers(False, True)[1], want["probability"], dense_dl)
    if mix:   # a masked plane has weight 0: never the best one
        assert bool((res.plane_index[:, :, :2] < 49).all())


@pytest.mark.parametrize("pair", [(1, 2), (0, 3)])
@pytest.mark.parametrize("mix", [True, False])
def test_the_lower_index_wins_a_tie(pair, mix):
    """Two identical planes that dominate the others.  The first of them becomes the softmax reference (weight e^0 / sigma); no
    plane after it moves the reference, so the best weight is never rescaled and the second one arrives with the same bits: the
    strict comparison keeps the lower index."""
    B, N, H, W = shape = (1, 4, 2, 8)
    g = torch.Generator().manual_seed(11)
    rl, rs = _conv_outputs(shape, g, False)
    rl.clamp_(-2.0, 2.0)
    lo, hi = pair
    rl[:, lo] = 6.0 + torch.rand(B, H, W, generator=g).to(DEV)
    rl[:, hi] = rl[:, lo]
    rs[:, lo] = -3.0          # the smallest sigma of the four as well: the largest weight with the mixture
    rs[:, hi] = rs[:, lo]
    rs[:, [i for i in range(N) if i not in pair]] = 0.0
    lv = _levels(B, N, W, g).to(DEV)
    lv[:, hi] = lv[:, lo]
    with torch.no_grad():
        res = ops.decoder_tail_inference(rl, rs if mix else None, None, lv.expand(B, N, H, W), use_mixture_loss=mix, want=ALL)
        prob = res.layers(False, True)[1]
    assert torch.equal(prob[:, lo], prob[:, hi]) and bool((prob[:, lo] == prob.amax(1)).all())
    assert bool((res.plane_index == lo).all())


@pytest.mark.parametrize("want", [(), ("confidence",), ("depth", "plane_index"), ("disp_best", "layers"), "depth"])
def test_outputs_not_asked_for_are_none(want):
    shape = (2, 5, 8, 16)
    g = torch.Generator().manual_seed(5)
    rl, rs = _conv_outputs(shape, g, False)
    dl, _ = _disp("plane", shape, g)
    names = (want,) if isinstance(want, str) else want
    with torch.no_grad():
        full = ops.decoder_tail_inference(rl, rs, None, dl, want=ALL)
        part = ops.decoder_tail_inference(rl, rs, None, dl, want=want)
        pfull = ops.plade_tail_inference(rl[:, :-1], rs, dl, want=ALL)
        ppart = ops.plade_tail_inference(rl[:, :-1], rs, dl, want=want)
    for a, b in ((full, part), (pfull, ppart)):
        assert torch.equal(a.disp, b.disp)
        for name in ("depth", "confidence", "plane_index", "disp_best"):
            if name in names:
                assert torch.equal(getattr(a, name), getattr(b, name)), name
            else:
                assert getattr(b, name) is None, name
        assert (b.layers is not None) == ("layers" in names)
        assert not b.disp.requires_grad and b.disp.grad_fn is None
    default = ops.decoder_tail_inference(rl, rs, None, dl)   # (gradients enabled, but no input asks for one: legal)
    assert default.depth is not None and default.confidence is not None
    assert default.plane_index is None and default.disp_best is None and default.layers is None


def _run_plade(shape, disp_form, mix, bf16, seed=0):
    B, N, H, W = shape
    g = torch.Generator().manual_seed(seed + sum(shape))
    rl, rs = _conv_outputs(shape, g, bf16, channels=N - 1)
    dl, dense_dl = _disp(disp_form, shape, g)
    ray = ops.camera_ray_norm(H, W, torch.device(DEV, torch.cuda.current_device()))
    with torch.no_grad():
        _, _, _, disp, depth, layers = ops.plade_tail(rl, rs if mix else None, dl, use_mixture_loss=mix)
        res = ops.plade_tail_inference(rl, rs if mix else None, dl, use_mixture_loss=mix, want=ALL)
    want = oracle.plade_tail(rl.double().cpu(), rs.double().cpu(), dense_dl.double().cpu(), W, ray.double().cpu()[None],
                             use_mixture_loss=mix)
    _check(res, disp, depth, layers.stash, layers(False, True)[1], want["probability"], dense_dl)


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("mix", [True, False], ids=["mix", "pi"])
@pytest.mark.parametrize("disp_form", DISP_FORMS)   # (rows: a row view, which this tail materialises)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_plade_tail_inference(shape, disp_form, mix, bf16):
    _run_plade(shape, disp_form, mix, bf16)


def test_nothing_plane_sized_is_allocated():
    """Peak memory of the call beyond what was allocated before it: below one [B,N,H,W] fp32 tensor for the inference operator,
    above it for the training tail under no_grad (which writes logits and sigma) — the probe sees the difference."""
    B, N, H, W = shape = (2, 16, 32, 64)
    plane_bytes = B * N * H * W * 4
    g = torch.Generator().manual_seed(16)
    rl, rs = _conv_outputs(shape, g, False)
    dl, _ = _disp("plane", shape, g)
    pm, _ = _mask("dense", shape, g)

    def peak(fn):
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        with torch.no_grad():
            out = fn()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - before, out

    infer, res = peak(lambda: ops.decoder_tail_inference(rl, rs, pm, dl))
    train, out = peak(lambda: ops.decoder_tail(rl, rs, pm, dl))
    print("peak bytes beyond the inputs: inference %d, training tail %d, one plane tensor %d" % (infer, train, plane_bytes))
    assert torch.equal(res.disp, out[2])
    assert infer < plane_bytes
    assert train > plane_bytes
