"""Novel views at inference on the GPU (ops.render_views / pd_render_views, predict.render) against the fp32 oracle on the CPU
evaluated as the operator's contract states it, against the product's own training route, and for what must hold whatever the
numbers are: the invariants of a baseline of zero, launch independence bit for bit, full overwrite of the outputs, no
plane-sized allocation.

Oracle, per view with baseline factor s (``_oracle``): ``decoder_tail`` (its logits / sigma), ``disp_grid(float32(s) *
disp_layered, "r")``, ``plane_sweep`` of the image and of a ones image, ``(probability_rec * disp_layered).sum(1)``.  It runs in
fp32 on the CPU, on the exactly widened inputs for bf16 conv outputs, once per case and baseline (``_CACHE``).

Bounds.  Against the oracle ``cases.rel_err`` below the suite's TOL = 1e-4, the bound tests/test_gpu_parity.py holds the disp
path to against the same oracle.  Against the training route (``ops.decoder_tail`` under no_grad, then ``ops.plane_sweep_disp``'s
``rgb_rec``) 2e-4: each side is within 1e-4 of the same oracle.  With bf16 conv outputs the training tail hands the sweep a sigma
ROUNDED to bf16 (a relative step of 2^-8), where the operator — like the oracle on the widened inputs — keeps the fp32 sigma; the
two sides then answer different questions, so the training route is run on the widened fp32 inputs there, which is the
evaluation both are bound to.

Shapes (B,N,H,W): (2,5,8,16) one partial wave; (1,3,3,5) odd W and H; (2,4,2,6) W % 4 != 0; (1,2,5,300) and (1,2,7,150) several
waves per row, the last one partial; (1,1,4,8) N = 1; (1,9,24,80) per plane and with row disparities and a row mask (H = 24 has
six rows whose vertical round trip is inexact, H = 7 and H = 8 one each: the two-source-row path); (1,2,3,1100) a row wider than
a workgroup has lanes, the kernel's other path: two columns per lane; (1,2,2,600) a width at which launches of one or two views
take two columns per lane and launches of three or four take one, so the launch-independence check compares the two paths."""
import ctypes
import itertools

import pytest
import torch

import planedepth_amd
from cases import rel_err
from oracle import planedepth_oracle as oracle
from planedepth_amd import _capi as C
from planedepth_amd import decoder_tail as DT
from planedepth_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
TOL = 1e-4            # tests/test_gpu_parity.py's bound for the disp path against this oracle
TRAIN_TOL = 2e-4      # two evaluations, each within TOL of the same oracle

SHAPES = [(2, 5, 8, 16), (1, 3, 3, 5), (2, 4, 2, 6), (1, 2, 5, 300), (1, 2, 7, 150), (1, 1, 4, 8), (1, 9, 24, 80), (1, 2, 3, 1100), (1, 2, 2, 600)]
ROWS_SHAPE = (1, 9, 24, 80)
SETS = [(1.0,), (-1.0,), (0.0,), (0.5, -0.5), (1.0, -1.0, 0.25, 2.0), (1.0, -1.0, 0.5, 0.25, 3.0)]


def _case(shape, rows, mix, bf16, applied):
    """The inputs of one case: what the operator gets (device) and the dense fp32 CPU tensors the oracle reads."""
    B, N, H, W = shape
    g = torch.Generator().manual_seed(sum(shape) + 17 * rows)
    rl = (torch.randn(B, N, H, W, generator=g) * 2.5).to(DEV)
    rs = (torch.randn(B, N, H, W, generator=g) * 3 - 1).to(DEV)
    rs.view(-1)[0::7] = -12.0    # sigmoid = 6e-6: clamped to 0.01
    rs.view(-1)[2::11] = 30.0    # sigmoid = 1.0 exactly: on the upper bound
    image = torch.rand(B, 3, H, W, generator=g).to(DEV)
    # disparities as the decoders space them, decreasing with the plane index, up to 0.47 * W
    lv = torch.arange(N, dtype=torch.float32)[None, :, None, None] + 0.5 * (torch.rand(B, N, 1, 1, generator=g) - 0.5)
    lv = (0.47 * W * (2.0 / 300.0) ** (lv.clamp_min(0.0) / max(N - 1, 1))).to(DEV)
    if rows:
        drows = (lv[..., 0] * (0.8 + 0.2 * torch.rand(B, 1, H, generator=g).to(DEV))).contiguous()
        dl, dense_dl = ops.row_view(drows, W), drows.unsqueeze(-1).expand(B, N, H, W).contiguous()
        mrows = (torch.rand(B, N, H, generator=g) > 0.4).float().to(DEV)
        mrows[:, 0] = 1.0        # plane 0 is always in view
        pm, dense_pm = ops.row_view(mrows, W), mrows.unsqueeze(-1).expand(B, N, H, W).contiguous()
    else:
        dl, dense_dl = lv.expand(B, N, H, W), lv.expand(B, N, H, W).contiguous()
        pm, dense_pm = None, torch.ones(B, N, H, W, device=DEV)
    if applied:   # logits / sigma as a tail wrote them
        rl, rs = rl * dense_pm, torch.clamp(torch.sigmoid(rs), 0.01, 1.0)
    if bf16:
        rl, rs = rl.to(BF), rs.to(BF)
    return dict(shape=shape, mix=mix, applied=applied, rl=rl, rs=rs if mix else None, pm=pm, dl=dl, image=image,
                cpu=dict(rl=rl.float().cpu(), rs=rs.float().cpu(), pm=dense_pm.cpu(), dl=dense_dl.cpu(), image=image.cpu()))


_CACHE = {}


def _oracle(key, case, s):
    """(rgb [B,3,H,W], coverage [B,1,H,W], disp [B,1,H,W]) of one view, fp32 on the CPU; computed once per case and baseline."""
    if (key, s) not in _CACHE:
        c, mix = case["cpu"], case["mix"]
        W = case["shape"][3]
        if case["applied"]:
            logits, sigma = c["rl"], c["rs"]
        else:
            tail = oracle.decoder_tail(c["rl"], c["rs"], c["pm"], c["dl"], W, mix)
            logits, sigma = tail["logits"], tail.get("sigma")
        grid = oracle.disp_grid(torch.tensor(s, dtype=torch.float32) * c["dl"], "r")
        mask = c["pm"][:, :, None]
        out = oracle.plane_sweep(c["image"], logits, sigma, grid, mask, use_mixture_loss=mix)
        ones = oracle.plane_sweep(torch.ones_like(c["image"]), logits, sigma, grid, mask, use_mixture_loss=mix)
        _CACHE[key, s] = (out["rgb_rec"], ones["rgb_rec"][:, :1], (out["probability_rec"] * c["dl"]).sum(1, True))
    return _CACHE[key, s]


def _render(case, baselines, want=("coverage", "disp")):
    with torch.no_grad():
        return ops.render_views(case["rl"], case["rs"], case["pm"], case["dl"], case["image"], baselines,
                                use_mixture_loss=case["mix"], tail_applied=case["applied"], want=want)


def _training_route(case, side):
    """rgb_rec of the product's training route for target ``side``: decoder_tail under no_grad, then the sweep's forward with the
    source image standing in as target (on the widened inputs for bf16 conv outputs: the module docstring)."""
    rl = case["rl"].float()
    rs = None if case["rs"] is None else case["rs"].float()
    with torch.no_grad():
        if case["applied"]:
            logits, sigma = rl, rs
        else:
            logits, sigma, _, _, _ = ops.decoder_tail(rl, rs, case["pm"], case["dl"], use_mixture_loss=case["mix"])
        return ops.plane_sweep_disp(case["image"], case["image"], logits, sigma, case["dl"], case["pm"], target_side=side,
                                    use_mixture_loss=case["mix"])[0]


def _variants():
    for shape, mix, bf16, applied in itertools.product(SHAPES, (True, False), (False, True), (False, True)):
        for rows in ((False, True) if shape == ROWS_SHAPE else (False,)):
            yield pytest.param(shape, rows, mix, bf16, applied,
                               id="%s-%s-%s-%s-%s" % ("x".join(map(str, shape)), "rows" if rows else "plane", "mix" if mix else "pi",
                                                      "bf16" if bf16 else "fp32", "applied" if applied else "raw"))


@pytest.mark.parametrize("shape,rows,mix,bf16,applied", list(_variants()))
def test_render_views(shape, rows, mix, bf16, applied):
    B, N, H, W = shape
    key = (shape, rows, mix, bf16, applied)
    case = _case(shape, rows, mix, bf16, applied)
    dense_dl, dense_pm = case["cpu"]["dl"], case["cpu"]["pm"]
    got = {}
    for baselines in SETS:
        res = _render(case, baselines)
        got[baselines] = res
        V = len(baselines)
        assert res.rgb.shape == (B, V, 3, H, W) and res.coverage.shape == res.disp.shape == (B, V, 1, H, W)
        for t in res:
            assert t.dtype == torch.float32 and not t.requires_grad and not torch.isnan(t).any()
        # 3. invariants
        cov = res.coverage.cpu()
        assert float(cov.min()) >= 0.0 and float(cov.max()) <= 1.0 + 1e-6
        lo, hi = dense_dl.amin(1, keepdim=True)[:, None], dense_dl.amax(1, keepdim=True)[:, None]   # per pixel's row
        d = res.disp.cpu()
        assert bool((d >= lo * (1 - 1e-5)).all()) and bool((d <= hi * (1 + 1e-5)).all())
        # 1. against the oracle
        for v, s in enumerate(baselines):
            rgb, coverage, disp = _oracle(key, case, s)
            errs = (rel_err(res.rgb[:, v].cpu(), rgb), rel_err(res.coverage[:, v].cpu(), coverage),
                    rel_err(res.disp[:, v].cpu(), disp))
            print("s = %+.2f in %s: rel_err vs oracle rgb %.3g coverage %.3g disp %.3g" % ((s, baselines) + errs))
            assert max(errs) < TOL, (s, baselines, errs)
    # 3. a baseline of zero is the source camera, on the rows where no plane is masked (a masked plane keeps logit 0 and a weight
    # in the softmax but contributes no colour: the reference's quirk, which the oracle comparison above covers)
    clear = dense_pm.amin(1).bool()[:, None]                      # [B,1,H,W]
    zero = got[(0.0,)]
    img = case["cpu"]["image"]
    err_img = float(((zero.rgb[:, 0].cpu() - img).abs() * clear).max() / img.abs().max())
    err_cov = float(((zero.coverage[:, 0].cpu() - 1.0).abs() * clear).max())
    print("s = 0: rgb vs image %.3g, |coverage - 1| %.3g" % (err_img, err_cov))
    assert err_img <= 1e-4 and err_cov <= 1e-4
    # 2. against the product's own training route
    for s, side in ((1.0, "r"), (-1.0, "l")):
        err = rel_err(got[(s,)].rgb[:, 0], _training_route(case, side))
        print("s = %+d: rel_err vs decoder_tail + plane_sweep_disp %.3g" % (s, err))
        assert err < TRAIN_TOL, (s, err)
    # 4. launch independence, bit for bit: alone, among four, in the chunked call of five (first and second chunk)
    four, five = got[SETS[4]], got[SETS[5]]
    for s in (1.0, -1.0):
        alone = got[(s,)]
        for other, v in ((four, SETS[4].index(s)), (five, SETS[5].index(s))):
            for a, b in zip(alone, other):
                assert torch.equal(a[:, 0], b[:, v]), (s, v)
    for a, b, c in zip(got[SETS[3]], four, five):
        assert torch.equal(a[:, 0], c[:, SETS[5].index(0.5)])      # 0.5: first of two, third of the first chunk
        assert torch.equal(b[:, SETS[4].index(0.25)], c[:, SETS[5].index(0.25)])
    three_alone = _render(case, (3.0,))                            # the second chunk's only view
    for a, c in zip(three_alone, five):
        assert torch.equal(a[:, 0], c[:, 4])
    again = _render(case, SETS[4])
    for a, b in zip(four, again):
        assert torch.equal(a, b)


@pytest.mark.parametrize("rows", [False, True], ids=["plane", "rows"])
def test_every_output_element_is_written(rows):
    """5. The C entry called directly on NaN-filled outputs; with coverage and disp NULL only rgb is written (and is the same)."""
    shape = B, N, H, W = ROWS_SHAPE
    case = _case(shape, rows, True, False, False)
    baselines = (1.0, -0.5, 3.0)
    V = len(baselines)
    flags = C.PD_TAIL_MIXTURE | ((C.PD_TAIL_DISP_ROWS | C.PD_TAIL_MASK_ROWS) if rows else 0)
    dl = case["dl"][..., 0].contiguous() if rows else case["dl"][:, :, 0, 0].contiguous()
    pm = case["pm"][..., 0].contiguous() if rows else None
    arr = (ctypes.c_float * V)(*baselines)
    nan = lambda c: torch.full((B, V, c, H, W), float("nan"), device=DEV)   # noqa: E731
    rgb, coverage, disp = nan(3), nan(1), nan(1)
    C.call("pd_render_views", rgb.device, B, N, H, W, V, flags, case["rl"], case["rs"], pm, dl, case["image"], arr, rgb, coverage, disp)
    for t in (rgb, coverage, disp):
        assert not torch.isnan(t).any()
    only = nan(3)
    C.call("pd_render_views", rgb.device, B, N, H, W, V, flags, case["rl"], case["rs"], pm, dl, case["image"], arr, only, None, None)
    assert torch.equal(only, rgb)
    res = _render(case, baselines, want=())
    assert res.coverage is None and res.disp is None and torch.equal(res.rgb, rgb)
    assert _render(case, baselines, want="disp").coverage is None


def test_nothing_plane_sized_is_allocated():
    """6. Peak memory of the call beyond what was allocated before it: the outputs and nothing plane-sized (less than a quarter
    of one [B,N,H,W] fp32 tensor on top of them, which leaves room for the allocator's rounding of three tensors only); the
    training route under no_grad, which writes logits and sigma, is above a plane tensor — the probe sees the difference."""
    B, N, H, W = shape = (2, 9, 24, 80)
    plane_bytes = B * N * H * W * 4
    case = _case(shape, True, True, False, False)
    baselines = (1.0, -1.0, 0.25, 2.0)

    def peak(fn):
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        with torch.no_grad():
            out = fn()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - before, out

    fused, res = peak(lambda: _render(case, baselines))
    out_bytes = sum(t.numel() * t.element_size() for t in res)
    train, _ = peak(lambda: _training_route(case, "r"))
    print("peak bytes beyond the inputs: render_views %d (outputs %d), training route %d, one plane tensor %d"
          % (fused, out_bytes, train, plane_bytes))
    assert out_bytes == B * len(baselines) * 5 * H * W * 4
    assert fused - out_bytes < plane_bytes // 4
    assert train > plane_bytes


class _Net(torch.nn.Module):
    """encoder + decoder stand-in that fills the outputs dict as the decoders do.  ``tail``: "keep" = the inference tail with
    ``keep_conv_outputs=True``, "infer" = the inference tail as it was, "stock" = the reference's torch tail."""
    NO_LEVELS, XZ_LEVELS = 5, 3

    def __init__(self, tail, mix=True, seed=1):
        super().__init__()
        n = self.NO_LEVELS + self.XZ_LEVELS
        self.tail, self.mix = tail, mix
        self.body = torch.nn.Conv2d(3, 12, 3, padding=1)
        self.dispconv = torch.nn.Conv2d(12, n, 3, padding=1)
        self.sigmaconv = torch.nn.Conv2d(12, n, 3, padding=1)
        g = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            for p in self.parameters():
                p.copy_(torch.randn(p.shape, generator=g) * (0.5 if p.dim() > 1 else 0.1))
        self.outputs = None

    def forward(self, x, grids):
        outputs = {}
        f = torch.relu(self.body(x))
        DT.fused_plane_geometry(outputs, grids, None, no_levels=self.NO_LEVELS, xz_levels=self.XZ_LEVELS, disp_min=0.5,
                                disp_max=20.0, xz_min=0.1852, xz_max=0.3704)
        raw_logits, raw_sigma = self.dispconv(f), self.sigmaconv(f)
        if self.tail == "stock":      # networks/depth_decoder.py:256-291
            mask, dl = outputs["padding_mask"], outputs["disp_layered"]
            outputs["logits"] = logits = raw_logits * mask
            prob = torch.softmax(logits.float(), 1)
            if self.mix:
                outputs["sigma"] = sigma = torch.clamp(torch.sigmoid(raw_sigma), 0.01, 1.0)
                weights = prob / sigma.float() * mask
                prob = weights / weights.sum(1, True)
            outputs["probability"] = prob
            outputs["disp"] = (prob * dl).sum(1, True)
        else:
            DT.fused_decoder_tail_inference(outputs, raw_logits, raw_sigma if self.mix else None, use_mixture_loss=self.mix,
                                            **({"keep_conv_outputs": True} if self.tail == "keep" else {}))
        self.raw = (raw_logits, raw_sigma if self.mix else None)
        self.outputs = outputs
        return outputs


@pytest.mark.parametrize("mix", [True, False], ids=["mix", "pi"])
@pytest.mark.parametrize("autocast", [False, True], ids=["fp32", "autocast"])
def test_predict_render(mix, autocast):
    """7. predict.render against render_views called directly, from the kept conv outputs and from a stock tail's logits /
    sigma; predict() itself is unchanged by the new keyword's default."""
    M, H, W = 2, 16, 48
    g = torch.Generator().manual_seed(4)
    images = torch.rand(M, 3, H, W, generator=g).to(DEV)
    baselines = (1.0, -1.0, 0.5)
    keep, plain, stock = (_Net(t, mix).to(DEV).eval() for t in ("keep", "infer", "stock"))

    views, pred = planedepth_amd.predict.render(keep, images, baselines, autocast=autocast)
    out = keep.outputs
    assert out["raw_logits"] is keep.raw[0] and (out["raw_sigma"] is keep.raw[1] if mix else "raw_sigma" not in out)
    assert out["raw_logits"].dtype == (BF if autocast else torch.float32)
    assert not ({"logits", "sigma", "pi"} & set(out))
    with torch.no_grad():
        direct = ops.render_views(out["raw_logits"], out.get("raw_sigma"), out["padding_mask"], out["disp_layered"], images,
                                  baselines, use_mixture_loss=mix)
    for a, b in zip(views, direct):
        assert a.shape[:2] == (M, len(baselines)) and torch.equal(a, b)

    # the keyword's default changes nothing: no new keys, the same prediction
    base = planedepth_amd.predict(plain, images, autocast=autocast)
    assert "raw_logits" not in plain.outputs and "raw_sigma" not in plain.outputs
    assert set(plain.outputs) == set(out) - {"raw_logits", "raw_sigma"}
    for a, b in zip(pred, base):
        assert torch.equal(a, b)
    for a, b in zip(planedepth_amd.predict(keep, images, autocast=autocast), base):
        assert torch.equal(a, b)

    # a stock tail's outputs["logits"] / ["sigma"]: tail_applied
    views_s, pred_s = planedepth_amd.predict.render(stock, images, baselines, autocast=autocast)
    so = stock.outputs
    lg, sg = so["logits"], so.get("sigma")
    if mix and autocast:   # logits * mask is fp32, sigma bf16: render widens both
        assert lg.dtype == torch.float32 and sg.dtype == BF
        lg, sg = lg.float(), sg.float()
    with torch.no_grad():
        direct_s = ops.render_views(lg, sg, so["padding_mask"], so["disp_layered"], images, baselines, use_mixture_loss=mix,
                                    tail_applied=True)
    for a, b in zip(views_s, direct_s):
        assert torch.equal(a, b)
    assert torch.equal(pred_s.raw_disp, so["disp"][:, 0])
    if not autocast:   # fp32: the stock tail's logits / sigma are the kept conv outputs after the tail step (a different rounding order only)
        assert rel_err(views_s.rgb, views.rgb) < TRAIN_TOL
