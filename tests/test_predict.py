"""planedepth_amd.predict on the GPU with a stand-in network: a small seeded conv stack whose head is fused_plane_geometry +
fused_decoder_tail_inference, against its twin that keeps the training tail (fused_decoder_tail)."""
import numpy as np
import pytest
import torch

import planedepth_amd
from planedepth_amd import decoder_tail as DT
from planedepth_amd import metrics

pytestmark = pytest.mark.gpu
DEV = "cuda"
M, H, W = 2, 32, 64
NO_LEVELS, XZ_LEVELS = 5, 3


class _Net(torch.nn.Module):
    """encoder + decoder stand-in: ``model(images, grids) -> outputs``.  ``inference`` picks the tail; the weights are the seed's."""

    def __init__(self, inference, seed=1):
        super().__init__()
        n = NO_LEVELS + XZ_LEVELS
        self.inference = inference
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
        DT.fused_plane_geometry(outputs, grids, None, no_levels=NO_LEVELS, xz_levels=XZ_LEVELS, disp_min=0.5, disp_max=20.0,
                                xz_min=0.1852, xz_max=0.3704)
        tail = DT.fused_decoder_tail_inference if self.inference else DT.fused_decoder_tail
        tail(outputs, self.dispconv(f), self.sigmaconv(f), use_mixture_loss=True)
        self.outputs = outputs
        return outputs


@pytest.fixture(scope="module")
def scene():
    g = torch.Generator().manual_seed(2)
    images = torch.rand(M, 3, H, W, generator=g).to(DEV)
    gt = torch.rand(M, 40, 100, generator=g) * 58.0 + 2.0
    gt[torch.rand(M, 40, 100, generator=g) > 0.3] = 0.0       # sparse, LiDAR-like
    return images, metrics.pack_gt(gt.to(DEV), "eigen_raw"), _Net(True).to(DEV).eval(), _Net(False).to(DEV).eval()


@pytest.mark.parametrize("autocast", [False, True], ids=["fp32", "autocast"])
@pytest.mark.parametrize("post_process", [False, True], ids=["single", "post_process"])
def test_predict_matches_the_training_tail(scene, post_process, autocast):
    images, gt, net, twin = scene
    got = planedepth_amd.predict(net, images, post_process=post_process, autocast=autocast)
    ref = planedepth_amd.predict(twin, images, post_process=post_process, autocast=autocast)
    passes = 2 * M if post_process else M
    assert got.raw_disp.shape == (passes, H, W) and got.disp.shape == (M, 1, H, W) and got.depth.shape == (M, 1, H, W)
    assert got.confidence.shape == (passes, 1, H, W) and got.mean_confidence.shape == (passes,)
    for t in got:
        assert t.dtype == torch.float32 and not t.requires_grad
    # the inference tail wrote nothing plane-sized, and nobody touched the lazy probability
    out = net.outputs
    assert not ({"logits", "sigma", "pi", "dists"} & set(out)) and out["probability"]._value is None
    assert out["probability"].shape == (passes, NO_LEVELS + XZ_LEVELS, H, W)
    assert out["plane_index"].dtype == torch.int32 and out["disp_best"].shape == (passes, 1, H, W)
    if autocast:
        assert twin.outputs["logits"].dtype == torch.bfloat16
    # the same disparities as the training tail, bit for bit
    assert torch.equal(got.raw_disp, ref.raw_disp)
    assert torch.equal(got.raw_disp, out["disp"][:, 0])
    # contract A1 of metrics: 0.5f * (d[:M] + fliplr(d[M:]))
    raw = got.raw_disp
    a1 = 0.5 * (raw[:M] + raw[M:].flip(-1)) if post_process else raw
    assert torch.equal(got.disp[:, 0], a1)
    assert torch.equal(got.depth, torch.tensor(np.float32(0.1 * 0.58 * W), device=DEV) / got.disp)
    # probabilities_max of evaluate_depth_HR.py:168 from the twin's materialised probability
    want = twin.outputs["probability"].amax(1).mean((-1, -2))
    err = float((got.mean_confidence - want).abs().max())
    print("mean_confidence: |vs probability.amax(1).mean| %.3g" % err)
    assert err <= 5e-6
    assert float((got.confidence - twin.outputs["probability"].amax(1, keepdim=True)).abs().max()) <= 5e-6
    # the evaluation takes raw_disp as it is
    e_got = metrics.eval_depth_errors(got.raw_disp, gt, width=W, post_process=post_process)
    e_ref = metrics.eval_depth_errors(ref.raw_disp, gt, width=W, post_process=post_process)
    assert e_got.metrics.shape == (M, 7) and bool(torch.isfinite(e_got.metrics).all())
    assert torch.equal(e_got.metrics, e_ref.metrics)
