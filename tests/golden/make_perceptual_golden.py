"""Generate tests/golden/perceptual.npz (the vectors of tests/test_feature_distance.py) with the REFERENCE's own
``Trainer.perceptual_loss`` (trainer.py:672-685).

Run where the reference tree is present:

    python tests/golden/make_perceptual_golden.py            # writes the fixture
    python tests/golden/make_perceptual_golden.py --check    # writes nothing: re-runs the reference against the committed file

The method is called unbound on the stub ``self`` of ref_import.make_trainer_namespace (whose own ``perceptual_loss`` stub is
not used: the class's method is called directly), with a seeded three-level convolutional stand-in as ``pc_net`` — the
pretrained VGG weights are not available, and the distance does not care which frozen net made the features.  Stored: the
features the stand-in produced for the three images, the loss and the gradient with respect to the prediction's features, with
and without a source image.  Only data is written.
"""
import json
import os
import sys

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from ref_import import load_reference, make_trainer_namespace  # noqa: E402

OUT = os.path.join(HERE, "perceptual.npz")
B, H, W = 2, 12, 20
CHANNELS = (8, 16, 32)     # levels [2,8,12,20], [2,16,6,10], [2,32,3,5]


class StandInNet(nn.Module):
    """Three feature levels at H, H/2, H/4 (conv + ReLU on the image pooled 0, 1 and 2 times); frozen.  The levels are separate
    branches of the image rather than a chain, so that the gradient autograd leaves on a level is the distance's own (in a chain,
    level 0 would also collect what flows back from levels 1 and 2)."""

    def __init__(self, seed=3):
        super().__init__()
        torch.manual_seed(seed)
        c1, c2, c3 = CHANNELS
        self.slice1 = nn.Sequential(nn.Conv2d(3, c1, 3, padding=1), nn.ReLU())
        self.slice2 = nn.Sequential(nn.AvgPool2d(2), nn.Conv2d(3, c2, 3, padding=1), nn.ReLU())
        self.slice3 = nn.Sequential(nn.AvgPool2d(4), nn.Conv2d(3, c3, 3, padding=1), nn.ReLU())
        for p in self.parameters():
            p.requires_grad = False
        self.seen = []     # the feature tuples handed out, in call order

    def forward(self, x):
        f1 = self.slice1(x)
        f2 = self.slice2(x)
        f3 = self.slice3(x)
        for f in (f1, f2, f3):
            if f.requires_grad:
                f.retain_grad()
        self.seen.append((f1, f2, f3))
        return f1, f2, f3


def make_images(seed=21):
    g = torch.Generator().manual_seed(seed)
    target = torch.rand(B, 3, H, W, generator=g)
    pred = (target + 0.15 * torch.randn(B, 3, H, W, generator=g)).clamp(0, 1)
    source = (target + 0.15 * torch.randn(B, 3, H, W, generator=g)).clamp(0, 1)
    return pred, target, source


def reference_outputs():
    ref = load_reference()
    out = {}
    for tag, with_source in (("plain", False), ("auto", True)):
        ns = make_trainer_namespace(ref, H, W)
        ns.pc_net = StandInNet()
        pred, target, source = make_images()
        pred.requires_grad_(True)
        loss = ref.trainer.Trainer.perceptual_loss(ns, pred, target, source if with_source else None)
        loss.backward()
        feats = ns.pc_net.seen
        assert len(feats) == (3 if with_source else 2)
        out["loss_" + tag] = loss.detach().numpy().astype(np.float32)
        for i in range(3):
            out["g_%s_%d" % (tag, i)] = feats[0][i].grad.numpy().copy()
            out["pred_f%d" % i] = feats[0][i].detach().numpy().copy()
            out["target_f%d" % i] = feats[1][i].detach().numpy().copy()
            if with_source:
                out["source_f%d" % i] = feats[2][i].detach().numpy().copy()
    out["meta"] = np.frombuffer(json.dumps({"B": B, "H": H, "W": W, "channels": list(CHANNELS), "levels": 3,
                                            "reference": "trainer.py:672-685 Trainer.perceptual_loss"}).encode(), np.uint8)
    return out


def main():
    out = reference_outputs()
    if "--check" in sys.argv:
        z = np.load(OUT)
        assert sorted(z.files) == sorted(out), (sorted(z.files), sorted(out))
        for k, v in out.items():
            if k != "meta":
                assert np.allclose(z[k], v, rtol=1e-6, atol=1e-9), k   # (another host's convolutions may differ in the last bits)
        assert bytes(z["meta"]) == bytes(out["meta"])
        print("check: %s is current" % OUT)
        return
    np.savez_compressed(OUT, **out)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
