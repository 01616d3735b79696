"""Generate tests/golden/grid_embedding.npz (the vectors of tests/test_grid_embedding.py) with the REFERENCE's own networks:
``DepthDecoder`` (ResNet-18 channels, ``num_ep=8``, ``pe_type="neural"``, no DenseASPP) and ``PoseDecoder(num_ep=8)``, run through
their real ``forward`` on the CPU.

Run where the reference tree is present:

    python tests/golden/make_embedding_golden.py            # writes the fixture
    python tests/golden/make_embedding_golden.py --check    # writes nothing: re-runs the reference against the committed file

Inputs: seeded features of a 32x64 image, B = 2; the grid of the first sample is a crop window of linspace(-1, 1), the second sample's is
the first's flipped as ``add_flip_right_inputs`` flips it (trainer.py:258-260).  While ``forward`` runs, ``F.interpolate`` is wrapped
and every bilinear call made on the E-channel embedding is recorded: sizes, order and values are the reference's.  The gradients of a
seeded random linear functional of the recorded maps with respect to the ``epconv`` parameters are recorded too.  Two more cases go
through ``layers.get_embedder(2)`` and through the raw grid (networks/plade_net.py:150-158), resampled by ``F.interpolate`` as the
decoders call it.  The file holds arrays and a JSON ``meta`` only.

The deepest feature of a 32x64 image has one row, which the trunk's ``ReflectionPad2d(1)`` (layers.py:123) refuses; while ``forward``
runs, a reflect padding of a one-row or one-column tensor is therefore served as a replicate padding.  That touches the trunk's 3x3
convolutions only: the recorded maps and their gradients depend on ``epconv`` and ``F.interpolate`` alone.
"""
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from ref_import import load_reference  # noqa: E402

OUT = os.path.join(HERE, "grid_embedding.npz")
B, H, W, NUM_EP = 2, 32, 64, 8
CH_ENC = (64, 64, 128, 256, 512)           # ResNet-18
EXTRA_SIZES = ((1, 2), (5, 9), (16, 32), (32, 64))   # of the Embedder and the raw-grid case


def make_grid():
    """[2,2,32,64]: a crop window of a 83 x 45 resize, and its flip_right twin."""
    full_w, full_h, w0, h0 = 83, 45, 11, 6
    g = torch.empty(1, 2, H, W)
    g[0, 0] = torch.linspace(-1, 1, full_w)[w0:w0 + W][None, :]
    g[0, 1] = torch.linspace(-1, 1, full_h)[h0:h0 + H][:, None]
    flipped = g.clone()
    flipped[:, 0, :, :] *= -1.
    flipped = flipped.flip(-1)
    return torch.cat([g, flipped], dim=0)


def make_features(seed):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(B, c, H >> (i + 1), W >> (i + 1), generator=gen) for i, c in enumerate(CH_ENC)]


class Recorder:
    """Wraps torch.nn.functional.interpolate: every bilinear call on a ``channels``-channel input is kept (the live tensors)."""

    def __init__(self, channels):
        self.channels, self.calls = channels, []

    def __enter__(self):
        self.saved, self.saved_pad = F.interpolate, F.pad

        def pad(input, pad, mode="constant", value=None):   # see the module docstring: one-row features under ReflectionPad2d(1)
            if mode == "reflect" and min(input.shape[-2:]) < 2:
                mode = "replicate"
            return self.saved_pad(input, pad, mode, value)
        F.pad = pad

        def inner(input, *a, **k):
            out = self.saved(input, *a, **k)
            if k.get("mode") == "bilinear" and input.shape[1] == self.channels:
                assert k.get("align_corners") is True
                self.calls.append(out)
            return out
        F.interpolate = inner
        return self

    def __exit__(self, *exc):
        F.interpolate, F.pad = self.saved, self.saved_pad
        return False


def epconv_case(tag, epconv, run, seed):
    """Run ``run()`` (a forward of the module that owns ``epconv``) under the recorder -> arrays of the case."""
    with Recorder(NUM_EP) as rec:
        run()
    maps = rec.calls
    gen = torch.Generator().manual_seed(seed)
    functional = [torch.randn(m.shape, generator=gen) for m in maps]
    loss = sum((m * r).sum() for m, r in zip(maps, functional))
    params = (epconv[0].weight, epconv[0].bias, epconv[2].weight, epconv[2].bias)
    grads = torch.autograd.grad(loss, params)
    arrays = {}
    for name, p, g in zip(("w1", "b1", "w2", "b2"), params, grads):
        arrays["%s/%s" % (tag, name)] = p.detach().numpy().copy()
        arrays["%s/g_%s" % (tag, name)] = g.detach().numpy().copy()
    for l, (m, r) in enumerate(zip(maps, functional)):
        arrays["%s/map%d" % (tag, l)] = m.detach().numpy().copy()
        arrays["%s/functional%d" % (tag, l)] = r.numpy().copy()
    return dict(sizes=[list(m.shape[2:]) for m in maps], E=NUM_EP), arrays


def reference_outputs():
    """(meta, arrays) from the reference on this host."""
    ref = load_reference()
    grid = make_grid()
    meta, arrays = dict(B=B, H=H, W=W, cases={}), {"grid": grid.numpy().copy()}

    torch.manual_seed(11)
    decoder = ref.networks.DepthDecoder(np.array(CH_ENC), no_levels=5, num_ep=NUM_EP, pe_type="neural", use_denseaspp=False)
    feats = make_features(21)
    meta["cases"]["decoder"], a = epconv_case("decoder", decoder.convs["epconv"], lambda: decoder(feats, grid), 31)
    arrays.update(a)

    torch.manual_seed(12)
    pose = ref.networks.PoseDecoder(np.array(CH_ENC), num_input_features=1, num_frames_to_predict_for=1, num_ep=NUM_EP)
    pose_feats = make_features(22)
    meta["cases"]["pose"], a = epconv_case("pose", pose.convs["epconv"], lambda: pose([pose_feats], grid), 32)
    arrays.update(a)

    embedder = ref.layers.get_embedder(2)
    with torch.no_grad():
        emb = embedder(grid)
        for l, s in enumerate(EXTRA_SIZES):
            arrays["frequency/map%d" % l] = F.interpolate(emb, size=s, align_corners=True, mode="bilinear").numpy().copy()
            arrays["identity/map%d" % l] = F.interpolate(grid, size=s, align_corners=True, mode="bilinear").numpy().copy()
    kw = {k: v for k, v in embedder.kwargs.items() if k != "periodic_fns"}
    meta["cases"]["frequency"] = dict(sizes=[list(s) for s in EXTRA_SIZES], E=int(emb.shape[1]), multires=2, kwargs=kw)
    meta["cases"]["identity"] = dict(sizes=[list(s) for s in EXTRA_SIZES], E=2)
    return meta, arrays


def main():
    meta, arrays = reference_outputs()
    for tag, c in meta["cases"].items():
        print("%-10s E %2d  sizes %s" % (tag, c["E"], c["sizes"]))
    if "--check" in sys.argv:
        z = np.load(OUT)
        assert json.loads(str(z["meta"])) == json.loads(json.dumps(meta)), "meta differs"
        for k, v in arrays.items():
            err = float(np.abs(z[k].astype(np.float64) - v.astype(np.float64)).max())
            assert err <= 1e-6 * max(1.0, float(np.abs(v).max())), (k, err)
        print("grid_embedding.npz agrees with the reference on this host")
        return
    np.savez_compressed(OUT, meta=np.asarray(json.dumps(meta)), **arrays)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
