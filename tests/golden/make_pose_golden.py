"""Generate tests/golden/pose_chain.npz (the vectors of tests/test_pose_tail_abi.py and tests/test_pose_tail.py) with the REFERENCE's
own pose path: the tail of ``networks.PoseDecoder.forward`` (networks/pose_net.py:148-155) and ``Trainer.predict_poses``
(trainer.py:358-402), in fp32 on the CPU.

Run where the reference tree is present:

    python tests/golden/make_pose_golden.py            # writes the fixture
    python tests/golden/make_pose_golden.py --check    # writes nothing: re-runs the reference against the committed file

The pose decoder is the reference's class with its convolutions replaced by identities, so that line 147's ``out`` IS the stored conv
output and lines 148-155 run as written; the pose encoder is a stub that hands that tensor over (as make_golden.py's PoseStub
does for the axis-angles).  ``novel_frame_ids = [-1, 1]`` gives ``invert`` both ways; sample 0 of the batch is an uncropped frame
(Resize grid), samples 1 and 2 are crops of a resized frame (RandomResizeCrop grids).  A second run takes the COLMAP branch on a
stored ``Rt``.  Stored per frame: the conv output ``x``, the ``outputs`` entries, a random ``W`` and the reference's gradient of
``sum(W * Rt_Rc)`` w.r.t. ``x`` and the axis-angle.  ``meta["E_ref"]``: the reference's fp32 distance from the fp64 restatement of
tests/test_pose_tail_abi.py (``block_err``), per tensor, the worst over the frames.  Arrays and a JSON ``meta`` only.
"""
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from ref_import import load_reference  # noqa: E402

from planedepth_amd.synthetic import crop_grid  # noqa: E402

OUT = os.path.join(HERE, "pose_chain.npz")
B, H, W = 3, 6, 20          # the conv output at 192 x 640
GH, GW = 8, 12              # the grid's size does not matter: four corners are read
NOVEL = [-1, 1]
SEED = 20


def grids():
    return torch.stack([crop_grid(GH, GW, GH, GW, 0, 0),          # Resize: the whole frame
                        crop_grid(GH, GW, 13, 19, 3, 5),          # RandomResizeCrop: a window of a larger resized frame
                        crop_grid(GH, GW, 11, 31, 0, 17)], 0)


def conv_outputs(gen):
    """Per frame a [B,6,H,W] conv output: noise around per-channel offsets, so that 0.01 * mean is a pose of a few hundredths."""
    return {f: (torch.randn(B, 6, H, W, generator=gen) * 2 + torch.randn(B, 6, 1, 1, generator=gen) * 4) for f in NOVEL}


def identity_decoder(ref):
    dec = ref.networks.PoseDecoder([6], num_input_features=1, num_frames_to_predict_for=1, num_ep=0)
    for key in list(dec.convs):
        dec.convs[key] = torch.nn.Identity()
    dec.relu = torch.nn.Identity()
    return dec


def run_reference(ref, x, grid, W_, colmap_Rt):
    out = {}
    leafs = {f: x[f].clone().requires_grad_(True) for f in NOVEL}
    ns = types.SimpleNamespace()
    ns.opt = types.SimpleNamespace(novel_frame_ids=NOVEL, use_colmap=False)
    # predict_poses walks the frames in order and calls the encoder once per frame: the stub hands out the leafs in that order
    order = iter(NOVEL)
    ns.models = {"pose_encoder": lambda images: [leafs[next(order)]], "pose": identity_decoder(ref)}
    color = torch.zeros(B, 3, 2, 2)
    inputs = {"grid": grid, ("Rt", "r"): torch.eye(4)[None].repeat(B, 1, 1), ("color_aug", "l"): color}
    for f in NOVEL:
        inputs[("color_aug", f)] = color
    outputs = ref.trainer.Trainer.predict_poses(ns, inputs)
    assert outputs[("Rt", "r")] is inputs[("Rt", "r")]
    for f in NOVEL:
        aa = outputs[("axisangle", f)]
        aa.retain_grad()
        (outputs[("Rt", f)] * W_[f]).sum().backward()
        out["x/%d" % f] = x[f]
        out["W/%d" % f] = W_[f]
        out["axisangle/%d" % f] = aa.detach()
        out["translation/%d" % f] = outputs[("translation", f)].detach()
        out["Rc/%d" % f] = outputs[("Rc", f)].detach()
        out["Rt/%d" % f] = outputs[("Rt", f)].detach()
        out["g_x/%d" % f] = leafs[f].grad.clone()
        out["g_axisangle/%d" % f] = aa.grad.clone()
    ns.opt.use_colmap = True
    inputs[("Rt", 1)] = colmap_Rt
    ns.opt.novel_frame_ids = [1]
    outputs = ref.trainer.Trainer.predict_poses(ns, inputs)
    out["colmap/Rt_in"], out["colmap/Rc"], out["colmap/Rt"] = colmap_Rt, outputs[("Rc", 1)].detach(), outputs[("Rt", 1)].detach()
    return out


def measure_e_ref(out, grid):
    from test_pose_tail_abi import block_err, chain_grads64, colmap64
    e = {}
    for f in NOVEL:
        o64, g64 = chain_grads64(out["x/%d" % f], grid, f < 0, out["W/%d" % f])
        for k, (ref32, mine) in dict(axisangle=(out["axisangle/%d" % f].view(B, 3), o64["axisangle"]),
                                     translation=(out["translation/%d" % f].view(B, 3), o64["translation"]),
                                     Rc=(out["Rc/%d" % f], o64["Rc"]), Rt=(out["Rt/%d" % f], o64["Rt_Rc"]),
                                     g_x=(out["g_x/%d" % f], g64)).items():
            e[k] = max(e.get(k, 0.0), block_err(ref32, mine))
    c64 = colmap64(out["colmap/Rt_in"], grid)
    e["colmap_Rc"] = block_err(out["colmap/Rc"], c64["Rc"])
    e["colmap_Rt"] = block_err(out["colmap/Rt"], c64["Rt_Rc"])
    return e


def main():
    from planedepth_amd.synthetic import small_pose
    ref = load_reference()
    gen = torch.Generator().manual_seed(SEED)
    grid = grids()
    x = conv_outputs(gen)
    W_ = {f: torch.randn(B, 4, 4, generator=gen) for f in NOVEL}
    colmap_Rt = small_pose(gen, B, rot=0.05, trans=0.3)
    out = run_reference(ref, x, grid, W_, colmap_Rt)
    out["grid"] = grid
    e_ref = measure_e_ref(out, grid)
    meta = dict(B=B, hw=[H, W], novel_frame_ids=NOVEL, seed=SEED, E_ref=e_ref)
    for k, v in sorted(e_ref.items()):
        print("E_ref %-12s %.3e" % (k, v))
    arrays = {k: v.detach().numpy() for k, v in out.items()}
    if "--check" in sys.argv:
        z = np.load(OUT)
        for k, v in arrays.items():
            err = float(np.abs(z[k].astype(np.float64) - v.astype(np.float64)).max())
            assert err <= 1e-6 * max(1.0, float(np.abs(v).max())), (k, err)
        print("pose_chain.npz agrees with the reference on this host")
        return
    np.savez_compressed(OUT, meta=np.asarray(json.dumps(meta)), **arrays)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
