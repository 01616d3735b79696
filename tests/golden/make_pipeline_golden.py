"""Generate tests/golden/pipeline_aug.npz (the vectors of tests/test_input_pipeline.py) with the REFERENCE's own transforms
(datasets/pair_transforms.py: RandomResizeCrop, Resize, RandomGamma, RandomBrightness, RandomColorBrightness), driven the way
datasets/mono_dataset.py:149-187 drives them.

Run where the reference tree is present:

    python tests/golden/make_pipeline_golden.py            # writes the fixture
    python tests/golden/make_pipeline_golden.py --check    # writes nothing: re-runs the reference against the committed file

Per case the script seeds ``random`` and ``numpy.random``, and per sample it draws the flip itself (``random.random() > 0.5``, as
``__getitem__`` does), fills the dict in ``__getitem__``'s insertion order (mirrored frames under the flip, the left file under the
key ``r``), converts the uint8 frames as ToTensor does and applies the reference's transform objects in ``data_aug``'s order
(``no_data_aug``'s for the evaluation case).  The module functions the reference draws from (``random.random`` / ``uniform`` /
``randint``, ``numpy.random.uniform``) are wrapped while it runs, so every draw is logged in order.  Seeds are scanned until the
first sample of a case shows the wanted combination of flip and stages.  The file holds the seeds, the frames, the logged draws and
every output tensor: arrays and a JSON ``meta`` only.
"""
import contextlib
import importlib
import json
import os
import random
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from ref_import import load_reference  # noqa: E402

OUT = os.path.join(HERE, "pipeline_aug.npz")
H, W = 8, 16
B = 2            # samples per case: consecutive __getitem__ calls on one random stream
GAMMA, BRIGHTNESS, CHANNEL, FLIP = 1, 2, 4, 8
# tag -> frame size, novel frame ids, train, use_crop, depth_gt, and what the FIRST sample must draw: flip, stage bits (None: any)
CASES = (
    ("all_on", dict(src_hw=(23, 41), novel=[], train=True, use_crop=True, depth=False, flip=False, stages=7)),
    ("all_off", dict(src_hw=(20, 37), novel=[], train=True, use_crop=True, depth=False, flip=False, stages=0)),
    ("flip_v4", dict(src_hw=(11, 19), novel=[-1, 1], train=True, use_crop=True, depth=False, flip=True, stages=7)),
    ("resize", dict(src_hw=(11, 19), novel=[], train=True, use_crop=False, depth=False, flip=None, stages=7)),
    ("depth_flip", dict(src_hw=(20, 37), novel=[], train=True, use_crop=True, depth=True, flip=True, stages=None)),
    ("depth_v4", dict(src_hw=(11, 19), novel=[-1, 1], train=True, use_crop=True, depth=True, flip=False, stages=5)),
    ("eval", dict(src_hw=(11, 19), novel=[], train=False, use_crop=True, depth=True, flip=None, stages=None)),
)


@contextlib.contextmanager
def logged_draws(log):
    """Wrap the module-level functions the reference draws from; every call appends (name, value) to ``log``."""
    saved = (random.random, random.uniform, random.randint, np.random.uniform)

    def wrap(name, fn):
        def inner(*a, **k):
            v = fn(*a, **k)
            log.append([name, float(v) if name != "randint" else int(v)])
            return v
        return inner
    random.random, random.uniform = wrap("random", saved[0]), wrap("uniform", saved[1])
    random.randint, np.random.uniform = wrap("randint", saved[2]), wrap("np.uniform", saved[3])
    try:
        yield
    finally:
        random.random, random.uniform, random.randint, np.random.uniform = saved


def case_inputs(index, spec):
    """White-noise uint8 frames [B,V,hs,ws,3] in file order (left, right, novel...) and sparse depth maps [B,2,hs,ws]."""
    rng = np.random.RandomState(9000 + index)
    hs, ws = spec["src_hw"]
    V = 2 + len(spec["novel"])
    frames = rng.randint(0, 256, size=(B, V, hs, ws, 3)).astype(np.uint8)
    depth = (rng.uniform(1.0, 80.0, size=(B, 2, hs, ws)) * (rng.uniform(size=(B, 2, hs, ws)) < 0.4)).astype(np.float32)
    return frames, depth


def run_sample(pt, spec, frames, depth, log):
    """One __getitem__ (mono_dataset.py:149-187) on decoded frames: the flip, the dict in insertion order, the transform chain."""
    def to_tensor(u8):   # torchvision's ToTensor on an HWC uint8 image
        return torch.from_numpy(np.ascontiguousarray(u8)).permute(2, 0, 1).float().div(255)
    with logged_draws(log):
        do_flip = spec["train"] and random.random() > 0.5
        keys = (["r", "l"] if do_flip else ["l", "r"]) + list(spec["novel"])
        inputs = {}
        for v, key in enumerate(keys):   # get_color(..., do_flip): the PIL transpose
            inputs[("color", key, -1)] = to_tensor(frames[v][:, ::-1] if do_flip else frames[v])
        if spec["depth"]:
            for v, key in enumerate(keys[:2]):   # get_depth(..., do_flip): np.fliplr
                d = np.fliplr(depth[v]) if do_flip else depth[v]
                inputs[("depth_gt", key)] = torch.from_numpy(np.expand_dims(np.ascontiguousarray(d), 0).astype(np.float32))
        resize = pt.Resize((H, W))
        if spec["train"]:
            chain = [pt.RandomResizeCrop((H, W), factor=(0.75, 1.5)) if spec["use_crop"] else resize,
                     pt.RandomGamma(min=0.8, max=1.2), pt.RandomBrightness(min=0.5, max=2.0),
                     pt.RandomColorBrightness(min=0.8, max=1.2)]
        else:
            chain = [resize]
        for step in chain:
            inputs = step(inputs)
    out = {"grid": inputs["grid"]}
    for key in keys:
        out["color_%s" % key] = inputs[("color", key)]
        out["color_aug_%s" % key] = inputs[("color_aug", key)]
    if spec["depth"]:
        out["depth_gt_l"], out["depth_gt_r"] = inputs[("depth_gt", "l")], inputs[("depth_gt", "r")]
    return do_flip, {k: v.detach().clone().numpy() for k, v in out.items()}


def run_case(pt, spec, frames, depth, seed):
    """B consecutive samples under one seed -> (per-sample flips, stacked outputs, per-sample draw logs)."""
    random.seed(seed)
    np.random.seed(seed)
    flips, outs, logs = [], [], []
    for b in range(B):
        log = []
        flip, out = run_sample(pt, spec, frames[b], depth[b], log)
        flips.append(bool(flip))
        outs.append(out)
        logs.append(log)
    return flips, {k: np.stack([o[k] for o in outs]) for k in outs[0]}, logs


def stage_bits(spec, log):
    """The stages the first sample drew, read off its log by position (coins are 'random' entries < 0.5 after the geometry)."""
    from pipeline_cases import logged_params
    case = dict(V=2 + len(spec["novel"]), H=H, W=W, src_hw=spec["src_hw"], train=spec["train"], use_crop=spec["use_crop"],
                log=[log])
    return logged_params(case)[0][2] & 7


def reference_case(pt, index, tag, spec, seed=None):
    """(meta entry, arrays) of one case; ``seed=None`` scans for the first seed whose first sample shows the wanted draws."""
    frames, depth = case_inputs(index, spec)
    seeds = [seed] if seed is not None else range(100 * index, 100 * index + 5000)
    for s in seeds:
        flips, out, logs = run_case(pt, spec, frames, depth, s)
        if seed is not None or ((spec["flip"] is None or flips[0] == spec["flip"])
                                and (spec["stages"] is None or not spec["train"] or stage_bits(spec, logs[0]) == spec["stages"])):
            break
    else:
        raise RuntimeError("no seed gives case %s" % tag)
    arrays = {"frames": frames}
    if spec["depth"]:
        arrays["depth"] = depth
    arrays.update(out)
    meta = dict(seed=s, B=B, V=frames.shape[1], H=H, W=W, src_hw=list(spec["src_hw"]), novel=spec["novel"], train=spec["train"],
                use_crop=spec["use_crop"], depth=spec["depth"], flips=flips, log=logs)
    return meta, arrays


def reference_outputs(tag, seed):
    """Re-run the reference for one committed case (tests/test_input_pipeline.py: the live check)."""
    load_reference()
    pt = importlib.import_module("datasets.pair_transforms")
    index = [t for t, _ in CASES].index(tag)
    return reference_case(pt, index, tag, CASES[index][1], seed)


def main():
    load_reference()
    pt = importlib.import_module("datasets.pair_transforms")
    meta, out = dict(cases={}), {}
    for index, (tag, spec) in enumerate(CASES):
        m, arrays = reference_case(pt, index, tag, spec)
        meta["cases"][tag] = m
        out.update({"%s/%s" % (tag, k): v for k, v in arrays.items()})
        print("%-10s seed %4d  flips %s  draws %s" % (tag, m["seed"], m["flips"], [len(l) for l in m["log"]]))
    if "--check" in sys.argv:
        z = np.load(OUT)
        assert json.loads(str(z["meta"])) == json.loads(json.dumps(meta)), "meta differs"
        for k, v in out.items():
            err = float(np.abs(z[k].astype(np.float64) - v.astype(np.float64)).max())
            assert err <= (0 if v.dtype == np.uint8 or "depth" in k else 1e-6), (k, err)
        print("pipeline_aug.npz agrees with the reference on this host")
        return
    np.savez_compressed(OUT, meta=np.asarray(json.dumps(meta)), **out)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
