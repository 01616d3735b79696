"""Generate tests/golden/depth_eval.npz (the depth-evaluation vectors of tests/test_depth_eval.py) with the REFERENCE's own
metric functions.

Run where the reference tree is present:

    python tests/golden/make_eval_golden.py

The reference functions called: ``evaluate_depth_HR.compute_errors`` and ``batch_post_process_disparity``,
``Trainer.compute_depth_losses`` (on a stub ``self``, ``opt.no_stereo`` both ways) and, through it,
``layers.compute_depth_errors``.  What the reference does around them inline (resize, depth, masks, medians, clamps:
steps A1-A7 of planedepth_amd/metrics.py) comes from the restatement in tests/test_depth_eval.py.  Only data is written;
the GT is stored sparsely (flat indices + values).
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from ref_import import load_reference  # noqa: E402
from test_depth_eval import CONFIGS, config_name, cv2_resize, eval_mask, restate_trainer  # noqa: E402

F32 = np.float32
OUT = os.path.join(HERE, "depth_eval.npz")
WIDTH = 640
SHAPES = [(375, 1242), (40, 132), (37, 122), (38, 125), (41, 124), (40, 130)]   # the last two: empty set, NaN in the set
CLEAN = 4                                                                       # images with a finite metrics row
PRED_HW = (24, 80)
B_SHAPE = (3, 1, 40, 128)


def quantised(rng, n, lo, hi):
    return (np.round(rng.uniform(lo, hi, n) * 256) / 256).astype(F32)   # KITTI PNG depth: 1/256 m steps


def make_inputs(seed=11):
    rng = np.random.default_rng(seed)
    M = len(SHAPES)
    pred = rng.uniform(0.5, 60.0, (2 * M,) + PRED_HW).astype(F32)
    pred[1, 14:18, 20:27] = 0.0                  # zero disparity: infinite depth, clamped to 80
    pred[5, 10:14, 36:44] = np.nan               # a NaN reaches the median's set of the last image
    gts = []
    for i, (h, w) in enumerate(SHAPES):
        g = np.zeros((h, w), F32)
        density = 0.05 if i == 0 else (0.0 if i == 4 else 0.5 if i == 5 else 0.3)
        keep = rng.random((h, w)) < density
        g[keep] = quantised(rng, int(keep.sum()), 0.5, 90.0)
        gts.append(g)
    g = gts[2]   # the exact edge values inside the Eigen crop (and for the positive mask): 1e-3, 80, above 80, 0
    g[30, 20], g[30, 21], g[31, 22], g[31, 23], g[32, 24] = F32(1e-3), F32(80), F32(80.5), F32(0), F32(1e-3)
    # B: a "cropped" grid (pair_transforms' RandomResizeCrop): x from a per-image / per-row range, so one divisor per row
    Bn, _, H, W = B_SHAPE
    x0 = rng.uniform(-1.0, -0.6, (Bn, 1, H, 1)).astype(F32)
    x1 = rng.uniform(0.6, 1.0, (Bn, 1, H, 1)).astype(F32)
    t = np.linspace(0, 1, W, dtype=F32)[None, None, None, :]
    gx = x0 + (x1 - x0) * t
    gy = np.broadcast_to(np.linspace(-1, 1, H, dtype=F32)[None, None, :, None], gx.shape)
    grid = np.concatenate([gx, gy], 1).astype(F32)
    depth = rng.uniform(0.05, 30.0, B_SHAPE).astype(F32)
    gt_b = np.zeros(B_SHAPE, F32)
    keep = rng.random(B_SHAPE) < 0.3
    gt_b[keep] = quantised(rng, int(keep.sum()), 0.5, 90.0)
    fx = {"a_pred": pred, "a_width": np.int64(WIDTH), "a_clean": np.int64(CLEAN), "b_depth": depth, "b_grid": grid}
    # even pooled count for the trainer (so torch's lower median differs from numpy's)
    crop = np.zeros(B_SHAPE, bool)
    crop[:, :, int(0.40810811 * H):int(0.99189189 * H), int(0.03594771 * W):int(0.96405229 * W)] = True
    if ((gt_b > 0) & crop).sum() % 2:
        idx = np.argwhere((gt_b > 0) & crop)[0]
        gt_b[tuple(idx)] = 0
    fx["b_gt"] = gt_b
    fx["a_gt_shapes"] = np.array(SHAPES, np.int64)
    idx, val, ptr = [], [], [0]
    for g in gts:
        nz = np.flatnonzero(g)
        idx.append(nz.astype(np.int32))
        val.append(g.ravel()[nz])
        ptr.append(ptr[-1] + nz.size)
    fx["a_gt_idx"], fx["a_gt_val"], fx["a_gt_ptr"] = np.concatenate(idx), np.concatenate(val), np.array(ptr, np.int64)
    fx["gts"] = gts
    return fx


def _evaluate_module():
    load_reference()
    sys.modules["cv2"].setNumThreads = lambda n: None   # the stand-in cv2 (ref_import) only needs this at import
    import importlib
    return importlib.import_module("evaluate_depth_HR")


def reference_outputs(fx):
    """Every fixture output, from the reference functions plus the restatement's glue."""
    ref = load_reference()
    ev = _evaluate_module()
    gts = fx["gts"]
    M = len(gts)
    pred_disps = fx["a_pred"]
    out = {}
    for pp, mono, split in CONFIGS:
        c = config_name(pp, mono, split)
        disps = ev.batch_post_process_disparity(pred_disps[:M], pred_disps[M:, :, ::-1]) if pp else pred_disps[:M]
        scale = 1.0 if mono else ev.STEREO_SCALE_FACTOR
        errors, ratios, meds, counts = [], [], [], []
        for i in range(M):
            gt_depth = gts[i].copy()
            pred_disp = cv2_resize(disps[i].astype(F32), *gt_depth.shape)
            with np.errstate(divide="ignore", invalid="ignore"):
                pred_depth = 0.1 * 0.58 * WIDTH / pred_disp
            mask, gt_depth = eval_mask(gt_depth, split)
            pred_depth, gt_depth = pred_depth[mask], gt_depth[mask]
            pred_depth *= scale
            with np.errstate(divide="ignore", invalid="ignore"):
                if mono:
                    mg = np.median(gt_depth) if gt_depth.size else F32(np.nan)
                    md = np.median(pred_depth) if pred_depth.size else F32(np.nan)
                    ratio = mg / md
                    pred_depth *= ratio
                else:
                    mg = md = F32(np.nan)
                    ratio = F32(1)
                pred_depth[pred_depth < 1e-3] = 1e-3
                pred_depth[pred_depth > 80] = 80
                thresh = np.maximum(gt_depth / pred_depth, pred_depth / gt_depth)
                if gt_depth.size:
                    errors.append(np.array(ev.compute_errors(gt_depth, pred_depth), np.float64))
                else:
                    errors.append(np.full(7, np.nan))   # (compute_errors of an empty set: every mean is NaN)
            ratios.append(F32(ratio))
            meds.append((F32(mg), F32(md)))
            counts.append([gt_depth.size] + [int((thresh < 1.25 ** k).sum()) for k in (1, 2, 3)])
        out["A__%s__metrics" % c] = np.array(errors)
        out["A__%s__ratio" % c] = np.array(ratios, F32)
        out["A__%s__med" % c] = np.array(meds, F32)
        out["A__%s__counts" % c] = np.array(counts, np.int64)
        out["A__%s__summary" % c] = np.array(errors[:CLEAN]).mean(0)
        r = np.array(ratios[:CLEAN], F32)
        med = np.median(r)
        out["A__%s__ratio_stats" % c] = np.array([med, np.std(r / med)], np.float64)
    for ns in (0, 1):
        stub = types.SimpleNamespace(opt=types.SimpleNamespace(no_stereo=bool(ns)),
                                     depth_metric_names=["de/abs_rel", "de/sq_rel", "de/rms", "de/log_rms", "da/a1", "da/a2",
                                                         "da/a3"])
        inputs = {"grid": torch.from_numpy(fx["b_grid"]), ("depth_gt", "l"): torch.from_numpy(fx["b_gt"])}
        losses = ref.trainer.Trainer.compute_depth_losses(stub, inputs, {"depth": torch.from_numpy(fx["b_depth"])})
        out["B__%d__metrics" % ns] = np.array([float(losses[k]) for k in stub.depth_metric_names], np.float64)
        glue = restate_trainer(fx["b_depth"], fx["b_grid"], fx["b_gt"], bool(ns))
        out["B__%d__ratio" % ns] = np.asarray(glue["ratio"], F32)
        out["B__%d__med" % ns] = glue["med"].astype(F32)
        out["B__%d__counts" % ns] = glue["counts"].astype(np.int64)
    return out


def main():
    fx = make_inputs()
    out = reference_outputs(fx)
    n = out["A__pp0_mono_eigen_raw__counts"][:, 0]
    assert (n == 0).any() and (n % 2 == 1).any() and (n[n > 0] % 2 == 0).any(), n   # empty, odd and even sets
    assert np.isnan(out["A__pp0_mono_eigen_raw__ratio"][5]) and np.isfinite(out["A__pp0_mono_eigen_raw__ratio"][:CLEAN]).all()
    data = {k: v for k, v in fx.items() if k != "gts"}
    data.update(out)
    np.savez_compressed(OUT, **data)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
