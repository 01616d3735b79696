"""Depth evaluation on the device: the Eigen metrics with median scaling of ``evaluate_depth_HR.py`` and the in-training
metrics of ``Trainer.compute_depth_losses``, both over the kernels of ``csrc/pd_depth_eval.hip``.

The contract (every constant fp32 unless marked otherwise):

A. Offline evaluation (``evaluate_depth_HR.py:148-166, 217-279``), per image ``i`` of a ``[M,h,w]`` prediction
   (``[2M,h,w]`` with ``post_process``: image ``i``'s mirrored pass is image ``i+M``) and a ``gt_h x gt_w`` GT:

   1. post-process: ``d = 0.5f * (pred[i] + fliplr(pred[i+M]))`` at the source resolution (``:51-59``: only ``m_disp``
      is live).  Fused into the resize by averaging each pair of taps first: bitwise "average, then resize".
   2. ``cv2.resize(d, (gt_w, gt_h))`` INTER_LINEAR as OpenCV 4's coefficient setup and ``resizeGeneric_`` state it:
      ``inv = (double)gt_w / w``, ``scale = 1.0 / inv`` (fp64), ``fx = (float)((dx + 0.5) * scale - 0.5)``,
      ``sx = floor(fx)``, ``f = fx - sx``.  Columns: ``sx < 0`` -> ``sx = 0, f = 0``; ``sx >= w-1`` -> ``sx = w-1, f = 0``
      (one tap).  Rows: the same formula, both tap rows clamped to ``[0, h-1]`` with the fraction kept (at the edges
      ``r0*(1-f) + r0*f``, which can be 1 ulp away from ``r0``).  Horizontal ``a*(1-f) + b*f`` first, then vertical, fp32,
      no FMA contraction.  This is a restatement of OpenCV's source, not a measurement of cv2: whether a given cv2 build
      matches it to the last bit is not checked (its SIMD vertical pass may use FMA, depending on how it was built).
   3. ``depth = float32(0.1*0.58*width) / disp``, a correctly rounded fp32 division (``width`` = the network's input
      width, ``opt.width``, not the GT's).
   4. Eigen splits (``eigen_raw``, ``eigen_improved``): GT clamped to ``[1e-3, 80]``; valid = ``1e-3 < gt < 80`` inside
      the crop ``[y0,y1) x [x0,x1)`` with ``int32(trunc(c * gt_h))`` etc. and the fp64 constants 0.40810811, 0.99189189,
      0.03594771, 0.96405229.  Other splits: valid = ``gt > 0``, no clamp, no crop.
   5. ``depth *= float32(scale_factor)`` (1 mono, 5.4 ``--eval_stereo``).
   6. Median scaling: ``ratio = med(gt_valid) / med(depth_valid)``, ``depth *= ratio``.  ``med`` is numpy's median: for
      an even count ``(a + b) / 2`` (an fp32 add of the two middle order statistics, then an exact halving); an empty set
      or any NaN gives NaN.
   7. ``depth`` clamped to ``[1e-3, 80]`` by compare-and-replace (NaN stays NaN).
   8. Per image, over the valid set (``compute_errors``, ``:30-49``): ``thresh = max(gt/d, d/gt)``,
      ``a_k = #(thresh < 1.25^k) / n`` (exact counts), ``rmse = sqrt(mean((gt-d)^2))``,
      ``rmse_log = sqrt(mean((log gt - log d)^2))``, ``abs_rel = mean(|gt-d|/gt)``, ``sq_rel = mean((gt-d)^2/gt)``.
      The fp32 terms are summed in fp64 in a fixed order (no float atomics: two runs are bit-identical).
   9. Split summary (:func:`summarize`): the fp64 mean of the per-image rows; with median scaling ``med(ratios)`` and
      ``std(ratios / med)``.

B. Trainer metrics (``trainer.py:775-810``, ``layers.py:356-374``), pooled over the whole batch:

   1. ``d = clamp((depth * 2) / (grid[:,0,:,W-1] - grid[:,0,:,0]), 1e-3, 80)``: one divisor per row (``:784-785``).
   2. valid = ``gt > 0`` inside the crop (``int(c*H)`` with ``H``, ``W`` of ``depth_gt``); ``gt_v = clamp(gt, 1e-3, 80)``.
   3. ``opt.no_stereo``: ``d *= lower_median(gt_v) / lower_median(d_v)``, where the medians are ``torch.median`` over the
      whole batch POOLED, which for an even count returns the LOWER middle value.  Otherwise ``d *= 5.4``.  No clamp after.
   4. The same 7 metrics over the pooled set, as 0-dim device tensors under the reference's names (``trainer.py:171-172``).
   5. ``depth_gt`` must have the prediction's ``H x W`` (the reference indexes the prediction with a GT-sized mask, which
      raises otherwise); resizing to GT resolution is what A is for.

Neither path synchronises with the host: no ``.item()``, no boolean indexing, no ``nonzero``.  The small per-image table
(offsets, sizes, crops) goes to the device with a non-blocking copy from pinned memory.
"""
import collections

import numpy as np
import torch

from . import _capi as C

METRIC_NAMES = ("abs_rel", "sq_rel", "rmse", "rmse_log", "a1", "a2", "a3")
TRAINER_METRIC_NAMES = ("de/abs_rel", "de/sq_rel", "de/rms", "de/log_rms", "da/a1", "da/a2", "da/a3")   # trainer.py:171-172
EIGEN_SPLITS = ("eigen_raw", "eigen_improved")
EIGEN_CROP = (0.40810811, 0.99189189, 0.03594771, 0.96405229)   # evaluate_depth_HR.py:242-243, trainer.py:796
MIN_DEPTH, MAX_DEPTH = 1e-3, 80.0
STEREO_SCALE_FACTOR = 5.4

DepthEval = collections.namedtuple("DepthEval", "metrics ratio medians counts")
DepthEval.__doc__ = ("Per-segment results on the device: metrics [S,7] fp32 (METRIC_NAMES), ratio [S] (the median-scaling "
                     "ratio; 1 without it), medians [S,2] (of gt, of depth; NaN without median scaling), counts [S,4] int32 "
                     "(n, #a1, #a2, #a3)")


class PackedGT:
    """Ragged GT on the device: one fp32 buffer (every image starts on a 16-byte boundary), the per-image table
    ``meta`` int64 [M,8] = (offset, gt_h, gt_w, y0, y1, x0, x1, 0) and the host-side sizes."""

    def __init__(self, data, meta, shapes, offsets):
        self.data, self.meta, self.shapes, self.offsets = data, meta, shapes, offsets
        self.max_hw = max(h * w for h, w in shapes)
        self.max_tiles = -(-self.max_hw // C.PD_EVAL_TILE)

    def __len__(self):
        return len(self.shapes)


def _crop(h, w, eigen):
    if not eigen:
        return (0, h, 0, w)
    c = EIGEN_CROP
    return tuple(int(np.int32(v)) for v in (c[0] * h, c[1] * h, c[2] * w, c[3] * w))   # np.array(...).astype(np.int32)


def _to_device(host, device):
    """Host array -> device tensor without a host sync (pinned staging, non-blocking copy)."""
    t = torch.from_numpy(np.ascontiguousarray(host))
    return t.pin_memory().to(device, non_blocking=True)


def _meta(shapes, offsets, eigen, device):
    m = np.zeros((len(shapes), 8), np.int64)
    for i, ((h, w), o) in enumerate(zip(shapes, offsets)):
        m[i, :7] = (o, h, w) + _crop(h, w, eigen)
    return _to_device(m, device)


def pack_gt(gt_depths, split="eigen_raw", device=None):
    """GT depths -> :class:`PackedGT`.  ``gt_depths``: a list of 2-D numpy arrays or tensors (any sizes), or a dense
    ``[M,H,W]`` array / tensor.  Host arrays are copied to ``device`` (default: the current CUDA device) once."""
    eigen = split in EIGEN_SPLITS
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device())
    if torch.is_tensor(gt_depths) and gt_depths.dim() == 3 and gt_depths.is_cuda:
        M, H, W = gt_depths.shape
        data = C.require_gpu_tensor("gt_depths", gt_depths.contiguous()).reshape(-1)
        offsets = [i * H * W for i in range(M)]
        return PackedGT(data, _meta([(H, W)] * M, offsets, eigen, data.device), [(int(H), int(W))] * M, offsets)
    items = list(gt_depths)
    if not items:
        raise ValueError("gt_depths is empty")
    shapes = []
    for g in items:
        if g.ndim != 2:
            raise ValueError("every GT depth map must be 2-D, got shape %s" % (tuple(g.shape),))
        shapes.append((int(g.shape[0]), int(g.shape[1])))
    offsets, total = [], 0
    for h, w in shapes:
        offsets.append(total)
        total += (h * w + 3) // 4 * 4
    if all(torch.is_tensor(g) and g.is_cuda for g in items):
        device = items[0].device
        data = torch.zeros(total, dtype=torch.float32, device=device)
        for g, o, (h, w) in zip(items, offsets, shapes):
            data[o:o + h * w].copy_(C.require_gpu_tensor("gt_depths[i]", g).reshape(-1))
    else:
        host = torch.zeros(total, dtype=torch.float32).pin_memory()
        view = host.numpy()
        for g, o, (h, w) in zip(items, offsets, shapes):
            g = g.detach().cpu().numpy() if torch.is_tensor(g) else np.asarray(g)
            view[o:o + h * w] = g.astype(np.float32, copy=False).reshape(-1)
        data = host.to(device, non_blocking=True)
    return PackedGT(data, _meta(shapes, offsets, eigen, data.device), shapes, offsets)


def _outputs(S, device):
    return (torch.empty(S, 7, device=device), torch.empty(S, device=device), torch.empty(S, 2, device=device),
            torch.empty(S, 4, dtype=torch.int32, device=device))


def _launch(M, h, w, flags, max_tiles, disp_num, scale_factor, pred, grid, grid_w, gt, meta, S, device):
    lib = C.load()
    ws = torch.empty(lib.pd_depth_eval_workspace_bytes(M, max_tiles, flags), dtype=torch.uint8, device=device)
    metrics, ratio, medians, counts = _outputs(S, device)
    C.call("pd_depth_eval", device, M, h, w, flags, max_tiles, float(np.float32(disp_num)), float(np.float32(scale_factor)),
           pred, grid, grid_w, gt, meta, ws, metrics, ratio, medians, counts)
    return DepthEval(metrics, ratio, medians, counts)


def _pred_maps(pred_disp, n_gt, post_process):
    if not torch.is_tensor(pred_disp):
        raise TypeError("pred_disp must be a tensor")
    if pred_disp.dim() == 4 and pred_disp.shape[1] == 1:
        pred_disp = pred_disp[:, 0]
    if pred_disp.dim() != 3:
        raise ValueError("pred_disp must be [M,h,w] or [M,1,h,w], got %s" % (tuple(pred_disp.shape),))
    want = 2 * n_gt if post_process else n_gt
    if pred_disp.shape[0] != want:
        raise ValueError("pred_disp holds %d maps, %d GT maps need %d%s" % (
            pred_disp.shape[0], n_gt, want, " (post_process: the mirrored passes follow the images)" if post_process else ""))
    return C.require_gpu_tensor("pred_disp", pred_disp).contiguous()


def eval_depth_errors(pred_disp, gt_depths, *, width, split="eigen_raw", post_process=False, median_scaling=True,
                      scale_factor=1.0):
    """Per-image Eigen metrics of ``evaluate_depth_HR.py`` (contract A above) on the device.

    ``pred_disp``: [M,h,w] (or [M,1,h,w]) fp32 disparities on the GPU, [2M,...] with ``post_process``; ``gt_depths``: a
    list of 2-D arrays / tensors, a dense [M,H,W] tensor, or a :class:`PackedGT` (from :func:`pack_gt` with the same
    ``split``).  ``width``: the network's input width.  Returns a :class:`DepthEval` of device tensors, one row per image;
    :func:`summarize` gives the reference's split line."""
    packed = gt_depths if isinstance(gt_depths, PackedGT) else pack_gt(
        gt_depths, split, pred_disp.device if torch.is_tensor(pred_disp) and pred_disp.is_cuda else None)
    M = len(packed)
    pred = _pred_maps(pred_disp, M, post_process)
    if pred.device != packed.data.device:
        raise ValueError("pred_disp is on %s, the GT on %s" % (pred.device, packed.data.device))
    flags = ((C.PD_EVAL_POST_PROCESS if post_process else 0) | (C.PD_EVAL_EIGEN if split in EIGEN_SPLITS else 0) |
             (C.PD_EVAL_MEDIAN if median_scaling else 0))
    _, h, w = pred.shape
    return _launch(M, h, w, flags, packed.max_tiles, 0.1 * 0.58 * width, scale_factor, pred, None, 0, packed.data,
                   packed.meta, M, pred.device)


def resize_disp(pred_disp, gt_depths, *, post_process=False):
    """Step A2 alone (and A1 with ``post_process``): the disparity resized to every GT's size, as a list of device maps."""
    packed = gt_depths if isinstance(gt_depths, PackedGT) else pack_gt(
        gt_depths, "eigen_raw", pred_disp.device if torch.is_tensor(pred_disp) and pred_disp.is_cuda else None)
    pred = _pred_maps(pred_disp, len(packed), post_process)
    _, h, w = pred.shape
    out = torch.empty_like(packed.data)
    C.call("pd_depth_eval_resize", pred.device, len(packed), h, w, C.PD_EVAL_POST_PROCESS if post_process else 0, packed.max_hw,
           pred, packed.meta, out)
    return [out[o:o + hh * ww].view(hh, ww) for o, (hh, ww) in zip(packed.offsets, packed.shapes)]


_TRAINER_META = {}


def trainer_depth_metrics(depth, grid, depth_gt, *, no_stereo, scale_factor=STEREO_SCALE_FACTOR):
    """Contract B: the pooled metrics of ``Trainer.compute_depth_losses`` -> :class:`DepthEval` with one segment."""
    depth = C.require_gpu_tensor("depth", depth.detach())
    depth_gt = C.require_gpu_tensor("depth_gt", depth_gt.detach())
    grid = C.require_gpu_tensor("grid", grid.detach())
    if depth_gt.dim() != 4 or depth_gt.shape[1] != 1:
        raise ValueError("depth_gt must be [B,1,H,W], got %s" % (tuple(depth_gt.shape),))
    B, _, H, W = depth_gt.shape
    if tuple(depth.shape) != (B, 1, H, W):
        raise ValueError("depth %s and depth_gt %s differ in shape: the reference indexes the prediction with the GT's mask "
                         "(trainer.py:798-800); resize to GT resolution with eval_depth_errors instead"
                         % (tuple(depth.shape), tuple(depth_gt.shape)))
    if grid.dim() != 4 or grid.shape[0] != B or grid.shape[1] < 1 or grid.shape[2] != H:
        raise ValueError("grid must be [B,2,H,Wg] with the depth's B and H, got %s" % (tuple(grid.shape),))
    if H * W >= 1 << 31:
        raise ValueError("depth maps of 2^31 pixels or more are not supported")
    key = (depth.device, B, H, W)
    meta = _TRAINER_META.get(key)
    if meta is None:
        meta = _TRAINER_META[key] = _meta([(H, W)] * B, [i * H * W for i in range(B)], True, depth.device)
    g0 = grid[:, 0].contiguous()
    flags = C.PD_EVAL_TRAINER | (C.PD_EVAL_MEDIAN if no_stereo else 0)
    max_tiles = -(-H * W // C.PD_EVAL_TILE)
    return _launch(B, H, W, flags, max_tiles, 0.0, scale_factor, depth.contiguous(), g0, g0.shape[-1],
                   depth_gt.contiguous(), meta, 1, depth.device)


def summarize(result, median_scaling=True):
    """Step A9 on the host (this one synchronises): ``mean_errors`` (the fp64 mean of the per-image rows, a_k from the
    exact counts) and, with median scaling, ``ratio_med`` / ``ratio_std`` as the reference prints them (:270-273)."""
    metrics = result.metrics.detach().cpu().numpy().astype(np.float64)
    counts = result.counts.detach().cpu().numpy().astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        metrics[:, 4:] = counts[:, 1:] / counts[:, :1]
    out = {"mean_errors": metrics.mean(0), "names": METRIC_NAMES}
    if median_scaling:
        ratios = result.ratio.detach().cpu().numpy().astype(np.float32)
        med = np.median(ratios)
        out["ratio_med"], out["ratio_std"] = med, np.std(ratios / med)
    return out


def format_summary(summary):
    """The reference's table lines (:270-273, :277-278)."""
    lines = []
    if "ratio_med" in summary:
        lines.append(" Scaling ratios | med: {:0.3f} | std: {:0.3f}".format(summary["ratio_med"], summary["ratio_std"]))
    lines.append("\n  " + ("{:>8} | " * 7).format(*METRIC_NAMES))
    lines.append(("&{: 8.5f}  " * 7).format(*summary["mean_errors"].tolist()) + "\\\\")
    return "\n".join(lines)
