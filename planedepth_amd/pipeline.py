"""The reference's input pipeline on the device: from decoded frames to the ``inputs`` dict of a training step.

``datasets/mono_dataset.py:149-187`` runs ``datasets/pair_transforms.py`` per sample on the host: ToTensor, a bicubic resize of
the whole frame by a random factor, a clamp, a crop, three photometric steps on ``color_aug`` and a nearest resize-crop of
``depth_gt``.  Here the host keeps what only it can do — decoding the files and drawing the random numbers (``draw_params``: the
reference's draws in the reference's order) — and the device does the rest from the uint8 frames in one fused kernel
(``resize_crop_augment``, ``resize_crop_depth``; ``device_batch`` assembles the dict).  No eager / CPU implementation stands
behind the two operators.
"""
from collections import namedtuple

import torch

from . import _capi as C

FLAG_GAMMA, FLAG_BRIGHTNESS, FLAG_CHANNEL, FLAG_FLIP = C.PD_PIPE_GAMMA, C.PD_PIPE_BRIGHTNESS, C.PD_PIPE_CHANNEL, C.PD_PIPE_FLIP

# What the two operators take besides the pixels: src_hw [B,2] int32 (hs, ws), crop [B,4] int32 (full_w, full_h, w0, h0: the layout
# of ops.crop_grid), flags [B] int32 (FLAG_*), aug [B,V,5] float32 (gamma, brightness, c0, c1, c2).
PipelineParams = namedtuple("PipelineParams", "src_hw crop flags aug")


# ---------------------------------------------------------------------------------------------------------------------
# parameter tensors: checked where the host can see them, trusted (and clamped by the kernels) where it cannot
# ---------------------------------------------------------------------------------------------------------------------
def _int_param(name, t, shape):
    if not torch.is_tensor(t):
        raise TypeError("%s must be a tensor" % name)
    if t.dtype != torch.int32:
        raise TypeError("%s must be int32, got %s" % (name, t.dtype))
    if tuple(t.shape) != tuple(shape):
        raise ValueError("%s must have shape %s, got %s" % (name, tuple(shape), tuple(t.shape)))
    return t


def check_params(src_hw, crop, flags, h_max, w_max, height, width, aug=None):
    """Range checks of the CPU-resident parameter tensors (a tensor on the GPU is not read back: the kernels clamp)."""
    if not src_hw.is_cuda:
        for b, (hs, ws) in enumerate(src_hw.tolist()):
            if not (1 <= hs <= h_max and 1 <= ws <= w_max):
                raise ValueError("src_hw[%d] = (%d, %d) is outside the frames' %d x %d" % (b, hs, ws, h_max, w_max))
    if not crop.is_cuda:
        for b, (fw, fh, w0, h0) in enumerate(crop.tolist()):
            if fw < 2 or fh < 2:
                raise ValueError("crop[%d]: the resized frame is %d x %d, need at least 2 x 2" % (b, fh, fw))
            if w0 < 0 or h0 < 0 or w0 + width > fw or h0 + height > fh:
                raise ValueError("crop[%d]: the %d x %d window at (h0 %d, w0 %d) leaves the resized %d x %d frame"
                                 % (b, height, width, h0, w0, fh, fw))
    if not flags.is_cuda:
        for b, f in enumerate(flags.tolist()):
            if not 0 <= f < 16:
                raise ValueError("flags[%d] = %d has bits other than gamma 1, brightness 2, channel 4, flip 8" % (b, f))
    if aug is not None and not aug.is_cuda and not bool((torch.isfinite(aug) & (aug > 0)).all()):
        raise ValueError("aug: every factor must be finite and > 0")


def _on(device, t):
    return t.contiguous() if t.is_cuda else t.to(device, non_blocking=True)


def resize_crop_augment(src, src_hw, crop, flags, aug, height, width):
    """``("color", s)`` and ``("color_aug", s)`` of every view from the decoded frames, one launch (``pd_resize_crop_augment``).

    ``src``: uint8 ``[B,V,Hmax,Wmax,3]`` (HWC, as an image decoder leaves a frame) or float32 ``[B,V,3,Hmax,Wmax]``, on the GPU;
    ``src_hw`` ``[B,2]`` int32: the true size (hs, ws) of sample b's frames, the rest is padding; ``crop`` ``[B,4]`` int32
    (full_w, full_h, w0, h0) as ``ops.crop_grid`` takes it; ``flags`` ``[B]`` int32 (gamma 1, brightness 2, channel 4, flip 8);
    ``aug`` ``[B,V,5]`` float32 (gamma, brightness, c0, c1, c2).  Parameter tensors on the CPU are range-checked (``ValueError``
    before any launch) and uploaded; on the GPU they are trusted.  -> ``(color, color_aug)``, each ``[B,V,3,height,width]``."""
    if not torch.is_tensor(src):
        raise TypeError("src must be a tensor")
    if src.dtype == torch.uint8:
        fmt, ok = C.PD_SRC_U8_HWC, src.dim() == 5 and src.shape[-1] == 3
        B, V, h_max, w_max = (int(s) for s in src.shape[:4]) if ok else (0, 0, 0, 0)
    elif src.dtype == torch.float32:
        fmt, ok = C.PD_SRC_F32_CHW, src.dim() == 5 and src.shape[2] == 3
        B, V, h_max, w_max = (int(src.shape[i]) for i in (0, 1, 3, 4)) if ok else (0, 0, 0, 0)
    else:
        raise TypeError("src must be uint8 [B,V,Hmax,Wmax,3] or float32 [B,V,3,Hmax,Wmax], got %s" % src.dtype)
    if not ok:
        raise ValueError("src must be uint8 [B,V,Hmax,Wmax,3] or float32 [B,V,3,Hmax,Wmax], got %s %s" % (src.dtype, tuple(src.shape)))
    height, width = int(height), int(width)
    _int_param("src_hw", src_hw, (B, 2))
    _int_param("crop", crop, (B, 4))
    _int_param("flags", flags, (B,))
    if not torch.is_tensor(aug) or aug.dtype != torch.float32 or tuple(aug.shape) != (B, V, 5):
        raise TypeError("aug must be a float32 tensor [%d,%d,5] (gamma, brightness, c0, c1, c2)" % (B, V))
    check_params(src_hw, crop, flags, h_max, w_max, height, width, aug)
    C.require_gpu_tensor("src", src, dtype=src.dtype)
    dev = src.device
    with torch.no_grad():
        src = src.contiguous()
        src_hw, crop, flags, aug = _on(dev, src_hw), _on(dev, crop), _on(dev, flags), _on(dev, aug)
        color = torch.empty(B, V, 3, height, width, device=dev, dtype=torch.float32)
        color_aug = torch.empty_like(color)
        C.call("pd_resize_crop_augment", dev, B, V, h_max, w_max, height, width, fmt, src, src_hw, crop, flags, aug, color,
               color_aug)
    return color, color_aug


def resize_crop_depth(depth, src_hw, crop, flags, height, width):
    """The ``depth_gt`` branch of the same transforms (``pd_resize_crop_nearest``): float32 ``[B,1,Hd,Wd]`` with its own ``src_hw``
    -> ``[B,1,height,width]``, torch's legacy ``nearest`` resize to the crop's full size, the same window, the same flip bit.  A
    selection of source elements: bit-exact."""
    if not torch.is_tensor(depth):
        raise TypeError("depth must be a tensor")
    if depth.dim() != 4 or depth.shape[1] != 1:
        raise ValueError("depth must be [B,1,Hd,Wd], got %s" % (tuple(depth.shape),))
    B, _, h_d, w_d = (int(s) for s in depth.shape)
    height, width = int(height), int(width)
    _int_param("src_hw", src_hw, (B, 2))
    _int_param("crop", crop, (B, 4))
    _int_param("flags", flags, (B,))
    check_params(src_hw, crop, flags, h_d, w_d, height, width)
    C.require_gpu_tensor("depth", depth)
    dev = depth.device
    with torch.no_grad():
        depth = depth.contiguous()
        src_hw, crop, flags = _on(dev, src_hw), _on(dev, crop), _on(dev, flags)
        out = torch.empty(B, 1, height, width, device=dev, dtype=torch.float32)
        C.call("pd_resize_crop_nearest", dev, B, h_d, w_d, height, width, depth, src_hw, crop, flags, out)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the host's share: the random numbers
# ---------------------------------------------------------------------------------------------------------------------
def draw_params(py_rng, np_rng, B, views, src_hw, height, width, *, train=True, crop=True, factor=(0.75, 1.5),
                gamma=(0.8, 1.2), brightness=(0.5, 2.0), channel=(0.8, 1.2), log=None):
    """The parameters of ``B`` samples with ``views`` frames each, drawn as ``B`` calls of the reference's ``__getitem__`` draw them.

    ``py_rng`` (a ``random.Random``) and ``np_rng`` (a ``numpy.random.RandomState``) stand for the ``random`` and ``numpy.random``
    modules the reference draws from, so that a reference run seeded alike agrees on every value.  Per sample, in this order:

    1. ``random.random() > 0.5``: the flip (mono_dataset.py:152; ``train`` only);
    2. ``np.random.uniform(min_factor, factor[1])`` with ``min_factor`` of pair_transforms.py:30 (``crop`` only);
    3. ``random.randint`` for h0, then for w0 (:32-33; ``crop`` only);
    4. ``random.random() < 0.5``, then ``random.uniform(*gamma)`` if so (:95-96);
    5. the same for the brightness (:113-114);
    6. ``random.random() < 0.5``, then for c in 0..2, for every view, one ``random.uniform(*channel)`` (:132-136).

    Views are counted in the order the reference inserts its ``("color", s, -1)`` keys (mono_dataset.py:162-171), which is the
    order of the decoded files — left file, right file, novel frames — with or without the flip: under the flip the left file's
    frame is the one the key ``r`` names (``device_batch`` does that renaming).  ``train=False`` is the reference's ``no_data_aug``:
    the plain Resize, nothing drawn.  ``crop=False`` is ``use_crop=False``: Resize, then the photometric draws.

    ``src_hw``: ``[B,2]`` (hs, ws) per sample (tensor or nested list).  ``log``: a list that receives every draw as
    ``(function name, value)`` in order.  -> ``PipelineParams(src_hw, crop, flags, aug)``, CPU tensors."""
    src_hw = torch.as_tensor(src_hw, dtype=torch.int32).reshape(B, 2)
    note = (lambda name, v: log.append((name, v))) if log is not None else (lambda name, v: None)

    def rnd():
        v = py_rng.random()
        note("random", v)
        return v

    def uniform(lo, hi):
        v = py_rng.uniform(lo, hi)
        note("uniform", v)
        return v

    def randint(lo, hi):
        v = py_rng.randint(lo, hi)
        note("randint", v)
        return v

    crops, flags, aug = [], [], torch.ones(B, views, 5, dtype=torch.float64)
    for b, (hs, ws) in enumerate(src_hw.tolist()):
        f = 0
        if train and rnd() > 0.5:
            f |= FLAG_FLIP
        if train and crop:
            min_factor = max(max((height + 1) / hs, (width + 1) / ws), factor[0])
            fac = float(np_rng.uniform(low=min_factor, high=factor[1]))
            note("np.uniform", fac)
            h0 = randint(0, int(hs * fac - height))
            w0 = randint(0, int(ws * fac - width))
            crops.append((int(ws * fac), int(hs * fac), w0, h0))
        else:
            crops.append((width, height, 0, 0))
        if train:
            if rnd() < 0.5:
                f |= FLAG_GAMMA
                aug[b, :, 0] = uniform(*gamma)
            if rnd() < 0.5:
                f |= FLAG_BRIGHTNESS
                aug[b, :, 1] = uniform(*brightness)
            if rnd() < 0.5:
                f |= FLAG_CHANNEL
                for c in range(3):
                    for v in range(views):
                        aug[b, v, 2 + c] = uniform(*channel)
        flags.append(f)
    return PipelineParams(src_hw, torch.tensor(crops, dtype=torch.int32).reshape(B, 4), torch.tensor(flags, dtype=torch.int32),
                          aug.to(torch.float32))


# ---------------------------------------------------------------------------------------------------------------------
# the minibatch
# ---------------------------------------------------------------------------------------------------------------------
def device_batch(frames, depth_gt, params, height, width, novel_frame_ids=()):
    """The ``inputs`` dict of a training step with the reference's keys, from decoded frames on the device.

    ``frames``: uint8 ``[B,V,Hmax,Wmax,3]`` or float32 ``[B,V,3,Hmax,Wmax]``, views in file order: the left file, the right file,
    then one frame per entry of ``novel_frame_ids``.  ``depth_gt``: None, or the pair (left file's, right file's) of float32
    ``[B,1,Hd,Wd]`` maps sized like the frames.  ``params``: ``PipelineParams`` (``draw_params``).  Under a sample's flip bit every
    frame is read mirrored and the left file's window is filed under ``r``, the right file's under ``l`` (mono_dataset.py:162-178).

    -> ``("color", s)`` / ``("color_aug", s)`` for s in l, r, novel ids; ``"grid"`` (``ops.crop_grid``); ``"K"`` / ``"inv_K"``
    (``synthetic.dataset_intrinsics``); ``("Rt","l")`` / ``("Rt","r")``; ``("depth_gt","l")`` / ``("depth_gt","r")`` when given.
    The reference's ``("color", s, -1)`` direct-resize copies are not produced (nothing in its trainer reads them), and ``color`` is
    never augmented (its Resize chain aliases ``color_aug`` to ``color``, so there the in-place channel step also alters ``color``)."""
    from .postprocess import crop_grid
    from .synthetic import dataset_intrinsics
    novel_frame_ids = tuple(novel_frame_ids)
    src_hw, crop, flags, aug = params
    dev = frames.device
    if frames.dim() != 5 or frames.shape[1] != 2 + len(novel_frame_ids):
        raise ValueError("frames must hold %d views (left, right%s), got %s"
                         % (2 + len(novel_frame_ids), ", novel" * bool(novel_frame_ids), tuple(frames.shape)))
    B = frames.shape[0]
    h_max, w_max = (frames.shape[2:4] if frames.dtype == torch.uint8 else frames.shape[3:5])
    check_params(src_hw, crop, flags, int(h_max), int(w_max), int(height), int(width))
    src_hw, crop, flags = _on(dev, src_hw), _on(dev, crop), _on(dev, flags)   # uploaded once, for the four launches below
    color, color_aug = resize_crop_augment(frames, src_hw, crop, flags, aug, height, width)
    sample = torch.arange(B, device=dev)
    flip = (flags.long() >> 3) & 1                     # the view the key "l" names: 0 (left file), 1 under the flip
    inputs = {}
    for name, t in (("color", color), ("color_aug", color_aug)):
        inputs[(name, "l")] = t[sample, flip]
        inputs[(name, "r")] = t[sample, 1 - flip]
        for i, s in enumerate(novel_frame_ids):
            inputs[(name, s)] = t[:, 2 + i].contiguous()
    inputs["grid"] = crop_grid(crop, height, width)
    K, inv_K = dataset_intrinsics(B, int(height), int(width))
    inputs["K"], inputs["inv_K"] = K.to(dev), inv_K.to(dev)
    Tl, Tr = torch.eye(4)[None].repeat(B, 1, 1), torch.eye(4)[None].repeat(B, 1, 1)
    Tl[:, 0, 3], Tr[:, 0, 3] = 0.1, -0.1
    inputs[("Rt", "l")], inputs[("Rt", "r")] = Tl.to(dev), Tr.to(dev)
    if depth_gt is not None:
        d = [resize_crop_depth(g, src_hw, crop, flags, height, width) for g in depth_gt]
        pick = (flip != 0)[:, None, None, None]
        inputs[("depth_gt", "l")] = torch.where(pick, d[1], d[0])
        inputs[("depth_gt", "r")] = torch.where(pick, d[0], d[1])
    return inputs
