"""Helpers of tests/test_input_pipeline.py: a plain fp64 restatement of the two input-pipeline operators (the checker, not the
product), torch's own fp32 formulation on the CPU (what the reference computes), and the reader of tests/golden/pipeline_aug.npz.

The restatement follows datasets/pair_transforms.py (RandomResizeCrop :27-56, Resize :66-84, RandomGamma :94-102, RandomBrightness
:112-121, RandomColorBrightness :131-141) and ATen's upsample_bicubic2d (A = -0.75, align_corners=True, taps clamped into the
frame), with the source coordinate (y + h0) (hs - 1) / (full_h - 1) split into floor and fraction by an integer division."""
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

from conftest import GOLDEN

GAMMA, BRIGHTNESS, CHANNEL, FLIP = 1, 2, 4, 8
FIXTURE = os.path.join(GOLDEN, "pipeline_aug.npz")
ULP1 = float(np.finfo(np.float32).eps)   # the spacing of fp32 at 1.0


def cubic_weights(t):
    """[4, n] fp64: ATen's cubic convolution coefficients of the taps i-1 .. i+2 at the fractions t [n]."""
    A = -0.75
    def inner(x):
        return ((A + 2) * x - (A + 3)) * x * x + 1
    def outer(x):
        return ((A * x - 5 * A) * x + 8 * A) * x - 4 * A
    return torch.stack([outer(t + 1), inner(t), inner(1 - t), outer(2 - t)])


def axis_taps(pos, size, full):
    """Tap indices [4, n] (clamped) and weights [4, n] of the output positions ``pos`` (int64 [n]) of an axis resized from ``size``
    to ``full`` with align_corners=True."""
    num, den = pos * (size - 1), max(full - 1, 1)
    i = torch.div(num, den, rounding_mode="floor")
    t = (num - i * den).double() / den
    idx = torch.stack([(i - 1 + k).clamp(0, size - 1) for k in range(4)])
    return idx, cubic_weights(t)


def frame_fp64(frame, hs, ws, flip):
    """[3, hs, ws] fp64 from one frame: uint8 [Hmax, Wmax, 3] (-> v / 255) or float [3, Hmax, Wmax]; padding cut, mirrored under flip."""
    frame = torch.as_tensor(frame)
    img = frame.double().permute(2, 0, 1) / 255 if frame.dtype == torch.uint8 else frame.double()
    img = img[:, :hs, :ws]
    return img.flip(-1) if flip else img


def resize_crop_fp64(frame, hs, ws, crop, flip, H, W):
    """``color`` [3,H,W] in fp64: the bicubic resize of the (hs, ws) frame to crop's full size, clamped, the window cut out."""
    full_w, full_h, w0, h0 = (int(v) for v in crop)
    img = frame_fp64(frame, hs, ws, flip)
    iy, wy = axis_taps(torch.arange(H) + h0, hs, full_h)
    ix, wx = axis_taps(torch.arange(W) + w0, ws, full_w)
    rows = sum(img[:, :, ix[k]] * wx[k] for k in range(4))                   # [3, hs, W]
    out = sum(rows[:, iy[k], :] * wy[k][:, None] for k in range(4))          # [3, H, W]
    return out.clamp(0.0, 1.0)


def augment(color, flags, aug):
    """``color_aug`` from ``color`` [3,H,W] in color's dtype (fp64: the checker; fp32: torch's chain as the reference runs it):
    the stages of pair_transforms.py:94-139 whose bit is set, aug = (gamma, brightness, c0, c1, c2) as Python floats."""
    x = color.clone()
    if flags & GAMMA:
        x = x ** float(aug[0])
    if flags & BRIGHTNESS:
        x = x * float(aug[1])
        x[x > 1] = 1
    if flags & CHANNEL:
        for c in range(3):
            x[c] = x[c] * float(aug[2 + c])
            x[x > 1] = 1
    return x


def nearest_index(n_out_from, n, size, full):
    """ATen's legacy nearest source index of output positions n_out_from .. n_out_from + n - 1, in fp32 as ATen forms it."""
    scale = np.float32(size) / np.float32(full)
    dst = np.arange(n_out_from, n_out_from + n).astype(np.float32)
    return np.minimum(np.floor(dst * scale).astype(np.int64), size - 1)


def resize_crop_nearest(depth, hs, ws, crop, flip, H, W):
    """``depth_gt`` [H,W] from one map [Hd,Wd]: the selection pd_resize_crop_nearest makes, restated with numpy."""
    full_w, full_h, w0, h0 = (int(v) for v in crop)
    d = np.asarray(depth)[:hs, :ws]
    d = d[:, ::-1] if flip else d
    return d[nearest_index(h0, H, hs, full_h)][:, nearest_index(w0, W, ws, full_w)]


def torch_color_fp32(frame, hs, ws, crop, flip, H, W):
    """The reference's own formulation in fp32 on the CPU: ToTensor, F.interpolate bicubic align_corners=True of the whole frame,
    clamp, crop (pair_transforms.py:43-45)."""
    full_w, full_h, w0, h0 = (int(v) for v in crop)
    frame = torch.as_tensor(frame)
    img = frame.float().permute(2, 0, 1).div(255) if frame.dtype == torch.uint8 else frame.float()
    img = img[:, :hs, :ws]
    img = img.flip(-1) if flip else img
    out = F.interpolate(img[None], size=(full_h, full_w), mode="bicubic", align_corners=True)[0].clamp(min=0.0, max=1.0)
    return out[:, h0:h0 + H, w0:w0 + W]


def torch_nearest_fp32(depth, hs, ws, crop, flip, H, W):
    """torch's CPU F.interpolate(mode="nearest") to the full size, then the crop (pair_transforms.py:52-53)."""
    full_w, full_h, w0, h0 = (int(v) for v in crop)
    d = torch.as_tensor(np.ascontiguousarray(depth))[:hs, :ws]
    d = d.flip(-1) if flip else d
    return F.interpolate(d[None, None], size=[full_h, full_w], mode="nearest")[0, 0, h0:h0 + H, w0:w0 + W]


def padded(frames, h_max, w_max, fill):
    """Frames [..., hs, ws, 3] (uint8) or [..., 3, hs, ws] (float) embedded at the origin of h_max x w_max frames full of ``fill``."""
    frames = torch.as_tensor(frames)
    if frames.dtype == torch.uint8:
        out = torch.full(tuple(frames.shape[:-3]) + (h_max, w_max, 3), fill, dtype=torch.uint8)
        out[..., :frames.shape[-3], :frames.shape[-2], :] = frames
    else:
        out = torch.full(tuple(frames.shape[:-2]) + (h_max, w_max), fill, dtype=frames.dtype)
        out[..., :frames.shape[-2], :frames.shape[-1]] = frames
    return out


_fixture = {}


def load_fixture():
    """(meta dict, arrays) of tests/golden/pipeline_aug.npz (made by tests/golden/make_pipeline_golden.py from the reference)."""
    if not _fixture:
        z = np.load(FIXTURE)
        _fixture["meta"] = json.loads(str(z["meta"]))
        _fixture["arrays"] = {k: z[k] for k in z.files if k != "meta"}
    return _fixture["meta"], _fixture["arrays"]


def logged_params(case):
    """(flip, crop (full_w, full_h, w0, h0), flags, aug [V,5] of Python floats) per sample of a fixture case, from the draws the
    generator logged while the REFERENCE ran — decoded by position, as the reference's code consumes them."""
    out = []
    V, H, W = case["V"], case["H"], case["W"]
    hs, ws = case["src_hw"]
    for draws in case["log"]:
        it = iter(draws)
        def take(name):
            n, v = next(it)
            assert n == name, (n, name)
            return v
        flags, aug = 0, [[1.0] * 5 for _ in range(V)]
        crop = (W, H, 0, 0)
        if case["train"]:
            flags |= FLIP if take("random") > 0.5 else 0
            if case["use_crop"]:
                factor = take("np.uniform")
                h0 = take("randint")
                w0 = take("randint")
                crop = (int(ws * factor), int(hs * factor), w0, h0)
            if take("random") < 0.5:
                flags |= GAMMA
                g = take("uniform")
                for v in range(V):
                    aug[v][0] = g
            if take("random") < 0.5:
                flags |= BRIGHTNESS
                g = take("uniform")
                for v in range(V):
                    aug[v][1] = g
            if take("random") < 0.5:
                flags |= CHANNEL
                for c in range(3):
                    for v in range(V):          # the dict's insertion order = the order of the decoded files
                        aug[v][2 + c] = take("uniform")
        assert next(it, None) is None
        out.append((bool(flags & FLIP), crop, flags, aug))
    return out


def keys_of(case, flip):
    """The view names in file order: (left file, right file, novel...) -> the keys they are filed under."""
    return (["r", "l"] if flip else ["l", "r"]) + [str(s) for s in case["novel"]]
