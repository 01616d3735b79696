"""The device input pipeline (planedepth_amd/pipeline.py, pd_input_pipeline.hip): fused bicubic resize-crop and augmentation of
decoded frames, the nearest resize-crop of depth_gt, the host-side sampler and the assembled minibatch.

CPU: ``draw_params`` against the draws logged while the reference ran (tests/golden/pipeline_aug.npz, made by
tests/golden/make_pipeline_golden.py), the fp64 restatement of tests/pipeline_cases.py against the reference's tensors, the range
checks, and header <-> ctypes table.  GPU (``-m gpu``): the kernels per element against that fp64 restatement, the exact cases,
torch's own fp32 chain as the yardstick at KITTI size, the reference fixture through ``device_batch``, padding independence, write
extents and the stream."""
import ctypes
import os
import random
import sys

import numpy as np
import pytest
import torch

import capi_header
from conftest import GOLDEN
from pipeline_cases import (BRIGHTNESS, CHANNEL, FLIP, GAMMA, ULP1, augment, keys_of, load_fixture, logged_params, padded,
                            resize_crop_fp64, resize_crop_nearest, torch_color_fp32, torch_nearest_fp32)
from planedepth_amd import _capi as C
from planedepth_amd import ops, pipeline

H, W = 8, 16
SOURCES = ((11, 19), (20, 37), (23, 41))
TAGS = ("all_on", "all_off", "flip_v4", "resize", "depth_flip", "depth_v4", "eval")


# ---------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------
def test_fixture_covers_the_contract_cases():
    meta, arrays = load_fixture()
    cases = meta["cases"]
    assert set(cases) == set(TAGS) and len(cases) >= 6
    first = {tag: logged_params(c)[0] for tag, c in cases.items()}
    assert first["all_on"][2] & 7 == 7 and first["all_off"][2] & 7 == 0                  # every stage on / off
    assert first["flip_v4"][0] and first["flip_v4"][2] & CHANNEL and cases["flip_v4"]["V"] == 4
    assert {c["V"] for c in cases.values()} == {2, 4}
    assert cases["resize"]["train"] and not cases["resize"]["use_crop"]                   # the Resize chain, augmented
    assert not cases["eval"]["train"] and cases["eval"]["log"] == [[], []]                # no_data_aug draws nothing
    assert any(c["depth"] and any(c["flips"]) for c in cases.values())                    # depth_gt under the flip
    assert os.path.getsize(os.path.join(GOLDEN, "pipeline_aug.npz")) < 200 * 1024
    for tag, c in cases.items():
        assert arrays[tag + "/frames"].dtype == np.uint8
        assert [flip for flip, _, _, _ in logged_params(c)] == c["flips"]


@pytest.mark.parametrize("tag", TAGS)
def test_draw_params_reproduces_every_logged_draw(tag):
    """Seeded like the reference run, the sampler consumes the same draws in the same order: every value bit for bit."""
    case = load_fixture()[0]["cases"][tag]
    log = []
    p = pipeline.draw_params(random.Random(case["seed"]), np.random.RandomState(case["seed"]), case["B"], case["V"],
                             [case["src_hw"]] * case["B"], case["H"], case["W"], train=case["train"], crop=case["use_crop"], log=log)
    want = [(n, v) for sample in case["log"] for n, v in sample]
    assert log == want                                             # names, order and values (floats compare by value: every bit)
    assert all(type(a[1]) is type(b[1]) for a, b in zip(log, want))
    for b, (flip, crop, flags, aug) in enumerate(logged_params(case)):
        assert tuple(p.crop[b].tolist()) == crop and int(p.flags[b]) == flags and bool(int(p.flags[b]) & FLIP) == flip
        assert torch.equal(p.aug[b], torch.tensor(aug, dtype=torch.float64).float())      # per view, channel order included
        assert p.src_hw[b].tolist() == case["src_hw"]
    assert p.crop.dtype == p.flags.dtype == p.src_hw.dtype == torch.int32 and p.aug.dtype == torch.float32
    assert not any(t.is_cuda for t in p)


@pytest.mark.parametrize("tag", TAGS)
def test_fp64_restatement_meets_the_reference_fixture(tag):
    meta, arrays = load_fixture()
    case = meta["cases"][tag]
    hs, ws = case["src_hw"]
    for b, (flip, crop, flags, aug) in enumerate(logged_params(case)):
        for v, key in enumerate(keys_of(case, flip)):
            color = resize_crop_fp64(arrays[tag + "/frames"][b, v], hs, ws, crop, flip, case["H"], case["W"])
            got_aug = augment(color, flags, aug[v])
            assert float((color - torch.from_numpy(arrays["%s/color_%s" % (tag, key)][b]).double()).abs().max()) < 1e-4, (b, key)
            assert float((got_aug - torch.from_numpy(arrays["%s/color_aug_%s" % (tag, key)][b]).double()).abs().max()) < 1e-4, (b, key)
            if case["depth"] and v < 2:
                d = resize_crop_nearest(arrays[tag + "/depth"][b, v], hs, ws, crop, flip, case["H"], case["W"])
                assert np.array_equal(d, arrays["%s/depth_gt_%s" % (tag, key)][b, 0]), (b, key)


def test_fixture_matches_the_live_reference():
    sys.path.insert(0, GOLDEN)
    from ref_import import reference_available
    if not reference_available():
        pytest.skip("reference tree not present")
    from make_pipeline_golden import reference_outputs
    meta, arrays = load_fixture()
    for tag, case in meta["cases"].items():
        live_meta, live = reference_outputs(tag, case["seed"])
        assert live_meta == case, tag
        for k, v in live.items():
            have = arrays["%s/%s" % (tag, k)]
            if v.dtype == np.uint8 or "depth" in k:
                assert np.array_equal(have, v), (tag, k)
            else:
                assert float(np.abs(have.astype(np.float64) - v).max()) <= 1e-6, (tag, k)


def good_params(B=1, V=1):
    return dict(src_hw=torch.tensor([[11, 19]] * B, dtype=torch.int32), crop=torch.tensor([[19, 11, 1, 2]] * B, dtype=torch.int32),
                flags=torch.zeros(B, dtype=torch.int32), aug=torch.ones(B, V, 5))


VIOLATIONS = (
    ("crop", (1, 11, 0, 0)), ("crop", (19, 1, 0, 0)),                       # 2 <= full
    ("crop", (19, 11, -1, 0)), ("crop", (19, 11, 0, -1)),                   # 0 <= w0, h0
    ("crop", (19, 11, 4, 0)), ("crop", (19, 11, 0, 4)),                     # w0 + W <= full_w, h0 + H <= full_h
    ("crop", (15, 11, 0, 0)), ("crop", (19, 7, 0, 0)),                      # the window itself does not fit
    ("src_hw", (0, 19)), ("src_hw", (11, 0)), ("src_hw", (13, 19)), ("src_hw", (11, 22)),   # 1 <= hs <= Hmax, 1 <= ws <= Wmax
    ("flags", 16), ("flags", -1),
    ("aug", (0.0, 1, 1, 1, 1)), ("aug", (1, -0.5, 1, 1, 1)), ("aug", (1, 1, float("nan"), 1, 1)), ("aug", (1, 1, 1, float("inf"), 1)),
)


@pytest.mark.parametrize("name,value", VIOLATIONS)
def test_range_violations_raise_before_any_launch(name, value):
    """CPU-resident parameters are checked first: a ValueError, although the frames are CPU tensors no kernel could take."""
    src = torch.zeros(2, 1, 12, 21, 3, dtype=torch.uint8)
    p = good_params(B=2)
    p[name][1] = torch.tensor(value, dtype=p[name].dtype)                   # the second sample: every row is looked at
    with pytest.raises(ValueError):
        ops.resize_crop_augment(src, p["src_hw"], p["crop"], p["flags"], p["aug"], H, W)
    if name != "aug":
        with pytest.raises(ValueError):
            ops.resize_crop_depth(torch.zeros(2, 1, 12, 21), p["src_hw"], p["crop"], p["flags"], H, W)


def test_operators_check_types_and_refuse_cpu_frames():
    p = good_params()
    src = torch.zeros(1, 1, 12, 21, 3, dtype=torch.uint8)
    with pytest.raises(C.PlaneDepthHipError):                               # valid parameters: only the device is wrong
        ops.resize_crop_augment(src, p["src_hw"], p["crop"], p["flags"], p["aug"], H, W)
    with pytest.raises(C.PlaneDepthHipError):
        ops.resize_crop_depth(torch.zeros(1, 1, 12, 21), p["src_hw"], p["crop"], p["flags"], H, W)
    with pytest.raises(TypeError):
        ops.resize_crop_augment(src.to(torch.int16), p["src_hw"], p["crop"], p["flags"], p["aug"], H, W)
    with pytest.raises(ValueError):
        ops.resize_crop_augment(src[..., :2], p["src_hw"], p["crop"], p["flags"], p["aug"], H, W)
    with pytest.raises(TypeError):
        ops.resize_crop_augment(src, p["src_hw"].long(), p["crop"], p["flags"], p["aug"], H, W)
    with pytest.raises(ValueError):
        ops.resize_crop_augment(src, p["src_hw"], p["crop"][:, :3], p["flags"], p["aug"], H, W)
    with pytest.raises(TypeError):
        ops.resize_crop_augment(src, p["src_hw"], p["crop"], p["flags"], p["aug"].double(), H, W)
    assert ops.resize_crop_augment is pipeline.resize_crop_augment and ops.resize_crop_depth is pipeline.resize_crop_depth
    import planedepth_amd
    assert planedepth_amd.draw_params is pipeline.draw_params and planedepth_amd.device_batch is pipeline.device_batch


def test_header_capi_and_library_agree():
    for name, value in (("PD_SRC_U8_HWC", 0), ("PD_SRC_F32_CHW", 1), ("PD_PIPE_GAMMA", 1), ("PD_PIPE_BRIGHTNESS", 2),
                        ("PD_PIPE_CHANNEL", 4), ("PD_PIPE_FLIP", 8)):
        assert capi_header.constant(name) == getattr(C, name) == value, name
    assert (GAMMA, BRIGHTNESS, CHANNEL, FLIP) == (C.PD_PIPE_GAMMA, C.PD_PIPE_BRIGHTNESS, C.PD_PIPE_CHANNEL, C.PD_PIPE_FLIP)
    lib = C.load()
    for name, kinds in (("pd_resize_crop_augment", "IIIIIIIPPPPPPPP"), ("pd_resize_crop_nearest", "IIIIIPPPPPP")):
        res, args = C.SIGNATURES[name]
        assert res is ctypes.c_int
        assert capi_header.kinds(name) == capi_header.ctypes_kinds(args) == list(kinds), name
        assert hasattr(lib, name)


def test_entry_points_validate_without_gpu():
    lib = C.load()
    P = ctypes.c_void_p(16)   # never dereferenced: every call below is refused in validation
    aug = lambda B=1, V=1, Hm=12, Wm=21, h=H, w=W, dt=0, ptrs=None: lib.pd_resize_crop_augment(   # noqa: E731
        B, V, Hm, Wm, h, w, dt, *(ptrs or [None] * 8))
    assert aug() == 1 and b"NULL" in lib.pd_last_error()
    assert aug(B=0) == 1 and b"shape" in lib.pd_last_error()
    assert aug(B=256, V=256) == 1 and b"shape" in lib.pd_last_error()
    assert aug(h=0) == 1 and b"shape" in lib.pd_last_error()
    assert aug(Hm=40000) == 1 and b"shape" in lib.pd_last_error()
    assert aug(Hm=32768, Wm=32768) == 1 and b"shape" in lib.pd_last_error()
    assert aug(dt=2) == 1 and b"src_dtype" in lib.pd_last_error()
    assert aug(ptrs=[P] * 5 + [P, P, None]) == 1 and b"alias" in lib.pd_last_error()
    near = lambda B=1, Hd=12, Wd=21, h=H, w=W: lib.pd_resize_crop_nearest(B, Hd, Wd, h, w, *([None] * 6))   # noqa: E731
    assert near() == 1 and b"NULL" in lib.pd_last_error()
    assert near(B=0) == 1 and b"shape" in lib.pd_last_error()
    assert near(Wd=0) == 1 and b"shape" in lib.pd_last_error()


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
gpu = pytest.mark.gpu
DEV = "cuda:0"


def noise_frames(seed, B, V, hs, ws, dtype):
    """White noise, the hardest input of an interpolation: uint8 HWC frames, or the same values as fp32 CHW in [0, 1]."""
    g = torch.Generator().manual_seed(seed)
    u8 = torch.randint(0, 256, (B, V, hs, ws, 3), generator=g, dtype=torch.uint8)
    if dtype == "u8":
        return u8
    return (u8.float() + torch.rand(B, V, hs, ws, 3, generator=g)).div(256).permute(0, 1, 4, 2, 3).contiguous()


def windows(hs, ws, extra=()):
    """(crop, flip) per sample: factors 0.75 / 1.0 / 1.5 where the window fits, full = target + 1, whatever ``extra`` adds; each
    with the window at the near and at the far corner (taps clamp on all four borders), each plain and mirrored."""
    fulls = [(int(ws * f), int(hs * f)) for f in (0.75, 1.0, 1.5)] + [(W + 1, H + 1)] + list(extra)
    out = []
    for fw, fh in fulls:
        if fw < W or fh < H:
            continue
        for w0, h0 in ((0, 0), (fw - W, fh - H)):
            for flip in (False, True):
                out.append(((fw, fh, w0, h0), flip))
    return out


def tensors(hw, wins, flags=None, aug=None, V=1):
    B = len(wins)
    flags = [0] * B if flags is None else flags
    return pipeline.PipelineParams(
        torch.tensor([list(hw)] * B if isinstance(hw[0], int) else [list(x) for x in hw], dtype=torch.int32),
        torch.tensor([list(c) for c, _ in wins], dtype=torch.int32),
        torch.tensor([f | (FLIP if flip else 0) for f, (_, flip) in zip(flags, wins)], dtype=torch.int32),
        torch.ones(B, V, 5) if aug is None else aug)


def pad_poison(frames, pad, dtype):
    if not pad:
        return frames
    hs, ws = (frames.shape[2:4] if dtype == "u8" else frames.shape[3:5])
    return padded(frames, hs + 3, ws + 5, 255 if dtype == "u8" else float("nan"))


def fp64_colors(frames, p):
    """[B,V,3,H,W] fp64 from the UNPADDED frames of every sample."""
    B, V = frames.shape[:2]
    return torch.stack([torch.stack([resize_crop_fp64(frames[b, v], int(p.src_hw[b, 0]), int(p.src_hw[b, 1]), p.crop[b].tolist(),
                                                      bool(int(p.flags[b]) & FLIP), H, W) for v in range(V)]) for b in range(B)])


@gpu
@pytest.mark.parametrize("dtype", ("u8", "f32"))
@pytest.mark.parametrize("hw,V,pad", (((11, 19), 1, False), ((11, 19), 4, True), ((20, 37), 2, True), ((20, 37), 3, False),
                                      ((23, 41), 2, False), ((23, 41), 4, True)))
def test_color_matches_fp64_per_element(hw, V, pad, dtype):
    """Cap 1e-5 absolute against the fp64 restatement (torch's own fp32 chain on the CPU is 2.5e-6 to 3.1e-6 away at these shapes; the
    cap leaves a factor of 3 to 4 for a different summation order).  Measured: profiles/operator_parity.md."""
    wins = windows(*hw)
    frames = noise_frames(11 * hw[0] + V, len(wins), V, hw[0], hw[1], dtype)
    p = tensors(hw, wins, V=V)
    color, color_aug = ops.resize_crop_augment(pad_poison(frames, pad, dtype).to(DEV), *p, H, W)
    want = fp64_colors(frames, p)
    err = float((color.cpu().double() - want).abs().max())
    print("color vs fp64 %s V=%d pad=%d %s: %.3e over %d windows" % (hw, V, pad, dtype, err, len(wins)))
    assert tuple(color.shape) == (len(wins), V, 3, H, W) and color.dtype == torch.float32
    assert err <= 1e-5
    assert torch.equal(color_aug, color)                       # flags without stage bits: the clone


@gpu
@pytest.mark.parametrize("dtype", ("u8", "f32"))
def test_color_batch_of_three_frame_sizes(dtype):
    """B = 3 with three different src_hw inside one padded tensor, parameters resident on the GPU (trusted, not read back)."""
    g = torch.Generator().manual_seed(5)
    wins = [((int(ws * 1.5), int(hs * 1.5), 3, 2), b == 1) for b, (hs, ws) in enumerate(SOURCES)]
    singles = [noise_frames(40 + b, 1, 2, hs, ws, dtype) for b, (hs, ws) in enumerate(SOURCES)]
    fill = 255 if dtype == "u8" else float("nan")
    frames = torch.cat([padded(f, 25, 44, fill) for f in singles])
    aug = 0.8 + 0.4 * torch.rand(3, 2, 5, generator=g)
    p = tensors(SOURCES, wins, flags=[7, 5, 2], aug=aug, V=2)
    color, color_aug = ops.resize_crop_augment(frames.to(DEV), *(t.to(DEV) for t in p), H, W)
    host = ops.resize_crop_augment(frames.to(DEV), *p, H, W)
    assert torch.equal(color, host[0]) and torch.equal(color_aug, host[1])
    for b, (hs, ws) in enumerate(SOURCES):
        q = tensors((hs, ws), wins[b:b + 1], V=2)
        err = float((color[b].cpu().double() - fp64_colors(singles[b], q)[0]).abs().max())
        assert err <= 1e-5, (b, err)
        for v in range(2):
            want = augment(color[b, v].cpu().double(), int(p.flags[b]), aug[b, v].double().tolist())
            assert float((color_aug[b, v].cpu().double() - want).abs().max()) <= 1e-6, (b, v)


@gpu
@pytest.mark.parametrize("dtype", ("u8", "f32"))
def test_identity_resize_copies_the_source_bit_for_bit(dtype):
    """full == source: every coordinate is a whole number, the weights are (0, 1, 0, 0) exactly and ``color`` is uint8 / 255 (the
    fp32 source itself) cropped, mirrored under the flip; without stage bits ``color_aug`` has color's bits."""
    for hs, ws in SOURCES:
        wins = [((ws, hs, w0, h0), flip) for w0, h0 in ((0, 0), (ws - W, hs - H), (1, 2)) for flip in (False, True)]
        frames = noise_frames(7 + hs, len(wins), 2, hs, ws, dtype)
        p = tensors((hs, ws), wins, V=2)
        color, color_aug = ops.resize_crop_augment(pad_poison(frames, True, dtype).to(DEV), *p, H, W)
        chw = frames.permute(0, 1, 4, 2, 3).float().div(255) if dtype == "u8" else frames
        for b, ((_, _, w0, h0), flip) in enumerate(wins):
            src = chw[b].flip(-1) if flip else chw[b]
            assert torch.equal(color[b].cpu(), src[:, :, h0:h0 + H, w0:w0 + W]), (hs, ws, b)
        assert torch.equal(color_aug, color)


@gpu
def test_kitti_sized_frame_is_closer_to_fp64_than_torch():
    """One 375 x 1242 uint8 frame resized by 0.9, 8 x 16 windows at the near and the far corner.  torch forms scale * index in fp32
    and is 8e-5 from fp64 at the far corner; the kernel's integer coordinate holds the 1e-5 of the small shapes everywhere."""
    hs, ws = 375, 1242
    frames = noise_frames(3, 1, 1, hs, ws, "u8").expand(2, 1, hs, ws, 3).contiguous()
    fw, fh = int(ws * 0.9), int(hs * 0.9)
    wins = [((fw, fh, 0, 0), False), ((fw, fh, fw - W, fh - H), False)]
    p = tensors((hs, ws), wins)
    color, _ = ops.resize_crop_augment(frames.to(DEV), *p, H, W)
    want = fp64_colors(frames, p)
    for b, (crop, flip) in enumerate(wins):
        err = float((color[b, 0].cpu().double() - want[b, 0]).abs().max())
        err_torch = float((torch_color_fp32(frames[b, 0], hs, ws, crop, flip, H, W).double() - want[b, 0]).abs().max())
        print("375x1242 window %d: kernel %.3e, torch fp32 %.3e from fp64" % (b, err, err_torch))
        assert err <= 1e-5
        assert err <= err_torch
    assert err_torch > 1e-5                                    # the far corner: what the integer coordinate is for


LO, HI = (0.8, 0.5, 0.8, 1.2, 0.8), (1.2, 2.0, 1.2, 0.8, 1.2)   # gamma, brightness (2.0 saturates), channel factors


@gpu
def test_augmentation_stage_against_fp64_on_the_kernels_own_color():
    """color_aug against the fp64 chain applied to the kernel's OWN color (so that x^0.8 near zero does not blame the resize), for
    every subset of the three stages at both ends of the factor ranges.  Bound per sample: twice the distance of torch's fp32 chain
    on the CPU from the same fp64 chain on the same input, plus 4 ulp of 1.0."""
    subsets = list(range(8))
    wins = [((37, 20, 5, 3), False)] * 16
    flags = subsets + subsets
    aug = torch.tensor([LO] * 8 + [HI] * 8)[:, None, :].repeat(1, 2, 1)
    aug[:, 1, 2:] = aug[:, 1, 2:].flip(-1) * 1.01                   # the second view has channel factors of its own
    frames = noise_frames(21, 16, 2, 20, 37, "u8")
    p = tensors((20, 37), wins, flags=flags, aug=aug, V=2)
    color, color_aug = ops.resize_crop_augment(frames.to(DEV), *p, H, W)
    color, color_aug = color.cpu(), color_aug.cpu()
    worst = worst_torch = 0.0
    for b in range(16):
        for v in range(2):
            a = aug[b, v].double().tolist()
            want = augment(color[b, v].double(), flags[b], a)
            err = float((color_aug[b, v].double() - want).abs().max())
            err_torch = float((augment(color[b, v], flags[b], a).double() - want).abs().max())
            worst, worst_torch = max(worst, err), max(worst_torch, err_torch)
            assert err <= 2 * err_torch + 4 * ULP1, (b, v, err, err_torch)
            if flags[b] == 0:
                assert torch.equal(color_aug[b, v], color[b, v])
    assert bool((color_aug[8:] == 1).any())                        # brightness 2.0 saturated somewhere
    print("color_aug vs fp64 chain: kernel %.3e, torch fp32 %.3e" % (worst, worst_torch))


@gpu
@pytest.mark.parametrize("tag", TAGS)
def test_reference_fixture_through_device_batch(tag):
    """Every case of pipeline_aug.npz with the parameters the reference drew: color, color_aug and grid at the plain 1e-4, depth_gt
    bit for bit, the reference's keys — the left file's window under ``r`` where the sample was flipped."""
    meta, arrays = load_fixture()
    case = meta["cases"][tag]
    logged = logged_params(case)
    B, V = case["B"], case["V"]
    p = pipeline.PipelineParams(torch.tensor([case["src_hw"]] * B, dtype=torch.int32),
                                torch.tensor([list(crop) for _, crop, _, _ in logged], dtype=torch.int32),
                                torch.tensor([flags for _, _, flags, _ in logged], dtype=torch.int32),
                                torch.tensor([aug for _, _, _, aug in logged], dtype=torch.float64).float())
    frames = torch.from_numpy(arrays[tag + "/frames"]).to(DEV)
    depth = None
    if case["depth"]:
        depth = [torch.from_numpy(arrays[tag + "/depth"][:, v:v + 1].copy()).to(DEV) for v in range(2)]
    inputs = pipeline.device_batch(frames, depth, p, case["H"], case["W"], novel_frame_ids=case["novel"])
    sides = ["l", "r"] + case["novel"]
    keys = {(n, s) for n in ("color", "color_aug") for s in sides} | {"grid", "K", "inv_K", ("Rt", "l"), ("Rt", "r")}
    keys |= {("depth_gt", "l"), ("depth_gt", "r")} if case["depth"] else set()
    assert set(inputs) == keys
    for s in sides:
        for n in ("color", "color_aug"):
            got = inputs[(n, s)]
            assert got.is_contiguous() and tuple(got.shape) == (B, 3, case["H"], case["W"])
            err = float((got.cpu() - torch.from_numpy(arrays["%s/%s_%s" % (tag, n, s)])).abs().max())
            assert err < 1e-4, (n, s, err)
    assert float((inputs["grid"].cpu() - torch.from_numpy(arrays[tag + "/grid"])).abs().max()) < 1e-4
    if case["depth"]:
        for s in ("l", "r"):
            assert torch.equal(inputs[("depth_gt", s)].cpu(), torch.from_numpy(arrays["%s/depth_gt_%s" % (tag, s)])), s
    assert tuple(inputs["K"].shape) == tuple(inputs["inv_K"].shape) == (B, 4, 4)
    assert float(inputs[("Rt", "l")][0, 0, 3]) == pytest.approx(0.1) and float(inputs[("Rt", "r")][0, 0, 3]) == pytest.approx(-0.1)


@gpu
def test_depth_is_torchs_nearest_selection_bit_for_bit():
    """resize_crop_depth against torch's CPU F.interpolate(mode="nearest") + crop: factors 0.75 / 1 / 1.5 / 2, full = target + 1,
    both corners, plain and mirrored, three frame sizes inside poisoned padding, and the 375 x 1242 map."""
    g = torch.Generator().manual_seed(2)
    for hs, ws in SOURCES + ((375, 1242),):
        big = hs > 100
        wins = windows(hs, ws, extra=[(int(ws * 0.9), int(hs * 0.9))] if big else [(2 * ws, 2 * hs)])
        depth = torch.rand(len(wins), 1, hs, ws, generator=g) * 80
        p = tensors((hs, ws), wins)
        src = depth if big else padded(depth, hs + 2, ws + 3, float("nan"))
        out = ops.resize_crop_depth(src.to(DEV), p.src_hw, p.crop, p.flags, H, W).cpu()
        assert tuple(out.shape) == (len(wins), 1, H, W)
        for b, (crop, flip) in enumerate(wins):
            assert torch.equal(out[b, 0], torch_nearest_fp32(depth[b, 0].numpy(), hs, ws, crop, flip, H, W)), (hs, ws, crop, flip)


@gpu
@pytest.mark.parametrize("dtype", ("u8", "f32"))
def test_padding_never_influences_a_result(dtype):
    """The same windows with the frames' padding rows / columns full of 0, 255 and (fp32) NaN: bit-identical outputs."""
    hs, ws = 20, 37
    wins = windows(hs, ws)
    g = torch.Generator().manual_seed(8)
    aug = 0.8 + 0.4 * torch.rand(len(wins), 2, 5, generator=g)
    frames = noise_frames(31, len(wins), 2, hs, ws, dtype)
    p = tensors((hs, ws), wins, flags=[7] * len(wins), aug=aug, V=2)
    fills = (0, 255) if dtype == "u8" else (0.0, 255.0, float("nan"))
    outs = [ops.resize_crop_augment(padded(frames, hs + 3, ws + 5, fill).to(DEV), *p, H, W) for fill in fills]
    outs.append(ops.resize_crop_augment(frames.to(DEV), *p, H, W))           # and with no padding at all
    for color, color_aug in outs[1:]:
        assert torch.equal(color, outs[0][0]) and torch.equal(color_aug, outs[0][1])
    assert bool(torch.isfinite(outs[0][1]).all())


@gpu
def test_writes_cover_exactly_the_two_outputs():
    """Both outputs inside one larger pre-filled buffer: every element around them keeps its fill."""
    lib = C.load()
    hs, ws, V = 23, 41, 3
    wins = windows(hs, ws)
    B = len(wins)
    p = tensors((hs, ws), wins, flags=[7] * B, V=V)
    frames = noise_frames(17, B, V, hs, ws, "u8").to(DEV)
    n, guard, fill = B * V * 3 * H * W, 4096, -7.0
    buf = torch.full((3 * guard + 2 * n,), fill, device=DEV)
    color, color_aug = buf[guard:guard + n], buf[2 * guard + n:2 * guard + 2 * n]
    dev_p = [t.to(DEV) for t in p]
    C.check(lib.pd_resize_crop_augment(B, V, hs, ws, H, W, C.PD_SRC_U8_HWC, C.ptr(frames), *(C.ptr(t) for t in dev_p),
                                       C.ptr(color), C.ptr(color_aug), C.stream_handle(frames.device)), "pd_resize_crop_augment")
    torch.cuda.synchronize()
    want = ops.resize_crop_augment(frames, *p, H, W)
    assert torch.equal(color.view_as(want[0]), want[0]) and torch.equal(color_aug.view_as(want[1]), want[1])
    for lo, hi in ((0, guard), (guard + n, 2 * guard + n), (2 * guard + 2 * n, 3 * guard + 2 * n)):
        assert bool((buf[lo:hi] == fill).all()), (lo, hi)
    depth = torch.rand(B, 1, hs, ws, device=DEV)
    dbuf = torch.full((2 * guard + B * H * W,), fill, device=DEV)
    C.check(lib.pd_resize_crop_nearest(B, hs, ws, H, W, C.ptr(depth), *(C.ptr(t) for t in dev_p[:3]), C.ptr(dbuf[guard:]),
                                       C.stream_handle(depth.device)), "pd_resize_crop_nearest")
    torch.cuda.synchronize()
    assert bool((dbuf[:guard] == fill).all()) and bool((dbuf[guard + B * H * W:] == fill).all())
    assert torch.equal(dbuf[guard:guard + B * H * W].view(B, 1, H, W), ops.resize_crop_depth(depth, *p[:3], H, W))


@gpu
def test_launches_follow_torchs_current_stream():
    hs, ws = 20, 37
    wins = windows(hs, ws)
    p = tensors((hs, ws), wins, flags=[7] * len(wins), V=2)
    frames = noise_frames(4, len(wins), 2, hs, ws, "u8").to(DEV)
    depth = torch.rand(len(wins), 1, hs, ws, device=DEV)
    want = ops.resize_crop_augment(frames, *p, H, W) + (ops.resize_crop_depth(depth, *p[:3], H, W),)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        staged = frames.clone()                                  # produced on the side stream: only a launch there sees it in order
        got = ops.resize_crop_augment(staged, *p, H, W) + (ops.resize_crop_depth(depth, *p[:3], H, W),)
    side.synchronize()
    for a, b in zip(got, want):
        assert torch.equal(a, b)
