"""pd_pose_tail_fwd/_bwd through ops.pose_tail / pose_matrices / pose_conjugate and trainer_path.predict_poses on the GPU, per element
against the fp64 restatement of tests/test_pose_tail_abi.py (``pose_chain64``: pinned there to the reference's own fixture).

Bars.  None is taken from a product run.
    forward   the kernels evaluate in fp64 and round once:  |got - ref| <= 2^-23 |ref| + 1e-12 A, one fp32 ulp plus fp64 evaluation
              noise, A = the largest |entry| of the element's matrix / vector — the bar of pd_homography_matrices
              (tests/test_plane_params.py).
    backward  the same with A = the largest magnitude in that gradient tensor: the floor covers the fp64 rounding of the ~200
              operations of the adjoint where terms cancel.
    bf16      the reference is taken on the widened values; outputs as above; g_x within one bf16 rounding: 2^-8 |ref| + 1e-12 A.
    fixture   (trainer level) 2 E_ref + 1e-6 in ``block_err``, as the CPU file pins the restatement: the fixture is the reference's fp32.
PD_POSE_TAIL_PARITY_JSON=<file> writes every figure: the source of profiles/pose_tail_parity.md."""
import json
import os
import types

import pytest
import torch

import planedepth_amd
from planedepth_amd import _capi as C
from planedepth_amd import ops
from test_pose_tail_abi import PIN_TOL, block_err, colmap64, hw_shape, hw_table, load_fixture, matrices64, pose_chain64

DEV = "cuda"
gpu = pytest.mark.gpu
ULP = 2.0 ** -23
BF16_ULP = 2.0 ** -8
NOISE = 1e-12
REPORT = {}


def _record(key, figures):
    REPORT[key] = figures
    path = os.environ.get("PD_POSE_TAIL_PARITY_JSON")
    if path:
        with open(path, "w") as f:
            json.dump(REPORT, f, indent=1, sort_keys=True)


def ulp_report(got, ref64, per_image=True, ulp=ULP):
    """The worst element of |got - ref| / (ulp |ref| + NOISE A); A per image block (forward) or over the whole tensor (gradients)."""
    g, r = got.detach().double().cpu(), ref64.detach().double().cpu()
    assert g.shape == r.shape, (tuple(g.shape), tuple(r.shape))
    if per_image:
        A = r.reshape(r.shape[0], -1).abs().amax(1).reshape((-1,) + (1,) * (r.dim() - 1)).expand_as(r)
    else:
        A = r.abs().max().expand_as(r)
    diff = (g - r).abs()
    diff = torch.where(torch.isnan(diff), torch.full_like(diff, float("inf")), diff)
    allow = ulp * r.abs() + NOISE * A
    over = torch.where(allow > 0, diff / allow.clamp_min(1e-300), torch.where(diff > 0, torch.full_like(diff, float("inf")), diff))
    return float(over.max()) if over.numel() else 0.0


def make_grid(B, seed=0):
    """Grids of crops of resized frames (sample 0: the whole frame), as a view with non-trivial strides when asked."""
    from planedepth_amd.synthetic import crop_grid
    specs = [(7, 9, 0, 0), (13, 19, 3, 5), (11, 31, 2, 17)]
    return torch.stack([crop_grid(7, 9, *specs[(b + seed) % 3]) for b in range(B)], 0)


def conv_output(B, Cn, hw, seed, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    h, w = hw_shape(hw)
    x = torch.randn(B, Cn, h, w, generator=g) * 2 + torch.randn(B, Cn, 1, 1, generator=g) * 4
    return x.to(dtype)


def run_tail(x, grid, invert, frame, W, scale=0.01, g_aa=None, g_tr=None):
    leaf = x.to(DEV).requires_grad_(True)
    aa, tr, Rc, Rt_Rc = ops.pose_tail(leaf, grid.to(DEV), invert=invert, frame=frame, scale=scale)
    loss = (Rt_Rc * W.to(DEV)).sum()
    if g_aa is not None:
        loss = loss + (aa.view(-1, 3) * g_aa.to(DEV)).sum() + (tr.view(-1, 3) * g_tr.to(DEV)).sum()
    loss.backward()
    return dict(axisangle=aa.detach().view(-1, 3), translation=tr.detach().view(-1, 3), Rc=Rc, Rt_Rc=Rt_Rc.detach()), leaf.grad


def check_case(key, x, grid, invert, frame, scale=0.01, with_side_grads=False, g_ulp=ULP):
    B = x.shape[0]
    g = torch.Generator().manual_seed(11)
    W = torch.randn(B, 4, 4, generator=g)
    g_aa = torch.randn(B, 3, generator=g) if with_side_grads else None
    g_tr = torch.randn(B, 3, generator=g) if with_side_grads else None
    got, g_x = run_tail(x, grid, invert, frame, W, scale, g_aa, g_tr)
    leaf = x.detach().double().requires_grad_(True)
    ref = pose_chain64(leaf, grid, invert, frame, scale)
    loss = (ref["Rt_Rc"] * W.double()).sum()
    if with_side_grads:
        loss = loss + (ref["axisangle"] * g_aa.double()).sum() + (ref["translation"] * g_tr.double()).sum()
    loss.backward()
    figures = {k: ulp_report(got[k], ref[k]) for k in ("axisangle", "translation", "Rc", "Rt_Rc")}
    figures["g_x"] = ulp_report(g_x.float(), leaf.grad, per_image=False, ulp=g_ulp)
    print(key, {k: round(v, 4) for k, v in figures.items()})
    _record(key, figures)
    assert g_x.dtype == x.dtype and g_x.shape == x.shape
    for k, v in figures.items():
        assert v <= 1.0, (key, k, v)
    assert bool((got["Rt_Rc"][:, 3, :] == 0).all()) and bool((got["Rt_Rc"][:, :3, 3] == 0).all())
    # exactness of g_x: zeros outside the frame's channels, one value per channel
    gx = g_x.float().cpu()
    outside = [c for c in range(x.shape[1]) if not 6 * frame <= c < 6 * frame + 6]
    assert bool((gx[:, outside] == 0).all()), key
    flat = gx.reshape(B, x.shape[1], -1)
    assert bool((flat == flat[:, :, :1]).all()), key
    if not with_side_grads:
        assert bool((gx[:, 6 * frame + 3:6 * frame + 6] == 0).all()), key   # the matrix does not depend on the translation
    return got, g_x


@gpu
@pytest.mark.parametrize("Cn,frame", [(6, 0), (12, 0), (12, 1)])
@pytest.mark.parametrize("hw", hw_table())
def test_pose_tail_parity(hw, Cn, frame):
    for B in (1, 3):
        for invert in (False, True):
            x = conv_output(B, Cn, hw, seed=hw * 7 + Cn + frame + B)
            check_case("tail hw%d C%d f%d B%d inv%d" % (hw, Cn, frame, B, invert), x, make_grid(B, hw), invert, frame)


@gpu
@pytest.mark.parametrize("hw", [1, 120, 480])
def test_pose_tail_parity_with_axisangle_and_translation_gradients(hw):
    x = conv_output(3, 12, hw, seed=5)
    check_case("tail+side hw%d" % hw, x, make_grid(3), True, 1, with_side_grads=True)


@gpu
@pytest.mark.parametrize("hw", hw_table())
def test_pose_tail_bf16(hw):
    for invert in (False, True):
        x = conv_output(3, 12, hw, seed=hw + 1, dtype=torch.bfloat16)
        check_case("bf16 hw%d inv%d" % (hw, invert), x, make_grid(3), invert, 1, g_ulp=BF16_ULP)


@gpu
def test_pose_tail_channels_last_and_strided_grid():
    x = conv_output(3, 12, 120, seed=9).contiguous(memory_format=torch.channels_last)
    big = torch.zeros(3, 3, 9, 20)
    big[:, 1:3, 1:8, 2:20:2] = make_grid(3)
    grid_view = big.to(DEV)[:, 1:3, 1:8, 2:20:2]
    assert not grid_view.is_contiguous()
    got, g_x = check_case("channels_last", x, make_grid(3), False, 1)
    leaf = x.to(DEV).requires_grad_(True)
    aa, tr, Rc, Rt_Rc = ops.pose_tail(leaf, grid_view, frame=1)
    assert torch.equal(Rt_Rc, got["Rt_Rc"]) and torch.equal(Rc, got["Rc"])
    assert g_x.is_contiguous(memory_format=torch.channels_last)


MAGNITUDES = [0.0, 1e-8, 1e-6, 1e-3, 0.1, 3.0]


@gpu
@pytest.mark.parametrize("mag", MAGNITUDES)
def test_pose_tail_small_and_large_angles(mag):
    """|vec| through a constant conv output.  Below 1e-5 the ``+ 1e-7`` of ``axis = vec / (angle + 1e-7)`` matters: the axis is
    shorter than 1 there and a renormalised axis fails this test."""
    u = torch.tensor([0.36, -0.48, 0.8])
    for hw in (1, 120):
        h, w = hw_shape(hw)
        x = torch.zeros(3, 6, h, w)
        x[:, :3] = (u * mag / 0.01).view(1, 3, 1, 1)
        x[:, 3:] = 1.5
        for invert in (False, True):
            got, g_x = check_case("mag %g hw%d inv%d" % (mag, hw, invert), x, make_grid(3), invert, 0)
            assert bool(torch.isfinite(g_x).all())
            if mag == 0.0:
                assert bool((g_x == 0).all())


@gpu
@pytest.mark.parametrize("invert", [False, True])
def test_pose_matrices_strided_axisangle(invert):
    """The reference's ``axisangle[:, 0]``: a [B,1,3] slice of a [B,1,1,6] tensor, batch stride 6, read in place (hw = 1, scale = 1)."""
    B = 3
    g = torch.Generator().manual_seed(4)
    both = (torch.randn(B, 1, 1, 6, generator=g) * 0.05).to(DEV).requires_grad_(True)
    axisangle = both[..., :3][:, 0]
    assert axisangle.stride(0) == 6 and tuple(axisangle.shape) == (B, 1, 3)
    grid = make_grid(B)
    W = torch.randn(B, 4, 4, generator=g)
    Rt_Rc, Rc = ops.pose_matrices(axisangle, grid.to(DEV), invert=invert)
    (Rt_Rc * W.to(DEV)).sum().backward()
    leaf = both.detach().cpu().double().requires_grad_(True)
    ref, ref_Rc = matrices64(leaf[:, 0, 0, :3], grid, invert)
    (ref * W.double()).sum().backward()
    figures = dict(Rt_Rc=ulp_report(Rt_Rc, ref), Rc=ulp_report(Rc, ref_Rc), g=ulp_report(both.grad, leaf.grad, per_image=False))
    print(figures)
    _record("matrices inv%d" % invert, figures)
    assert max(figures.values()) <= 1.0, figures
    assert bool((both.grad[..., 3:] == 0).all())
    # [B,3], contiguous, gives the same bits
    flat = both.detach()[:, 0, 0, :3].contiguous()
    assert torch.equal(ops.pose_matrices(flat, grid.to(DEV), invert=invert)[0], Rt_Rc)


@gpu
def test_pose_conjugate_colmap():
    _, t = load_fixture()
    Rt, grid = t["colmap/Rt_in"], t["grid"]
    Rt_Rc, Rc = ops.pose_conjugate(Rt.to(DEV), grid.to(DEV))
    ref = colmap64(Rt, grid)
    figures = dict(Rt_Rc=ulp_report(Rt_Rc, ref["Rt_Rc"]), Rc=ulp_report(Rc, ref["Rc"]))
    _record("colmap", figures)
    assert max(figures.values()) <= 1.0, figures
    assert bool((Rt_Rc[:, 3, :] == 0).all())
    assert not Rt_Rc.requires_grad
    with pytest.raises(ValueError):
        ops.pose_conjugate(Rt.to(DEV).requires_grad_(True), grid.to(DEV))


@gpu
def test_pose_tail_is_deterministic():
    x, grid, W = conv_output(3, 12, 480, seed=2), make_grid(3), torch.randn(3, 4, 4, generator=torch.Generator().manual_seed(1))
    a, ga = run_tail(x, grid, True, 1, W)
    b, gb = run_tail(x, grid, True, 1, W)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert torch.equal(ga, gb)


@gpu
def test_pose_ops_do_not_sync_the_host():
    x = conv_output(3, 6, 120, seed=3).to(DEV).requires_grad_(True)
    grid = make_grid(3).to(DEV)
    W = torch.randn(3, 4, 4, device=DEV)
    Rt = torch.eye(4, device=DEV)[None].repeat(3, 1, 1)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):   # the mode reports on this build: a deliberate sync is caught
            W.sum().item()
        aa, tr, Rc, Rt_Rc = ops.pose_tail(x, grid, invert=True)
        (Rt_Rc * W).sum().backward()
        ops.pose_matrices(aa.detach()[:, 0], grid)
        ops.pose_conjugate(Rt, grid)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(x.grad).all())


# ---------------------------------------------------------------------------------------------------------------------
# trainer level
# ---------------------------------------------------------------------------------------------------------------------
class _StockDecoder(torch.nn.Module):
    """The stock return convention of PoseDecoder.forward on an identity 'network': (axisangle, translation) [B,1,1,3]."""

    def forward(self, feats, grid):
        out = feats[0][-1].mean(3).mean(2)
        out = 0.01 * out.view(-1, 1, 1, 6)
        return out[..., :3], out[..., 3:]


class _RawDecoder(torch.nn.Module):
    def forward(self, feats, grid):
        return planedepth_amd.RawPose(feats[0][-1])


def _stub_trainer(decoder, leafs, novel, use_colmap=False):
    cls = planedepth_amd.patch_trainer_poses(type("StubTrainer", (), {}))
    tr = cls()
    tr.opt = types.SimpleNamespace(novel_frame_ids=novel, use_colmap=use_colmap)
    order = iter(novel)
    tr.models = {"pose_encoder": lambda images: [leafs[next(order)]], "pose": decoder}
    return tr


@gpu
@pytest.mark.parametrize("decoder", [_StockDecoder, _RawDecoder], ids=["stock", "rawpose"])
def test_predict_poses_reproduces_the_reference_fixture(decoder):
    meta, t = load_fixture()
    novel = meta["novel_frame_ids"]
    leafs = {f: t["x/%d" % f].to(DEV).requires_grad_(True) for f in novel}
    color = torch.zeros(3, 3, 2, 2, device=DEV)
    inputs = {"grid": t["grid"].to(DEV), ("Rt", "r"): torch.eye(4, device=DEV)[None].repeat(3, 1, 1), ("color_aug", "l"): color}
    inputs.update({("color_aug", f): color for f in novel})
    outputs = _stub_trainer(decoder(), leafs, novel).predict_poses(inputs)
    want_keys = {("Rt", "r")} | {(k, f) for f in novel for k in ("axisangle", "translation", "Rc", "Rt")}
    assert set(outputs) == want_keys
    assert outputs[("Rt", "r")] is inputs[("Rt", "r")]
    figures = {}
    for f in novel:
        (outputs[("Rt", f)] * t["W/%d" % f].to(DEV)).sum().backward()
        for k, fx in (("axisangle", "axisangle"), ("translation", "translation"), ("Rc", "Rc"), ("Rt", "Rt")):
            got, ref32 = outputs[(k, f)], t["%s/%d" % (fx, f)]
            assert tuple(got.shape) == tuple(ref32.shape), (k, f, tuple(got.shape))
            lead = got.shape[0]
            e = block_err(got.reshape(lead, -1), ref32.double().reshape(lead, -1))
            figures["%s/%d" % (k, f)] = e
            assert e <= 2 * meta["E_ref"][k] + PIN_TOL, (k, f, e)
        e = block_err(leafs[f].grad, t["g_x/%d" % f].double())
        figures["g_x/%d" % f] = e
        assert e <= 2 * meta["E_ref"]["g_x"] + PIN_TOL, (f, e)
    print(figures)
    _record("trainer " + decoder.__name__, figures)


@gpu
def test_predict_poses_rawpose_with_two_predicted_frames():
    """A decoder built with num_frames_to_predict_for = 2: ``axisangle`` / ``translation`` are the reference's [B,2,1,3], the matrix
    is frame 0's (``axisangle[:, 0]``)."""
    x, grid = conv_output(3, 12, 120, seed=23), make_grid(3)
    leafs = {1: x.to(DEV).requires_grad_(True)}
    color = torch.zeros(3, 3, 2, 2, device=DEV)
    inputs = {"grid": grid.to(DEV), ("Rt", "r"): torch.eye(4, device=DEV)[None].repeat(3, 1, 1), ("color_aug", "l"): color,
              ("color_aug", 1): color}
    outputs = _stub_trainer(_RawDecoder(), leafs, [1]).predict_poses(inputs)
    assert tuple(outputs[("axisangle", 1)].shape) == (3, 2, 1, 3) and tuple(outputs[("translation", 1)].shape) == (3, 2, 1, 3)
    for frame in (0, 1):
        ref = pose_chain64(x, grid, False, frame)
        assert ulp_report(outputs[("axisangle", 1)][:, frame, 0], ref["axisangle"]) <= 1.0
        assert ulp_report(outputs[("translation", 1)][:, frame, 0], ref["translation"]) <= 1.0
    assert ulp_report(outputs[("Rt", 1)], pose_chain64(x, grid, False, 0)["Rt_Rc"]) <= 1.0


@gpu
def test_predict_poses_colmap():
    _, t = load_fixture()
    meta = load_fixture()[0]
    inputs = {"grid": t["grid"].to(DEV), ("Rt", "r"): torch.eye(4, device=DEV)[None].repeat(3, 1, 1),
              ("Rt", 1): t["colmap/Rt_in"].to(DEV)}
    outputs = _stub_trainer(None, {}, [1], use_colmap=True).predict_poses(inputs)
    assert set(outputs) == {("Rt", "r"), ("Rc", 1), ("Rt", 1)}
    for k in ("Rc", "Rt"):
        e = block_err(outputs[(k, 1)], t["colmap/" + k].double())
        assert e <= 2 * meta["E_ref"]["colmap_" + k] + PIN_TOL, (k, e)


# ---------------------------------------------------------------------------------------------------------------------
# end to end: the fused T into the plane-uniform homography algebra
# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("invert", [False, True])
def test_gradient_through_uniform_homographies(invert):
    """conv output -> T -> homography_matrices_fused(PD_HMAT_UNIFORM) -> sum(g_H * H): the gradient on the conv output against the
    torch chain (the fp64 restatement, cast to fp32) feeding the same operator.

    Composition of the bars.  Forward: both T are within one ulp of the fp64 value (the torch arm's is its rounding: half an ulp), so
    they differ by at most 1.5 ulp per element — asserted.  The homography operator is deterministic, but its g_T moves with T at the
    conditioning of K (H W ~ 1e3): a 1.5 ulp difference in T would enter g_x amplified by a factor that belongs to that operator, not
    to the pose path.  So the torch arm hands the operator the fused arm's T bits (value snapped by the <= 1.5 ulp just asserted, the
    gradient path untouched): g_T is then the same bits in both arms, and what is left between the two g_x is the pose adjoint alone —
    the backward bar, one fp32 ulp + 1e-12 of the largest magnitude in g_x."""
    from planedepth_amd.synthetic import dataset_intrinsics
    B, N = 3, 5
    g = torch.Generator().manual_seed(17)
    x = conv_output(B, 6, 120, seed=31)
    grid = make_grid(B)
    K, inv_K = (m.to(DEV) for m in dataset_intrinsics(B, 24, 80))
    distance = (torch.rand(B, N, generator=g) * 3 + 1).to(DEV)
    norm = torch.nn.functional.normalize(torch.randn(B, N, 3, generator=g) * 0.1 + torch.tensor([0.0, 0.0, 1.0]), dim=-1).to(DEV)
    g_H = torch.randn(B, 4, 3, 3, generator=g).to(DEV)

    leaf = x.to(DEV).requires_grad_(True)
    T = ops.pose_tail(leaf, grid.to(DEV), invert=invert)[3]
    H, _ = ops.homography_matrices_fused(distance, norm, T, K, inv_K, C.PD_HMAT_UNIFORM)
    (H * g_H).sum().backward()

    leaf64 = x.detach().double().requires_grad_(True)
    T64 = pose_chain64(leaf64, grid, invert)["Rt_Rc"]
    assert ulp_report(T, T64) <= 1.0
    T_torch = T64.float().to(DEV)
    assert float(((T.detach() - T_torch.detach()).abs() / (1.5 * ULP * T64.detach().abs().to(DEV) + NOISE)).max()) <= 1.0
    T_arm = T.detach().clone().requires_grad_(True)   # the fused arm's bits, a leaf in front of the operator
    H2, _ = ops.homography_matrices_fused(distance, norm, T_arm, K, inv_K, C.PD_HMAT_UNIFORM)
    assert torch.equal(H2, H)
    (H2 * g_H).sum().backward()
    T64.backward(T_arm.grad.cpu().double())   # the torch chain's own adjoint, in fp64, from the operator's g_T
    worst = ulp_report(leaf.grad, leaf64.grad, per_image=False)
    print("g_x through the uniform homographies: %.4f of the bar" % worst)
    _record("end_to_end inv%d" % invert, dict(g_x=worst))
    assert worst <= 1.0
    assert float(leaf.grad.abs().max()) > 0
