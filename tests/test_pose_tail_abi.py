"""pd_pose_tail_fwd/_bwd and ops.pose_matrices / pose_tail / pose_conjugate without a GPU: the host-side refusals, the fp64
restatement of the pose chain that tests/test_pose_tail.py measures the kernels against, and that restatement pinned to the
reference's own numbers (tests/golden/pose_chain.npz, written by tests/golden/make_pose_golden.py).

The restatement (``pose_chain64``) is networks/pose_net.py:148-155, layers.py:17-92 and trainer.py:386-400 in plain torch, double
precision, autograd and all: ``torch.norm`` (gradient 0 at 0), ``axis = vec / (angle + 1e-7)`` without renormalisation, the nine
entries in the reference's operation order, ``torch.inverse(Rc)``.

Error measure (``block_err``): per element |a - b| / A with A the largest |entry| of the element's per-image block in the fp64 value
(a matrix holds exact zeros and entries that cancel: an element-relative figure has no meaning there; this is the A of
tests/test_plane_params.py's homography section).  The rule of tests/test_plane_params.py: E_ref is the reference's fp32 distance
from fp64 in this measure, taken on the CPU when the fixture is made and stored in it; the restatement is held to 2 E_ref + 1e-6.
E_ref itself is capped by E_REF_CAP, which is reasoned, not measured."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from planedepth_amd import _capi as C
from planedepth_amd import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64
FIXTURE = os.path.join(GOLDEN, "pose_chain.npz")
PIN_TOL = 1e-6
# The reference's fp32 chain is a mean over 120 values, ~40 rounded element-wise operations, a 3x3 LU inverse and two 3x3 products at
# cond(Rc) < 10: under 100 roundings of 2^-24 on terms no larger than A, i.e. 6e-6; the adjoint doubles the operation count: 1e-5.
E_REF_CAP = 1e-5
PD_ERR_ARG = 1


def kernel_constants():
    text = open(os.path.join(ROOT, "planedepth_amd", "csrc", "pd_common.h")).read()
    return tuple(int(re.search(r"constexpr int %s = (\d+);" % k, text).group(1)) for k in ("kBlock", "kWave"))


def hw_table():
    """The hw sizes of the parity cases, from the kernel's constants (deduplicated, ascending)."""
    kBlock, kWave = kernel_constants()
    return sorted({1, 2, kWave - 1, kWave, kWave + 1, kBlock - 1, kBlock, kBlock + 1, 120, 480})


def hw_shape(hw):
    return {120: (6, 20), 480: (12, 40)}.get(hw, (1, hw))


# ---------------------------------------------------------------------------------------------------------------------
# the fp64 restatement
# ---------------------------------------------------------------------------------------------------------------------
def rc64(grid):
    """trainer.py:388-394 -> Rc [B,3,3] in fp64."""
    g = grid.double()
    left, right, top, bottom = g[:, 0, 0, 0], g[:, 0, 0, -1], g[:, 1, 0, 0], g[:, 1, -1, 0]
    centre_x, centre_y, half_width = (right + left) / 2., (bottom + top) / 2., (right - left) / 2.
    Rc = torch.eye(3, dtype=F64)[None].repeat(g.shape[0], 1, 1)
    Rc[:, :, 2] = torch.stack([-centre_x / (2 * 0.58), -centre_y / (2 * 1.92), half_width], dim=1)
    return Rc


def rotation64(vec):
    """layers.py:53-92 for vec [B,3] (fp64, differentiable) -> [B,3,3]."""
    angle = torch.norm(vec, 2, 1, True)
    axis = vec / (angle + 1e-7)
    ca, sa = torch.cos(angle)[:, 0], torch.sin(angle)[:, 0]
    Cc = 1 - ca
    x, y, z = axis[:, 0], axis[:, 1], axis[:, 2]
    xs, ys, zs = x * sa, y * sa, z * sa
    xC, yC, zC = x * Cc, y * Cc, z * Cc
    xyC, yzC, zxC = x * yC, y * zC, z * xC
    rows = [x * xC + ca, xyC - zs, zxC + ys, xyC + zs, y * yC + ca, yzC - xs, zxC - ys, yzC + xs, z * zC + ca]
    return torch.stack(rows, 1).view(-1, 3, 3)


def conjugate64(R, grid, t=None):
    """trainer.py:386-400: Rt_Rc [B,4,4] (zeros but for Rc R Rc^-1 and, COLMAP, Rc t) and Rc."""
    Rc = rc64(grid)
    Rt_Rc = torch.zeros(R.shape[0], 4, 4, dtype=F64)
    Rt_Rc[:, :3, :3] = torch.matmul(Rc, torch.matmul(R, torch.inverse(Rc)))
    if t is not None:
        Rt_Rc[:, :3, 3:4] = torch.matmul(Rc, t)
    return Rt_Rc, Rc


def matrices64(vec, grid, invert):
    R = rotation64(vec.double())
    return conjugate64(R.transpose(1, 2) if invert else R, grid)


def pose_chain64(x, grid, invert, frame=0, scale=0.01):
    """x [B,6F,h,w] (any float dtype, widened exactly) -> dict of fp64 tensors; differentiable in x."""
    xd = x.double()
    v = scale * xd[:, 6 * frame:6 * frame + 6].mean(3).mean(2)
    Rt_Rc, Rc = matrices64(v[:, :3], grid, invert)
    return dict(axisangle=v[:, :3], translation=v[:, 3:], Rc=Rc, Rt_Rc=Rt_Rc)


def colmap64(Rt, grid):
    Rt = Rt.double()
    Rt_Rc, Rc = conjugate64(Rt[:, :3, :3], grid, Rt[:, :3, 3:4])
    return dict(Rc=Rc, Rt_Rc=Rt_Rc)


def chain_grads64(x, grid, invert, W, frame=0, scale=0.01):
    """(outputs, d sum(W * Rt_Rc) / d x) of the restatement, fp64."""
    leaf = x.detach().double().requires_grad_(True)
    out = pose_chain64(leaf, grid, invert, frame, scale)
    (out["Rt_Rc"] * W.double()).sum().backward()
    return {k: v.detach() for k, v in out.items()}, leaf.grad


def block_scale(ref64):
    """A per element: the largest |entry| of the element's per-image block."""
    r = ref64.detach().double()
    return r.reshape(r.shape[0], -1).abs().amax(1).reshape((-1,) + (1,) * (r.dim() - 1)).expand_as(r)


def block_err(got, ref64):
    g, r = torch.as_tensor(got).detach().double().cpu(), ref64.detach().double().cpu()
    assert g.shape == r.shape, (tuple(g.shape), tuple(r.shape))
    A = block_scale(r)
    diff = (g - r).abs()
    diff = torch.where(torch.isnan(diff), torch.full_like(diff, float("inf")), diff)
    q = torch.where(A > 0, diff / A.clamp_min(1e-300), torch.where(diff > 0, torch.full_like(diff, float("inf")), diff))
    return float(q.max())


# ---------------------------------------------------------------------------------------------------------------------
# the fixture
# ---------------------------------------------------------------------------------------------------------------------
def load_fixture():
    z = np.load(FIXTURE)
    meta = json.loads(str(z["meta"]))
    return meta, {k: torch.from_numpy(z[k]) for k in z.files if k != "meta"}


def test_fixture_holds_what_the_tests_need():
    meta, t = load_fixture()
    assert meta["B"] == 3 and meta["hw"] == [6, 20] and meta["novel_frame_ids"] == [-1, 1]
    assert os.path.getsize(FIXTURE) < 64 * 1024
    assert tuple(t["x/-1"].shape) == (3, 6, 6, 20) and t["x/-1"].dtype == torch.float32
    g = t["grid"]
    # sample 0 is uncropped (the grid spans [-1, 1] both ways), the others are crops of a resized frame
    assert float(g[0, 0, 0, 0]) == -1 and float(g[0, 0, 0, -1]) == 1 and float(g[0, 1, -1, 0]) == 1
    assert float(g[1, 0, 0, -1] - g[1, 0, 0, 0]) < 1.9 and float(g[2, 1, -1, 0] - g[2, 1, 0, 0]) < 1.9
    for f in meta["novel_frame_ids"]:
        for k in ("axisangle", "translation", "Rc", "Rt", "W", "g_x"):
            assert "%s/%d" % (k, f) in t, (k, f)
        assert tuple(t["axisangle/%d" % f].shape) == (3, 1, 1, 3)
        assert bool((t["Rt/%d" % f][:, 3, :] == 0).all())   # [3,3] included: the reference fills a zeros_like
    for key, e in meta["E_ref"].items():
        assert 0 <= e <= E_REF_CAP, (key, e)


def test_restatement_matches_the_reference_fixture():
    meta, t = load_fixture()
    grid = t["grid"]
    worst = {}
    for f in meta["novel_frame_ids"]:
        out, g_x = chain_grads64(t["x/%d" % f], grid, f < 0, t["W/%d" % f])
        pairs = dict(axisangle=(t["axisangle/%d" % f].view(3, 3), out["axisangle"]),
                     translation=(t["translation/%d" % f].view(3, 3), out["translation"]),
                     Rc=(t["Rc/%d" % f], out["Rc"]), Rt=(t["Rt/%d" % f], out["Rt_Rc"]), g_x=(t["g_x/%d" % f], g_x))
        for k, (ref32, mine) in pairs.items():
            e = block_err(ref32, mine)
            worst[k] = max(worst.get(k, 0.0), e)
            print("frame %+d %-12s err %.3e   E_ref %.3e" % (f, k, e, meta["E_ref"][k]))
            assert e <= 2 * meta["E_ref"][k] + PIN_TOL, (f, k, e, meta["E_ref"][k])
    out = colmap64(t["colmap/Rt_in"], grid)
    for k, ref32 in (("Rc", t["colmap/Rc"]), ("Rt", t["colmap/Rt"])):
        e = block_err(ref32, out["Rc" if k == "Rc" else "Rt_Rc"])
        print("colmap   %-12s err %.3e   E_ref %.3e" % (k, e, meta["E_ref"]["colmap_" + k]))
        assert e <= 2 * meta["E_ref"]["colmap_" + k] + PIN_TOL, (k, e)


def test_restatement_gradient_at_zero_is_zero_and_finite():
    grid = load_fixture()[1]["grid"]
    x = torch.zeros(3, 6, 1, 5)
    W = torch.randn(3, 4, 4, generator=torch.Generator().manual_seed(3))
    for invert in (False, True):
        out, g_x = chain_grads64(x, grid, invert, W)
        assert bool(torch.isfinite(g_x).all()) and bool((g_x == 0).all())
        assert bool(torch.isfinite(out["Rt_Rc"]).all())


def test_restatement_rt_rc_corner_is_zero():
    _, t = load_fixture()
    out = pose_chain64(t["x/1"], t["grid"], False)
    assert bool((out["Rt_Rc"][:, 3, :] == 0).all()) and bool((out["Rt_Rc"][:, :3, 3] == 0).all())
    assert bool((colmap64(t["colmap/Rt_in"], t["grid"])["Rt_Rc"][:, 3, :] == 0).all())


def test_case_table_covers_every_reduction_trip():
    """The kernels' loop is ``for (i = lane; i < hw; i += kBlock)`` followed by a butterfly per wave and a sum over the kBlock / kWave
    waves: the table must hold every trip count a lane can make up to the largest production size (480), lanes that make none, both
    sides of every wave and block boundary, and 1, 2 and all waves holding data."""
    kBlock, kWave = kernel_constants()
    assert kBlock % kWave == 0 and kBlock // kWave >= 2
    table = hw_table()
    src = open(os.path.join(ROOT, "planedepth_amd", "csrc", "pd_pose_tail.hip")).read()
    assert "i += kBlock" in src and "__launch_bounds__(kBlock)" in src and "off = kWave / 2" in src
    trips = {-(-hw // kBlock) for hw in table}
    assert trips == set(range(1, -(-480 // kBlock) + 1)), trips
    assert {min(1, hw // kBlock) for hw in table} == {0, 1}          # a lane with no trip at all / every lane busy
    for edge in (kWave, kBlock):
        assert {edge - 1, edge, edge + 1} <= set(table)
    waves = {min(kBlock // kWave, -(-hw // kWave)) for hw in table}
    assert {1, 2, kBlock // kWave} <= waves, waves
    assert {120, 480} <= set(table) and {1, 2} <= set(table)


# ---------------------------------------------------------------------------------------------------------------------
# host-side refusals: nothing here touches a GPU (the pointers are never dereferenced)
# ---------------------------------------------------------------------------------------------------------------------
_P = ctypes.c_void_p(4096)
_GS = (ctypes.c_int64 * 4)(8, 4, 2, 1)


def _fwd(B=2, Cn=6, hw=4, frame=0, dtype=C.PD_DTYPE_F32, x=_P, Rt=None, grid=_P, gs=_GS, gH=2, gW=2, aa=None, tr=None, out=_P):
    return C.load().pd_pose_tail_fwd(B, Cn, hw, frame, dtype, 0, 0.01, x, Cn * hw, hw, 1, Rt, grid, gH, gW, gs, aa, tr, None, out, None)


def _bwd(B=2, Cn=6, hw=4, frame=0, dtype=C.PD_DTYPE_F32, x=_P, grid=_P, gs=_GS, g=_P, g_aa=None, g_tr=None, g_x=_P):
    return C.load().pd_pose_tail_bwd(B, Cn, hw, frame, dtype, 0, 0.01, x, Cn * hw, hw, 1, grid, 2, 2, gs, g, g_aa, g_tr, g_x,
                                     Cn * hw, hw, 1, None)


REFUSALS = [
    ("B=0", dict(B=0)), ("B<0", dict(B=-1)), ("hw=0", dict(hw=0)), ("hw<0", dict(hw=-3)),
    ("frame<0", dict(frame=-1)), ("frame=F", dict(frame=1)), ("frame=F of 2", dict(Cn=12, frame=2)),
    ("C=5", dict(Cn=5)), ("C=0", dict(Cn=0)), ("C=3 frame 1", dict(Cn=3, frame=1)),
    ("dtype", dict(dtype=7)), ("dtype<0", dict(dtype=-1)),
    ("null x", dict(x=None)), ("null grid", dict(grid=None)), ("null strides", dict(gs=None)),
    ("past 32-bit", dict(Cn=6, hw=(1 << 31) // 6 + 1)), ("past 32-bit, F=2", dict(Cn=12, hw=1 << 28)),
]


@pytest.mark.parametrize("name,kw", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_entry_points_refuse_on_the_host(name, kw):
    lib = C.load()
    assert _fwd(**kw) == PD_ERR_ARG, name
    assert lib.pd_last_error()
    assert _bwd(**kw) == PD_ERR_ARG, name
    assert lib.pd_last_error()


def test_mode_refusals():
    assert _fwd(x=_P, Rt=_P) == PD_ERR_ARG                 # both inputs
    assert _fwd(gH=0) == PD_ERR_ARG and _fwd(gW=0) == PD_ERR_ARG
    assert _fwd(x=None, Rt=_P, aa=_P) == PD_ERR_ARG        # COLMAP mode has no axis-angle
    assert _fwd(Cn=3, tr=_P) == PD_ERR_ARG                 # an axis-angle alone has no translation
    assert _bwd(g_x=None) == PD_ERR_ARG
    assert _bwd(g=None) == PD_ERR_ARG                      # no upstream gradient at all
    assert _bwd(Cn=3, g_tr=_P) == PD_ERR_ARG
    assert b"translation" in C.load().pd_last_error()


def test_ops_refuse_cpu_tensors_and_bad_arguments():
    grid = torch.zeros(2, 2, 4, 5)
    with pytest.raises(C.PlaneDepthHipError):
        ops.pose_matrices(torch.zeros(2, 1, 3), grid)
    with pytest.raises(C.PlaneDepthHipError):
        ops.pose_matrices(torch.zeros(2, 3), grid, invert=True)
    with pytest.raises(C.PlaneDepthHipError):
        ops.pose_tail(torch.zeros(2, 6, 3, 4), grid)
    with pytest.raises(C.PlaneDepthHipError):
        ops.pose_tail(torch.zeros(2, 6, 3, 4, dtype=torch.bfloat16), grid)
    with pytest.raises(C.PlaneDepthHipError):
        ops.pose_conjugate(torch.zeros(2, 4, 4), grid)
    with pytest.raises(ValueError):
        ops.pose_conjugate(torch.zeros(2, 4, 4, requires_grad=True), grid)
    with pytest.raises(ValueError):
        ops.pose_tail(torch.zeros(2, 5, 3, 4), grid)
    with pytest.raises(ValueError):
        ops.pose_tail(torch.zeros(2, 6, 3, 4), grid, frame=1)
    with pytest.raises(ValueError):
        ops.pose_matrices(torch.zeros(2, 2, 3), grid)
    with pytest.raises(ValueError):
        ops.pose_matrices(torch.zeros(2, 3), torch.zeros(3, 2, 4, 5))
    import planedepth_amd
    with pytest.raises(ValueError):
        planedepth_amd.RawPose(torch.zeros(2, 5, 3, 4))
    assert planedepth_amd.RawPose(torch.zeros(2, 6, 3, 4)).out.shape[1] == 6
    assert planedepth_amd.patch_trainer_poses(type("T", (), {})).predict_poses is planedepth_amd.predict_poses
