"""CPU checks of pd_render_poses' C ABI and of the Python layers above it: the header, the ctypes table and the library agree; the
workspace size has its closed form; every refusal happens in argument validation, with a text that names the offending argument
or flag — nothing launches, so none of this needs a GPU; ``ops.render_poses`` and ``predict.render_poses`` refuse CPU tensors,
inputs that require grad (with gradients enabled), a dense mask without ``tail_applied`` and a ``T`` of the wrong shape."""
import ctypes

import pytest
import torch

import capi_header
import planedepth_amd
from planedepth_amd import _capi as C
from planedepth_amd import ops
from planedepth_amd import predict as predict_module   # (the package re-exports the function over the module's name)

P = ctypes.c_void_p
PTR = P(256)   # never dereferenced: every call below is refused before a launch
MIX = C.PD_TAIL_MIXTURE
POINTERS = ("logits", "sigma", "mask", "distance", "norm", "T", "K", "inv_K", "image", "rgb", "coverage", "disp", "workspace")


def _entry(B=2, N=5, H=8, W=16, V=1, flags=MIX, **over):
    ptrs = dict.fromkeys(POINTERS, PTR)
    ptrs.update(mask=None, coverage=None, disp=None)
    ptrs.update(over)
    lib = C.load()
    rc = lib.pd_render_poses(B, N, H, W, V, flags, *[ptrs[k] for k in POINTERS], None)
    return rc, lib.pd_last_error()


def test_header_capi_and_library_agree():
    lib = C.load()
    assert capi_header.params("pd_render_poses") == [
        "int B", "int N", "int H", "int W", "int V", "int flags", "const float* logits_in", "const float* sigma_in",
        "const float* mask_rows", "const float* distance", "const float* norm", "const float* T", "const float* K",
        "const float* inv_K", "const float* image", "float* rgb", "float* coverage", "float* disp", "float* workspace",
        "pd_stream_t stream"]
    assert C.SIGNATURES["pd_render_poses"] == (ctypes.c_int, [ctypes.c_int] * 6 + [P] * 14)
    assert capi_header.params("pd_render_poses_workspace_floats") == ["int B", "int N", "int V"]
    assert C.SIGNATURES["pd_render_poses_workspace_floats"] == (ctypes.c_size_t, [ctypes.c_int] * 3)
    assert hasattr(lib, "pd_render_poses") and hasattr(lib, "pd_render_poses_workspace_floats")


def test_constants_and_exports():
    assert C.PD_RENDER_VISIBLE_ONLY == 1 << 9 and C.PD_RENDER_TAIL_APPLIED == 1 << 8
    tail_flags = C.PD_TAIL_MIXTURE | C.PD_TAIL_DISP_DENSE | C.PD_TAIL_BF16 | C.PD_TAIL_DISP_ROWS | C.PD_TAIL_MASK_ROWS
    assert C.PD_RENDER_VISIBLE_ONLY & (tail_flags | C.PD_RENDER_TAIL_APPLIED) == 0
    assert callable(ops.render_poses)
    assert planedepth_amd.predict.render_poses is predict_module.render_poses


def test_workspace_closed_form():
    """Host only: 16 floats per (image, view, plane)."""
    lib = C.load()
    for B, N, V in ((1, 1, 1), (2, 5, 3), (8, 63, 4), (3, 49, 17)):
        assert lib.pd_render_poses_workspace_floats(B, N, V) == 16 * B * V * N
    assert lib.pd_render_poses_workspace_floats(8, 63, 8191) == 16 * 8 * 63 * 8191   # (beyond 2^25: no 32-bit product inside)
    for bad in ((0, 5, 1), (2, 0, 1), (2, 5, 0), (2, 5, -1)):
        assert lib.pd_render_poses_workspace_floats(*bad) == 0


def test_view_count():
    for V in (0, -1):
        rc, msg = _entry(V=V)
        assert rc == C.PD_ERR_ARG and b"V = %d" % V in msg, V
    rc, msg = _entry(B=256, V=256)
    assert rc == C.PD_ERR_ARG and b"B*V = 65536" in msg and b"grid" in msg
    rc, msg = _entry(B=255, V=257, workspace=None)    # 65535 pairs fit: the next refusal in line speaks
    assert b"B*V" not in msg and b"workspace" in msg


def test_flags():
    for flag, name in ((C.PD_TAIL_DISP_ROWS, b"PD_TAIL_DISP_ROWS"), (C.PD_TAIL_DISP_DENSE, b"PD_TAIL_DISP_DENSE")):
        rc, msg = _entry(flags=MIX | flag)
        assert rc == C.PD_ERR_ARG and name in msg and b"distance / norm" in msg, name
    for unknown in (32, 64, 128, 1024):
        rc, msg = _entry(flags=MIX | unknown)
        assert rc == C.PD_ERR_ARG and b"flags" in msg, unknown
    rc, msg = _entry(flags=MIX | C.PD_TAIL_MASK_ROWS, mask=None)
    assert rc == C.PD_ERR_ARG and b"PD_TAIL_MASK_ROWS" in msg and b"mask_rows" in msg and b"NULL" in msg
    rc, msg = _entry(flags=MIX, mask=PTR)
    assert rc == C.PD_ERR_ARG and b"mask_rows without PD_TAIL_MASK_ROWS" in msg
    # every legal combination gets past the flag checks (and stops at the NULL workspace)
    for flags in (0, MIX, MIX | C.PD_TAIL_BF16, MIX | C.PD_RENDER_TAIL_APPLIED, MIX | C.PD_RENDER_VISIBLE_ONLY,
                  C.PD_RENDER_TAIL_APPLIED | C.PD_RENDER_VISIBLE_ONLY | C.PD_TAIL_BF16):
        rc, msg = _entry(flags=flags, workspace=None)
        assert rc == C.PD_ERR_ARG and b"workspace" in msg, flags
    rc, msg = _entry(flags=MIX | C.PD_TAIL_MASK_ROWS, mask=PTR, workspace=None)
    assert rc == C.PD_ERR_ARG and b"workspace" in msg


def test_pointers_and_shapes():
    rc, msg = _entry(sigma=None)
    assert rc == C.PD_ERR_ARG and b"sigma_in" in msg and b"PD_TAIL_MIXTURE" in msg
    rc, msg = _entry(flags=0, sigma=None, workspace=None)        # (no mixture: sigma_in may be NULL; the workspace may not)
    assert rc == C.PD_ERR_ARG and b"workspace" in msg
    for name in ("workspace", "T", "K", "inv_K", "distance", "norm"):
        rc, msg = _entry(**{name: None})
        assert rc == C.PD_ERR_ARG and b"NULL" in msg and b"(%s:" % name.encode() in msg, name
    for name, text in (("logits", b"logits_in"), ("image", b"image"), ("rgb", b"rgb")):
        rc, msg = _entry(**{name: None})
        assert rc == C.PD_ERR_ARG and b"NULL" in msg and text in msg, name
    for bad in (dict(B=0), dict(N=0), dict(H=0), dict(W=-1), dict(H=1), dict(W=1)):
        rc, msg = _entry(**bad)
        assert rc == C.PD_ERR_ARG and b"shape" in msg and b"H >= 2, W >= 2" in msg, bad
    rc, msg = _entry(N=1 << 11, H=1 << 10, W=1 << 10)
    assert rc == C.PD_ERR_ARG and b"N*H*W" in msg
    rc, msg = _entry(N=(1 << 11) - 1, H=1 << 10, W=1 << 10, logits=P(258))   # one plane fewer fits: the next refusal speaks
    assert rc == C.PD_ERR_ARG and b"N*H*W" not in msg and b"misaligned" in msg


def test_alignment_is_the_tails_rule():
    """fp32 tensors on 4 bytes, bf16 conv outputs on 2."""
    for name in ("logits", "sigma"):
        rc, msg = _entry(**{name: P(258)})
        assert rc == C.PD_ERR_ARG and b"misaligned" in msg and b"logits_in / sigma_in" in msg and b"4-byte" in msg, name
        rc, msg = _entry(flags=MIX | C.PD_TAIL_BF16, **{name: P(257)})
        assert rc == C.PD_ERR_ARG and b"misaligned" in msg and b"2-byte" in msg, name
        rc, msg = _entry(flags=MIX | C.PD_TAIL_BF16, rgb=P(258), **{name: P(258)})   # legal for bf16: rgb speaks instead
        assert b"logits_in" not in msg and b"rgb" in msg
    for name in ("distance", "norm", "T", "K", "inv_K", "image", "workspace"):
        rc, msg = _entry(**{name: P(258)})
        assert rc == C.PD_ERR_ARG and b"misaligned" in msg and name.encode() in msg and b"4-byte" in msg, name
    for name in ("rgb", "coverage", "disp"):
        rc, msg = _entry(**{name: P(258)})
        assert rc == C.PD_ERR_ARG and b"misaligned" in msg and b"rgb, coverage, disp" in msg, name
    rc, msg = _entry(flags=MIX | C.PD_TAIL_MASK_ROWS, mask=P(257))
    assert rc == C.PD_ERR_ARG and b"misaligned" in msg and b"mask_rows" in msg


def _cpu_inputs(B=1, N=3, H=2, W=4, V=2):
    g = torch.Generator().manual_seed(3)
    rl, rs = torch.randn(B, N, H, W, generator=g), torch.randn(B, N, H, W, generator=g)
    distance = (torch.arange(N, dtype=torch.float32) + 1.0).view(1, N).expand(B, N).contiguous()
    norm = torch.tensor([0.0, 0.0, 1.0]).view(1, 1, 3).expand(B, N, 3).contiguous()
    T = torch.eye(4).view(1, 1, 4, 4).repeat(B, V, 1, 1)
    K = torch.eye(4).view(1, 4, 4).repeat(B, 1, 1)
    return dict(raw_logits=rl, raw_sigma=rs, padding_mask=None, distance=distance, norm=norm,
                image=torch.rand(B, 3, H, W, generator=g), T=T, K=K, inv_K=K.clone())


def test_operator_refuses_cpu_tensors():
    a = _cpu_inputs()
    with torch.no_grad():
        with pytest.raises(C.PlaneDepthHipError, match="GPU only"):
            ops.render_poses(**a)
        with pytest.raises(C.PlaneDepthHipError, match="GPU only"):
            ops.render_poses(**dict(a, raw_sigma=None, T=a["T"][0]), use_mixture_loss=False, tail_applied=True, visible_only=True)
        with pytest.raises(C.PlaneDepthHipError, match="GPU only"):
            planedepth_amd.predict.render_poses(lambda x, grids: {}, a["image"], a["T"])


def test_operator_refuses_inputs_that_require_grad():
    a = _cpu_inputs()
    for name in ("raw_logits", "raw_sigma", "distance", "norm", "image", "T", "K", "inv_K"):
        args = dict(a, **{name: a[name].clone().requires_grad_(True)})
        with pytest.raises(ValueError, match=r"%s requires grad, but render_poses is forward-only.*ops\.plane_sweep_homography," % name):
            ops.render_poses(**args)
    with torch.no_grad():   # under no_grad the same tensors get as far as the device check
        with pytest.raises(C.PlaneDepthHipError, match="GPU only"):
            ops.render_poses(**dict(a, raw_logits=a["raw_logits"].clone().requires_grad_(True)))


def test_operator_checks_its_arguments_before_the_device():
    a = _cpu_inputs()
    B, N, H, W = a["raw_logits"].shape
    with torch.no_grad():
        with pytest.raises(ValueError, match="want"):
            ops.render_poses(**a, want=("depth",))
        for bad in (torch.eye(4), a["T"][:, :, :3], torch.eye(4).view(1, 1, 4, 4).repeat(B + 1, 2, 1, 1), a["T"][:, :0], None):
            with pytest.raises(ValueError, match=r"T must be \[B,V,4,4\].*or \[V,4,4\]"):
                ops.render_poses(**dict(a, T=bad))
        with pytest.raises(TypeError, match="float32 or torch.bfloat16"):
            ops.render_poses(**dict(a, raw_logits=a["raw_logits"].half(), raw_sigma=a["raw_sigma"].half()))
        with pytest.raises(TypeError, match="one dtype"):
            ops.render_poses(**dict(a, raw_logits=a["raw_logits"].bfloat16()))
        dense = torch.ones(B, N, H, W)
        with pytest.raises(C.PlaneDepthHipError, match="padding_mask is a dense.*tail_applied"):
            ops.render_poses(**dict(a, padding_mask=dense))
        with pytest.raises(C.PlaneDepthHipError, match="GPU only"):    # with tail_applied no mask is read: the dense mask passes
            ops.render_poses(**dict(a, padding_mask=dense), tail_applied=True)
        with pytest.raises(C.PlaneDepthHipError, match="GPU only"):    # a row view passes as well
            ops.render_poses(**dict(a, padding_mask=ops.row_view(torch.ones(B, N, H), W)))
