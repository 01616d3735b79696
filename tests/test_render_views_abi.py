"""CPU checks of pd_render_views' C ABI and of the Python layers above it: the header, the ctypes table and the library agree;
every refusal happens in argument validation, with a text that names the offending argument or flag — nothing launches, so none
of this needs a GPU; ``ops.render_views`` and ``predict.render`` refuse CPU tensors and, with gradients enabled, inputs that
require grad."""
import ctypes

import pytest
import torch

import capi_header
import planedepth_amd
from planedepth_amd import _capi as C
from planedepth_amd import decoder_tail as DT
from planedepth_amd import ops
from planedepth_amd import predict as predict_module   # (the package re-exports the function over the module's name)

P = ctypes.c_void_p
PTR = P(256)   # never dereferenced: every call below is refused before a launch
MIX = C.PD_TAIL_MIXTURE


def _entry(B=2, N=5, H=8, W=16, V=1, flags=MIX, logits=PTR, sigma=PTR, mask=None, dl=PTR, image=PTR, baselines=(1.0,), rgb=PTR,
           coverage=None, disp=None):
    lib = C.load()
    arr = None if baselines is None else (ctypes.c_float * max(len(baselines), 1))(*baselines)   # a HOST array: it is read
    rc = lib.pd_render_views(B, N, H, W, V, flags, logits, sigma, mask, dl, image, arr, rgb, coverage, disp, None)
    return rc, lib.pd_last_error()


def test_header_capi_and_library_agree():
    lib = C.load()
    assert capi_header.params("pd_render_views") == [
        "int B", "int N", "int H", "int W", "int V", "int flags", "const float* logits_in", "const float* sigma_in",
        "const float* mask_rows", "const float* disp_layered", "const float* image", "const float* baselines", "float* rgb",
        "float* coverage", "float* disp", "pd_stream_t stream"]
    assert C.SIGNATURES["pd_render_views"] == (ctypes.c_int, [ctypes.c_int] * 6 + [P] * 10)
    assert hasattr(lib, "pd_render_views")
    assert capi_header.params("pd_render_cols_per_lane") == ["int W", "int V"]
    assert C.SIGNATURES["pd_render_cols_per_lane"] == (ctypes.c_int, [ctypes.c_int] * 2)
    assert lib.pd_render_cols_per_lane(640, 1) == 2 and lib.pd_render_cols_per_lane(640, 4) == 1   # host only: no GPU asked
    assert [lib.pd_render_cols_per_lane(W, 1) for W in (1, 2, 2048, 2049)] == [0, 1, 2, 0]
    assert lib.pd_render_cols_per_lane(640, 0) == 0 and lib.pd_render_cols_per_lane(640, C.PD_RENDER_MAX_VIEWS + 1) == 0


def test_constants_are_module_attributes():
    assert C.PD_RENDER_MAX_VIEWS == 4
    assert C.PD_RENDER_TAIL_APPLIED == 1 << 8
    tail_flags = C.PD_TAIL_MIXTURE | C.PD_TAIL_DISP_DENSE | C.PD_TAIL_BF16 | C.PD_TAIL_DISP_ROWS | C.PD_TAIL_MASK_ROWS
    assert C.PD_RENDER_TAIL_APPLIED & tail_flags == 0          # ORed with pd_tail_flags
    assert callable(ops.render_views) and ops.Views._fields == ("rgb", "coverage", "disp")
    assert planedepth_amd.predict.render is predict_module.render


def test_view_count_and_baselines():
    for V in (0, -1, 5, 64):
        rc, msg = _entry(V=V, baselines=(1.0,) * 8)
        assert rc == C.PD_ERR_ARG and b"V = %d" % V in msg and b"PD_RENDER_MAX_VIEWS" in msg, V
    for bad in (float("nan"), float("inf"), float("-inf")):
        rc, msg = _entry(V=3, baselines=(1.0, -1.0, bad))
        assert rc == C.PD_ERR_ARG and b"baselines[2]" in msg and b"finite" in msg, bad
    rc, msg = _entry(baselines=None)
    assert rc == C.PD_ERR_ARG and b"NULL" in msg and b"baselines" in msg


def test_forms_out_of_scope_are_refused_by_name():
    rc, msg = _entry(flags=MIX | C.PD_TAIL_DISP_DENSE)
    assert rc == C.PD_ERR_UNSUPPORTED and b"PD_TAIL_DISP_DENSE" in msg and b"yz planes" in msg
    rc, msg = _entry(flags=MIX | C.PD_TAIL_MASK_ROWS, mask=None)
    assert rc == C.PD_ERR_ARG and b"PD_TAIL_MASK_ROWS" in msg and b"mask_rows" in msg and b"NULL" in msg
    rc, msg = _entry(flags=MIX, mask=PTR)
    assert rc == C.PD_ERR_ARG and b"mask_rows without PD_TAIL_MASK_ROWS" in msg
    rc, msg = _entry(flags=MIX | 32)
    assert rc == C.PD_ERR_ARG and b"flags" in msg
    rc, msg = _entry(flags=MIX | 512)
    assert rc == C.PD_ERR_ARG and b"flags" in msg
    rc, msg = _entry(W=2049)
    assert rc == C.PD_ERR_UNSUPPORTED and b"W = 2049" in msg


def test_pointers_and_shapes():
    rc, msg = _entry(sigma=None)
    assert rc == C.PD_ERR_ARG and b"sigma_in" in msg and b"PD_TAIL_MIXTURE" in msg
    rc, msg = _entry(flags=0, sigma=None, rgb=None)              # (no mixture: sigma_in may be NULL; rgb may not)
    assert rc == C.PD_ERR_ARG and b"rgb" in msg and b"NULL" in msg
    for name in ("logits", "dl", "image"):
        rc, msg = _entry(**{name: None})
        assert rc == C.PD_ERR_ARG and b"NULL" in msg, name
    for bad in (dict(B=0), dict(N=0), dict(H=0), dict(W=-1), dict(B=65536), dict(H=1), dict(W=1)):
        rc, msg = _entry(**bad)
        assert rc == C.PD_ERR_ARG and b"shape" in msg, bad
    rc, msg = _entry(N=1 << 11, H=1 << 10, W=1 << 10)
    assert rc == C.PD_ERR_ARG and b"N*H*W" in msg
    rc, msg = _entry(N=(1 << 11) - 1, H=1 << 10, W=1 << 10, V=0)   # one plane fewer fits: the next refusal in line speaks
    assert b"N*H*W" not in msg


def test_alignment_is_the_tails_rule():
    """fp32 tensors on 4 bytes, bf16 conv outputs on 2."""
    for name in ("logits", "sigma"):
        rc, msg = _entry(**{name: P(258)})
        assert rc == C.PD_ERR_ARG and b"misaligned" in msg and b"logits_in / sigma_in" in msg, name
        rc, msg = _entry(flags=MIX | C.PD_TAIL_BF16, **{name: P(257)})
        assert rc == C.PD_ERR_ARG and b"misaligned" in msg and b"2-byte" in msg, name
        rc, msg = _entry(flags=MIX | C.PD_TAIL_BF16, V=0, **{name: P(258)})   # legal for bf16: V speaks instead
        assert b"misaligned" not in msg
    for name in ("dl", "rgb", "coverage", "disp"):
        rc, msg = _entry(**{name: P(258)})
        assert rc == C.PD_ERR_ARG and b"misaligned" in msg and b"4-byte" in msg, name
    rc, msg = _entry(flags=MIX | C.PD_TAIL_MASK_ROWS, mask=P(257))
    assert rc == C.PD_ERR_ARG and b"misaligned" in msg
    rc, msg = _entry(image=P(130))
    assert rc == C.PD_ERR_ARG and b"misaligned" in msg and b"image" in msg


def _cpu_inputs(B=1, N=3, H=2, W=4):
    g = torch.Generator().manual_seed(3)
    rl, rs = torch.randn(B, N, H, W, generator=g), torch.randn(B, N, H, W, generator=g)
    dl = (torch.arange(N, dtype=torch.float32) + 1.0).view(1, N, 1, 1).expand(B, N, H, W)
    return rl, rs, dl, torch.rand(B, 3, H, W, generator=g)


def test_operator_refuses_cpu_tensors():
    rl, rs, dl, img = _cpu_inputs()
    with torch.no_grad():
        with pytest.raises(C.PlaneDepthHipError, match="GPU only"):
            ops.render_views(rl, rs, None, dl, img, (1.0,))
        with pytest.raises(C.PlaneDepthHipError, match="GPU only"):
            ops.render_views(rl, None, None, dl, img, (1.0, -1.0), use_mixture_loss=False, tail_applied=True)
        with pytest.raises(C.PlaneDepthHipError, match="GPU only"):
            planedepth_amd.predict.render(lambda x, grids: {}, img, (1.0,))
        with pytest.raises(C.PlaneDepthHipError, match="GPU only"):   # the new keyword reaches the same device check
            DT.fused_decoder_tail_inference({"disp_layered": dl}, rl, rs, all_ones_mask=True, keep_conv_outputs=True)


def test_operator_refuses_inputs_that_require_grad():
    rl, rs, dl, img = _cpu_inputs()
    for which in range(4):
        args = [t.clone().requires_grad_(i == which) for i, t in enumerate((rl, rs, dl, img))]
        with pytest.raises(ValueError, match=r"requires grad, but render_views is forward-only.*ops\.plane_sweep_disp,"):
            ops.render_views(args[0], args[1], None, args[2], args[3], (1.0,))
    with torch.no_grad():   # under no_grad the same tensors get as far as the device check
        with pytest.raises(C.PlaneDepthHipError, match="GPU only"):
            ops.render_views(rl.clone().requires_grad_(True), rs, None, dl, img, (1.0,))


def test_operator_checks_its_arguments_before_the_device():
    rl, rs, dl, img = _cpu_inputs()
    B, N, H, W = rl.shape
    with torch.no_grad():
        with pytest.raises(ValueError, match="want"):
            ops.render_views(rl, rs, None, dl, img, (1.0,), want=("depth",))
        with pytest.raises(ValueError, match="empty"):
            ops.render_views(rl, rs, None, dl, img, ())
        with pytest.raises(ValueError, match=r"baselines\[1\].*finite"):
            ops.render_views(rl, rs, None, dl, img, (1.0, float("nan")))
        with pytest.raises(TypeError, match="float32 or torch.bfloat16"):
            ops.render_views(rl.half(), rs.half(), None, dl, img, (1.0,))
        with pytest.raises(TypeError, match="one dtype"):
            ops.render_views(rl.bfloat16(), rs, None, dl, img, (1.0,))
        dense = dl * (1.0 + torch.rand(B, N, H, W))
        with pytest.raises(C.PlaneDepthHipError, match="disp_layered is a dense.*PD_TAIL_DISP_DENSE"):
            ops.render_views(rl, rs, None, dense, img, (1.0,))
        with pytest.raises(C.PlaneDepthHipError, match="padding_mask is a dense"):
            ops.render_views(rl, rs, torch.ones(B, N, H, W), dl, img, (1.0,))
