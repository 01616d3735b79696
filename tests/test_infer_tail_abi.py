"""CPU checks of the inference tails' C ABI (pd_decoder_tail_infer / pd_plade_tail_infer) and of the Python layers above it: the
header, the ctypes table and the library agree; every refusal happens in argument validation, with text — nothing launches, so
none of this needs a GPU; the operators and ``predict`` refuse CPU tensors and, with gradients enabled, inputs that require grad."""
import ctypes

import pytest
import torch

import capi_header
import planedepth_amd
from planedepth_amd import _capi as C
from planedepth_amd import decoder_tail as DT
from planedepth_amd import ops

P = ctypes.c_void_p
PTR = P(256)   # never dereferenced: every call below is refused before a launch


def _decoder(B=2, N=5, H=8, W=16, flags=C.PD_TAIL_MIXTURE, raw_logits=PTR, raw_sigma=PTR, mask=None, dl=PTR, disp=PTR):
    lib = C.load()
    rc = lib.pd_decoder_tail_infer(B, N, H, W, flags, raw_logits, raw_sigma, mask, dl, disp, None, None, None, None, None, None)
    return rc, lib.pd_last_error()


def _plade(B=2, N=5, H=8, W=16, flags=C.PD_TAIL_MIXTURE, raw_logits=PTR, raw_sigma=PTR, dl=PTR, ray=PTR, disp=PTR):
    lib = C.load()
    rc = lib.pd_plade_tail_infer(B, N, H, W, flags, raw_logits, raw_sigma, dl, ray, disp, None, None, None, None, None, None)
    return rc, lib.pd_last_error()


def test_header_capi_and_library_agree():
    lib = C.load()
    for name, fwd, inputs in (("pd_decoder_tail_infer", "pd_decoder_tail_fwd", 4), ("pd_plade_tail_infer", "pd_plade_tail_fwd", 4)):
        args, fwd_args = capi_header.params(name), capi_header.params(fwd)
        assert args[:5 + inputs] == fwd_args[:5 + inputs]          # B, N, H, W, flags and the forward's input tensors
        assert args[5 + inputs:] == ["float* disp", "float* depth", "float* confidence", "int* plane_index", "float* disp_best",
                                     "float* stash", "pd_stream_t stream"]
        assert C.SIGNATURES[name] == (ctypes.c_int, [ctypes.c_int] * 5 + [P] * (len(args) - 5))
        assert hasattr(lib, name)


def test_decoder_entry_refuses_in_validation():
    rc, msg = _decoder(disp=None)
    assert rc == 1 and b"disp" in msg and b"NULL" in msg
    for bad in (dict(B=0), dict(N=0), dict(H=0), dict(W=-1), dict(B=65536)):
        rc, msg = _decoder(**bad)
        assert rc == 1 and b"shape" in msg, bad
    rc, msg = _decoder(flags=C.PD_TAIL_MIXTURE | 32)
    assert rc == 1 and b"flags" in msg
    rc, msg = _decoder(flags=C.PD_TAIL_DISP_DENSE | C.PD_TAIL_DISP_ROWS)
    assert rc == 1 and b"PD_TAIL_DISP_ROWS" in msg and b"PD_TAIL_DISP_DENSE" in msg
    rc, msg = _decoder(flags=C.PD_TAIL_MASK_ROWS, mask=None)
    assert rc == 1 and b"PD_TAIL_MASK_ROWS" in msg and b"padding_mask" in msg
    rc, msg = _decoder(raw_logits=None)
    assert rc == 1 and b"NULL" in msg
    rc, msg = _decoder(dl=None, flags=C.PD_TAIL_DISP_ROWS)
    assert rc == 1 and b"PD_TAIL_DISP_ROWS" in msg
    rc, msg = _decoder(raw_sigma=None)
    assert rc == 1 and b"raw_sigma" in msg


def test_plade_entry_refuses_in_validation():
    rc, msg = _plade(disp=None)
    assert rc == 1 and b"disp" in msg and b"NULL" in msg
    for flag in (C.PD_TAIL_DISP_ROWS, C.PD_TAIL_MASK_ROWS):
        rc, msg = _plade(flags=C.PD_TAIL_MIXTURE | flag)
        assert rc == 1 and b"row form" in msg and b"flags" in msg
    rc, msg = _plade(N=1)
    assert rc == 1 and b"N >= 2" in msg
    rc, msg = _plade(H=0)
    assert rc == 1 and b"shape" in msg
    rc, msg = _plade(flags=64)
    assert rc == 1 and b"flags" in msg
    rc, msg = _plade(ray=None)
    assert rc == 1 and b"NULL" in msg
    rc, msg = _plade(raw_sigma=None)
    assert rc == 1 and b"raw_sigma" in msg


def _cpu_inputs(B=1, N=3, H=2, W=4):
    g = torch.Generator().manual_seed(3)
    rl, rs = torch.randn(B, N, H, W, generator=g), torch.randn(B, N, H, W, generator=g)
    dl = (torch.arange(N, dtype=torch.float32) + 1.0).view(1, N, 1, 1).expand(B, N, H, W)
    return rl, rs, dl


def test_operators_refuse_cpu_tensors():
    rl, rs, dl = _cpu_inputs()
    with torch.no_grad():
        with pytest.raises(C.PlaneDepthHipError, match="GPU only"):
            ops.decoder_tail_inference(rl, rs, None, dl)
        with pytest.raises(C.PlaneDepthHipError, match="GPU only"):
            ops.plade_tail_inference(rl[:, :-1], rs, dl, ray_norm=torch.ones(2, 4))
        with pytest.raises(C.PlaneDepthHipError, match="GPU only"):
            DT.fused_decoder_tail_inference({"disp_layered": dl}, rl, rs, all_ones_mask=True)
        with pytest.raises(C.PlaneDepthHipError, match="GPU only"):
            DT.fused_plade_tail_inference({"disp_layered": dl}, rl[:, :-1], rs)
        with pytest.raises(C.PlaneDepthHipError, match="GPU only"):
            planedepth_amd.predict(lambda x, grids: {}, torch.zeros(1, 3, 4, 8))


def test_operators_refuse_inputs_that_require_grad():
    rl, rs, dl = _cpu_inputs()
    for which in range(3):
        args = [t.clone().requires_grad_(i == which) for i, t in enumerate((rl, rs, dl))]
        with pytest.raises(ValueError, match=r"forward-only.*ops\.decoder_tail,"):
            ops.decoder_tail_inference(args[0], args[1], None, args[2])
        with pytest.raises(ValueError, match=r"forward-only.*ops\.plade_tail,"):
            ops.plade_tail_inference(args[0][:, :-1], args[1], args[2], ray_norm=torch.ones(2, 4))
    with torch.no_grad():   # under no_grad the same tensors get as far as the device check
        with pytest.raises(C.PlaneDepthHipError, match="GPU only"):
            ops.decoder_tail_inference(rl.requires_grad_(True), rs, None, dl)


def test_dtype_rule_is_the_training_tails():
    rl, rs, dl = _cpu_inputs()
    with torch.no_grad():
        with pytest.raises(TypeError, match="float32 or torch.bfloat16"):
            ops.decoder_tail_inference(rl.half(), rs.half(), None, dl)
        with pytest.raises(TypeError, match="one dtype"):
            ops.decoder_tail_inference(rl.bfloat16(), rs, None, dl)
        with pytest.raises(TypeError, match="one dtype"):
            ops.plade_tail_inference(rl[:, :-1], rs.bfloat16(), dl)
        with pytest.raises(ValueError, match="want"):
            ops.decoder_tail_inference(rl, rs, None, dl, want=("sigma",))
