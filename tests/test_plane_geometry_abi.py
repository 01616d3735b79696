"""CPU checks of the row-form boundary: the header, the built library and the ctypes table agree on pd_plane_geometry_fwd / _bwd and
on PD_TAIL_DISP_ROWS / PD_TAIL_MASK_ROWS, every refusal happens in argument validation (nothing launches, no GPU needed), and the
Python operators exist and refuse CPU tensors."""
import ctypes

import pytest
import torch

import capi_header
from planedepth_amd import _capi as C
from planedepth_amd import decoder_tail, ops

GEOM = dict(no_levels=4, xz_levels=3, disp_min=2.0, disp_max=300.0, xz_min=0.1852, xz_max=0.3704)
P = ctypes.c_void_p(16)   # a non-NULL pointer that is never dereferenced: every call below is refused in validation


def test_header_capi_and_library_agree():
    for name, value in (("PD_TAIL_DISP_ROWS", 8), ("PD_TAIL_MASK_ROWS", 16)):
        assert capi_header.constant(name) == getattr(C, name) == value
    lib = C.load()
    for name in ("pd_plane_geometry_fwd", "pd_plane_geometry_bwd"):
        res, args = C.SIGNATURES[name]
        assert res is ctypes.c_int
        assert capi_header.kinds(name) == capi_header.ctypes_kinds(args) == list("IIIIIIFFFFPPPPPPP"), name
        assert hasattr(lib, name)


def geom_fwd(lib, B=1, nl=4, nx=3, H=8, W=8, flags=0, ptrs=None):
    return lib.pd_plane_geometry_fwd(B, nl, nx, H, W, flags, 2.0, 300.0, 0.1852, 0.3704, *(ptrs or [None] * 7))


def geom_bwd(lib, B=1, nl=4, nx=3, H=8, W=8, flags=0, ptrs=None):
    return lib.pd_plane_geometry_bwd(B, nl, nx, H, W, flags, 2.0, 300.0, 0.1852, 0.3704, *(ptrs or [None] * 7))


def test_geometry_refusals_have_text():
    lib = C.load()
    for call in (geom_fwd, geom_bwd):
        assert call(lib, nx=1) == 1 and b"xz_levels" in lib.pd_last_error()
        assert call(lib, nl=1) == 1 and b"no_levels" in lib.pd_last_error()
        assert call(lib, flags=1) == 1 and b"flags" in lib.pd_last_error()
        assert call(lib, H=0) == 1 and b"shape" in lib.pd_last_error()
        assert call(lib) == 1 and b"NULL" in lib.pd_last_error()
        assert call(lib, nx=0) == 1 and b"NULL" in lib.pd_last_error()      # xz_levels == 0 is legal: it gets to the pointers
    # bwd needs the residual (there is nothing to differentiate without one) and an upstream gradient
    assert geom_bwd(lib, ptrs=[None, P, P, P, P, P, None]) == 1 and b"NULL" in lib.pd_last_error()
    assert geom_bwd(lib, ptrs=[P, P, P, None, None, P, None]) == 1 and b"gradient" in lib.pd_last_error()


def test_tail_entry_points_take_the_row_flags_and_refuse_rows_with_dense():
    lib = C.load()
    rows = C.PD_TAIL_DISP_ROWS | C.PD_TAIL_MASK_ROWS
    for extra in (0, C.PD_TAIL_BF16, C.PD_TAIL_MIXTURE):
        for flags in (C.PD_TAIL_DISP_ROWS, C.PD_TAIL_MASK_ROWS, rows):
            assert lib.pd_decoder_tail_fwd(1, 4, 8, 8, flags | extra, *([None] * 10)) == 1
            assert b"NULL" in lib.pd_last_error() and b"unknown flags" not in lib.pd_last_error()
            assert lib.pd_decoder_tail_layers(1, 4, 8, 8, flags | extra, *([None] * 7)) == 1
            assert b"unknown flags" not in lib.pd_last_error()
            assert lib.pd_decoder_tail_bwd(1, 4, 8, 8, flags | extra, *([None] * 15)) == 1
            assert b"unknown flags" not in lib.pd_last_error()
        bad = C.PD_TAIL_DISP_ROWS | C.PD_TAIL_DISP_DENSE | extra
        assert lib.pd_decoder_tail_fwd(1, 4, 8, 8, bad, *([P] * 9 + [None])) == 1
        assert b"PD_TAIL_DISP_ROWS" in lib.pd_last_error() and b"PD_TAIL_DISP_DENSE" in lib.pd_last_error()
        assert lib.pd_decoder_tail_layers(1, 4, 8, 8, bad, *([P] * 6 + [None])) == 1
        assert b"PD_TAIL_DISP_ROWS" in lib.pd_last_error()
        assert lib.pd_decoder_tail_bwd(1, 4, 8, 8, bad, *([P] * 14 + [None])) == 1
        assert b"PD_TAIL_DISP_ROWS" in lib.pd_last_error()
    # a row mask that is not there
    args = [P] * 9 + [None]
    args[2] = None
    assert lib.pd_decoder_tail_fwd(1, 4, 8, 8, C.PD_TAIL_MASK_ROWS, *args) == 1
    assert b"PD_TAIL_MASK_ROWS" in lib.pd_last_error()
    # the PladeNet tail has no row form
    assert lib.pd_plade_tail_fwd(1, 4, 8, 8, C.PD_TAIL_DISP_ROWS, *([None] * 11)) == 1 and b"flags" in lib.pd_last_error()
    # the workspace query stays the per-plane form's need: the maximum over the forms
    assert lib.pd_decoder_tail_bwd_workspace_floats(2, 63, 192, 640) == 2 * 480 * 63


def test_operators_exist_and_refuse_cpu_tensors_and_wrong_shapes():
    B, H, W = 1, 4, 6
    grid = torch.zeros(B, 2, H, W)
    with pytest.raises(C.PlaneDepthHipError):
        ops.plane_geometry(grid, None, **GEOM)
    with pytest.raises(C.PlaneDepthHipError):
        decoder_tail.fused_plane_geometry({}, grid, None, **GEOM)
    with pytest.raises(TypeError):
        ops.plane_geometry(None, None, **GEOM)
    # the row view: reference shape, nothing W-sized behind it; a foreign consumer's dense gradient is summed over x, one that is
    # itself constant along x comes back without W times the elements (CPU tensors: this is autograd plumbing, no kernel)
    rows = torch.rand(2, 3, 5).requires_grad_(True)
    view = ops.row_view(rows, 7)
    assert tuple(view.shape) == (2, 3, 5, 7) and view.stride(3) == 0 and view.data_ptr() == rows.data_ptr()
    assert ops._row_view(view, 2, 3, 5, 7) and ops._row_view(view[:1], 1, 3, 5, 7) and ops._rows_of(view) is rows
    assert not ops._row_view(torch.rand(2, 3, 1, 1).expand(2, 3, 5, 7), 2, 3, 5, 7)      # per-plane scalars are not a row view
    assert not ops._row_view(torch.rand(2, 3, 5, 7), 2, 3, 5, 7)
    with pytest.raises(ValueError):
        ops._row_view(view, 2, 3, 5, 8)
    weight = torch.rand(2, 3, 5, 7)
    (view * weight).sum().backward()
    assert torch.allclose(rows.grad, weight.sum(-1))
    rows.grad = None
    g_rows = torch.rand(2, 3, 5)
    ops._FirstColumn.apply(view).backward(g_rows)          # hands g / W on every column, as a stride-0 gradient
    assert torch.allclose(rows.grad, g_rows, rtol=1e-6)
