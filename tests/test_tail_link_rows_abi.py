"""CPU checks of the row-form tail link's C ABI (pd_sweep_bwd_tail_rows_fuses / pd_plane_sweep_bwd_tail_rows): the header, the
ctypes table and the library agree, the query names the served set, pd_sweep_bwd_tail_fuses keeps its answers, and every
refusal happens in argument validation — nothing launches, so none of this needs a GPU."""
import ctypes
import itertools

import pytest

import capi_header
from planedepth_amd import _capi as C

ROW_FORMS = (0, C.PD_DISP_ROWS, C.PD_MASK_ROWS, C.PD_DISP_ROWS | C.PD_MASK_ROWS)
NULL_ROWS = [None] * 21


def desc(B=8, N=49, H=192, W=640, mode=C.PD_WARP_DISP, flags=C.PD_MIXTURE, sign=1.0, impl=C.PD_IMPL_AUTO):
    return C.SweepDesc(B, N, H, W, mode, flags, sign, impl)


def rows_fuses(d):
    return C.load().pd_sweep_bwd_tail_rows_fuses(ctypes.byref(d))


def test_header_capi_and_library_agree():
    assert capi_header.prototype("pd_sweep_bwd_tail_rows_fuses") == ("int", ["const pd_sweep_desc* d"])
    args, old_args = capi_header.params("pd_plane_sweep_bwd_tail_rows"), capi_header.params("pd_plane_sweep_bwd_tail")
    assert len(args) == len(old_args) + 1 == 22                      # the existing argument list + mask_rows
    assert [a for a in args if a != "const float* mask_rows"] == old_args
    assert C.SIGNATURES["pd_sweep_bwd_tail_rows_fuses"] == (ctypes.c_int, [ctypes.POINTER(C.SweepDesc)])
    assert C.SIGNATURES["pd_plane_sweep_bwd_tail_rows"] == (ctypes.c_int, [ctypes.POINTER(C.SweepDesc)] + [ctypes.c_void_p] * 21)
    assert C.SIGNATURES["pd_plane_sweep_bwd_tail"] == (ctypes.c_int, [ctypes.POINTER(C.SweepDesc)] + [ctypes.c_void_p] * 20)
    lib = C.load()
    assert hasattr(lib, "pd_sweep_bwd_tail_rows_fuses") and hasattr(lib, "pd_plane_sweep_bwd_tail_rows")


@pytest.mark.parametrize("N", [49, 63])
def test_served_set_at_the_headline_shape(N):
    for form, automask, sign in itertools.product(ROW_FORMS, (0, C.PD_AUTOMASK), (1.0, -1.0)):
        assert rows_fuses(desc(N=N, flags=C.PD_MIXTURE | form | automask, sign=sign)) == 1, (form, automask, sign)


def test_outside_the_served_set():
    for form in ROW_FORMS:
        assert rows_fuses(desc(flags=form)) == 0                                              # no mixture
        assert rows_fuses(desc(flags=C.PD_MIXTURE | C.PD_RENDER_PROB | form)) == 0
        assert rows_fuses(desc(flags=C.PD_MIXTURE | C.PD_LOGITS_BF16 | form)) == 0
        assert rows_fuses(desc(flags=C.PD_MIXTURE | form, sign=0.5)) == 0
        assert rows_fuses(desc(flags=C.PD_MIXTURE | form, sign=0.0)) == 0
        assert rows_fuses(desc(flags=C.PD_MIXTURE | form, W=641)) == 0                        # odd width
        assert rows_fuses(desc(flags=C.PD_MIXTURE | form, W=3000)) == 0                       # the row does not fit the LDS
        assert rows_fuses(desc(flags=C.PD_MIXTURE | form, impl=C.PD_IMPL_GENERAL)) == 0
        assert rows_fuses(desc(flags=C.PD_MIXTURE | form, impl=C.PD_IMPL_ROWS1)) == 0
    assert rows_fuses(desc(flags=C.PD_MIXTURE | C.PD_DISP_DENSE)) == 0
    assert rows_fuses(desc(flags=C.PD_MIXTURE | C.PD_DISP_DENSE | C.PD_MASK_ROWS)) == 0
    assert rows_fuses(desc(mode=C.PD_WARP_HOMOGRAPHY)) == 0
    assert rows_fuses(desc(mode=C.PD_WARP_HOMOGRAPHY, flags=C.PD_MIXTURE | C.PD_HOMO_UNIFORM)) == 0
    assert C.load().pd_sweep_bwd_tail_rows_fuses(None) == 0


def test_the_per_plane_query_keeps_its_answers():
    lib = C.load()
    for automask, sign in itertools.product((0, C.PD_AUTOMASK), (1.0, -1.0)):
        assert lib.pd_sweep_bwd_tail_fuses(ctypes.byref(desc(flags=C.PD_MIXTURE | automask, sign=sign))) == 1
        for form in ROW_FORMS[1:]:
            assert lib.pd_sweep_bwd_tail_fuses(ctypes.byref(desc(flags=C.PD_MIXTURE | automask | form, sign=sign))) == 0


def test_refusals_happen_in_validation():
    lib = C.load()
    for form in ROW_FORMS:
        d = desc(flags=C.PD_MIXTURE | C.PD_LOGITS_BF16 | form)
        assert lib.pd_plane_sweep_bwd_tail_rows(ctypes.byref(d), *NULL_ROWS) == 2             # PD_ERR_UNSUPPORTED
        assert b"PD_LOGITS_BF16" in lib.pd_last_error() and b"pd_plane_sweep_bwd_tail_rows" in lib.pd_last_error()
        d = desc(flags=C.PD_MIXTURE | form)
        assert lib.pd_plane_sweep_bwd_tail_rows(ctypes.byref(d), *NULL_ROWS) == 1             # PD_ERR_ARG: NULL tensors
        assert b"NULL" in lib.pd_last_error()
    assert lib.pd_plane_sweep_bwd_tail_rows(None, *NULL_ROWS) == 1
    # a mask without PD_MASK_ROWS would be a per-pixel mask: not a form this entry has (never dereferenced: refused first)
    args = list(NULL_ROWS)
    for i in (11, 12, 13):                    # raw_sigma, tail_stash, disp
        args[i] = ctypes.c_void_p(16)
    args[5] = ctypes.c_void_p(16)             # mask_rows
    assert lib.pd_plane_sweep_bwd_tail_rows(ctypes.byref(desc()), *args) == 1
    assert b"PD_MASK_ROWS" in lib.pd_last_error()
