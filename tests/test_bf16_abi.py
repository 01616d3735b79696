"""CPU checks of the bf16 storage contract (PD_LOGITS_BF16): the header, the ctypes table and the library agree on the flag and
on pd_sweep_native_bf16, the query names the native set, and every refusal happens in argument validation — nothing
launches, so none of this needs a GPU."""
import ctypes

import capi_header
from planedepth_amd import _capi as C

NULL_FWD = [None] * 14
NULL_BWD = [None] * 20


def desc(B=8, N=49, H=192, W=640, mode=C.PD_WARP_DISP, flags=C.PD_MIXTURE, impl=C.PD_IMPL_AUTO):
    return C.SweepDesc(B, N, H, W, mode, flags, 1.0, impl)


def native(d):
    return C.load().pd_sweep_native_bf16(ctypes.byref(d))


def test_header_capi_and_library_agree_on_the_flag_and_query():
    assert capi_header.constant("PD_LOGITS_BF16") == C.PD_LOGITS_BF16 == 2048
    assert capi_header.prototype("pd_sweep_native_bf16") == ("int", ["const pd_sweep_desc* d"])
    assert C.SIGNATURES["pd_sweep_native_bf16"] == (ctypes.c_int, [ctypes.POINTER(C.SweepDesc)])
    assert hasattr(C.load(), "pd_sweep_native_bf16")
    assert ctypes.sizeof(C.SweepDesc) == 32


def test_native_set():
    mix_am = C.PD_MIXTURE | C.PD_AUTOMASK
    rows = C.PD_DISP_ROWS | C.PD_MASK_ROWS
    assert native(desc())                                              # BASELINE configs[1]
    assert native(desc(N=63, flags=mix_am | rows))                     # N = 63, xz rows + automask
    assert native(desc(flags=rows | C.PD_MIXTURE))                     # per-row shifts (the stereo view of homography_warp)
    assert native(desc(flags=C.PD_DISP_ROWS))                          # L1, per-row disparities, no mask
    assert native(desc(flags=0))                                       # L1
    assert native(desc(flags=C.PD_AUTOMASK))                           # L1 + automask
    assert native(desc(flags=mix_am))
    assert native(desc(impl=C.PD_IMPL_FAST_ROWS)) and native(desc(impl=C.PD_IMPL_EXACT_ROWS))
    assert native(desc(B=2, N=9, H=384, W=1280))                       # HR
    assert native(desc(flags=C.PD_MIXTURE | C.PD_LOGITS_BF16))         # (the flag itself may be set)


def test_outside_the_native_set():
    assert not native(desc(mode=C.PD_WARP_HOMOGRAPHY))
    assert not native(desc(mode=C.PD_WARP_HOMOGRAPHY, flags=C.PD_MIXTURE | C.PD_HOMO_UNIFORM))
    assert not native(desc(flags=C.PD_MIXTURE | C.PD_DISP_DENSE))
    assert not native(desc(flags=C.PD_MIXTURE | C.PD_RENDER_PROB))
    assert not native(desc(impl=C.PD_IMPL_GENERAL)) and not native(desc(impl=C.PD_IMPL_ROWS1))
    assert not native(desc(W=257))                                     # odd width
    assert not native(desc(W=3000))                                    # the row does not fit the LDS
    assert C.load().pd_sweep_native_bf16(None) == 0


def test_refusals_name_the_flag_and_launch_nothing():
    lib = C.load()
    for d in (desc(mode=C.PD_WARP_HOMOGRAPHY), desc(flags=C.PD_MIXTURE | C.PD_DISP_DENSE), desc(W=257),
              desc(impl=C.PD_IMPL_GENERAL), desc(flags=C.PD_MIXTURE | C.PD_RENDER_PROB)):
        d.flags |= C.PD_LOGITS_BF16
        assert lib.pd_plane_sweep_fwd(ctypes.byref(d), *NULL_FWD) == 2, (d.mode, d.flags, d.W)   # PD_ERR_UNSUPPORTED
        assert b"PD_LOGITS_BF16" in lib.pd_last_error()
        assert lib.pd_plane_sweep_bwd(ctypes.byref(d), *NULL_BWD) == 2
        assert b"PD_LOGITS_BF16" in lib.pd_last_error()
    for extra in (C.PD_BWD_ACCUMULATE, C.PD_BWD_DEFER_GATHER):
        d = desc(flags=C.PD_MIXTURE | C.PD_LOGITS_BF16 | extra)
        assert lib.pd_plane_sweep_bwd(ctypes.byref(d), *NULL_BWD) == 2
        assert b"PD_LOGITS_BF16" in lib.pd_last_error()


def test_native_descriptor_reaches_the_pointer_checks():
    lib = C.load()
    d = desc(flags=C.PD_MIXTURE | C.PD_LOGITS_BF16)
    assert lib.pd_plane_sweep_fwd(ctypes.byref(d), *NULL_FWD) == 1   # PD_ERR_ARG: NULL tensors
    assert b"NULL" in lib.pd_last_error()
    assert lib.pd_plane_sweep_bwd(ctypes.byref(d), *NULL_BWD) == 1


def test_per_pixel_mask_is_refused():
    lib = C.load()
    d = desc(flags=C.PD_MIXTURE | C.PD_LOGITS_BF16)
    args = list(NULL_FWD)
    args[7] = ctypes.c_void_p(16)   # padding_mask (never dereferenced: refused in validation)
    assert lib.pd_plane_sweep_fwd(ctypes.byref(d), *args) == 2
    assert b"PD_LOGITS_BF16" in lib.pd_last_error()


def test_pair_and_tail_entry_points_refuse_the_flag():
    lib = C.load()
    d = desc(flags=C.PD_MIXTURE | C.PD_LOGITS_BF16)
    assert lib.pd_plane_sweep_bwd_tail(ctypes.byref(d), *([None] * 20)) == 2
    assert b"PD_LOGITS_BF16" in lib.pd_last_error()
    u = desc(mode=C.PD_WARP_HOMOGRAPHY, flags=C.PD_MIXTURE | C.PD_HOMO_UNIFORM | C.PD_LOGITS_BF16)
    v = C.SweepView()
    assert lib.pd_uniform_fwd_pair(ctypes.byref(u), None, None, None, ctypes.byref(v), ctypes.byref(v), None) == 2
    assert b"PD_LOGITS_BF16" in lib.pd_last_error()
    assert lib.pd_uniform_bwd_pair(ctypes.byref(u), None, None, None, ctypes.byref(v), ctypes.byref(v), None, None, None) == 2
    assert b"PD_LOGITS_BF16" in lib.pd_last_error()
    u.flags |= C.PD_BWD_DEFER_GATHER
    assert lib.pd_uniform_gather_pair(ctypes.byref(u), *([None] * 9)) == 2
    assert b"PD_LOGITS_BF16" in lib.pd_last_error()


def test_sizes_of_unflagged_descriptors_do_not_change():
    lib = C.load()
    d = desc(B=2)
    assert lib.pd_sweep_stash_floats(ctypes.byref(d)) == (4 + 2) * 192 * 640
    assert lib.pd_sweep_bwd_workspace_floats(ctypes.byref(d)) == 2 * 192 * 49 * (1 + 4 * 10)
    d.flags |= C.PD_LOGITS_BF16
    assert lib.pd_sweep_stash_floats(ctypes.byref(d)) == (4 + 2) * 192 * 640
