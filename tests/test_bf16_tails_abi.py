"""CPU-side checks of PD_TAIL_BF16 at the boundary: the Python constant is the header's, and both decoder tails accept the
flag in their argument validation (which needs no GPU) while unknown bits are still refused."""
import capi_header
from planedepth_amd import _capi as C


def test_flag_constant_is_the_headers():
    enum = capi_header.enum("pd_tail_flags")
    assert len(enum) == 5 and all(k.startswith("PD_TAIL_") for k in enum)
    assert enum["PD_TAIL_BF16"] == C.PD_TAIL_BF16 == 4
    assert enum["PD_TAIL_MIXTURE"] == C.PD_TAIL_MIXTURE and enum["PD_TAIL_DISP_DENSE"] == C.PD_TAIL_DISP_DENSE
    bits = list(enum.values())
    assert len(set(bits)) == len(bits) and all(b & (b - 1) == 0 for b in bits)
    assert 64 not in bits   # tests/test_capi.py relies on 64 being unknown


def test_both_tails_accept_the_flag_and_still_validate():
    lib = C.load()
    flags = C.PD_TAIL_MIXTURE | C.PD_TAIL_BF16
    assert lib.pd_decoder_tail_fwd(1, 4, 8, 8, flags, *([None] * 10)) == 1
    assert b"NULL" in lib.pd_last_error() and b"flags" not in lib.pd_last_error()
    assert lib.pd_plade_tail_fwd(1, 4, 8, 8, flags, *([None] * 11)) == 1
    assert b"NULL" in lib.pd_last_error() and b"flags" not in lib.pd_last_error()
    # layers and bwd take it too: the refusal is the NULL tensors', not the flag's
    assert lib.pd_decoder_tail_layers(1, 4, 8, 8, flags, *([None] * 7)) == 1
    assert b"flags" not in lib.pd_last_error()
    assert lib.pd_decoder_tail_bwd(1, 4, 8, 8, flags, *([None] * 15)) == 1
    assert b"flags" not in lib.pd_last_error()
    assert lib.pd_plade_tail_layers(1, 4, 8, 8, flags, *([None] * 8)) == 1
    assert b"flags" not in lib.pd_last_error()
    assert lib.pd_plade_tail_bwd(1, 4, 8, 8, flags, *([None] * 16)) == 1
    assert b"flags" not in lib.pd_last_error()
    # shape checks are unchanged under the flag
    assert lib.pd_plade_tail_fwd(1, 1, 8, 8, flags, *([None] * 11)) == 1
    assert b"shape" in lib.pd_last_error()


def test_unknown_flag_bits_are_still_refused():
    lib = C.load()
    for flags in (64, 64 | C.PD_TAIL_BF16, 8):
        assert lib.pd_decoder_tail_fwd(1, 4, 8, 8, flags, *([None] * 10)) == 1
        assert b"flags" in lib.pd_last_error()
        assert lib.pd_plade_tail_fwd(1, 4, 8, 8, flags, *([None] * 11)) == 1
        assert b"flags" in lib.pd_last_error()
