"""CPU: the speculative chain verification entry points exist — the two names eagle_utils.py:22 imports resolve from the shim, and the
C-ABI checks its argument struct before anything is launched (no compute calls)."""
import ctypes
import sys

from conftest import PKG


def test_both_names_resolve_from_the_shim():
    sys.path.insert(0, PKG)
    try:
        from flashinfer.sampling import chain_speculative_sampling_target_only, verify_chain_greedy
    finally:
        sys.path.remove(PKG)
    assert callable(verify_chain_greedy) and callable(chain_speculative_sampling_target_only)


def test_argument_struct_is_checked():
    from fluent_mi355._lib import lib
    from fluent_mi355.sampling import FlSpecVerifyArgs

    a = FlSpecVerifyArgs()
    a.struct_bytes = ctypes.sizeof(FlSpecVerifyArgs) - 8        # a caller built against another layout: refused, not read past its end
    assert lib.fl_spec_verify_sample(ctypes.byref(a), None) == 1 and b"struct_bytes" in lib.fl_last_error()
    a.struct_bytes = ctypes.sizeof(FlSpecVerifyArgs)            # the right layout with zeroed sizes: refused for the sizes
    for fn in (lib.fl_spec_verify_sample, lib.fl_spec_verify_greedy):
        assert fn(ctypes.byref(a), None) == 1 and b"struct_bytes" not in lib.fl_last_error() and b"bad sizes" in lib.fl_last_error()
