"""The progressive-rendering entry points of include/xrt.h (xrt_progressive_*) are exported and refuse
a NULL context (no GPU needed).  Without the feature the library has none of the six symbols."""
import ctypes as C

from xraytracer_amd import abi

SYMBOLS = ("xrt_progressive_begin", "xrt_progressive_add", "xrt_progressive_frame", "xrt_progressive_frame_device",
           "xrt_progressive_query", "xrt_progressive_end")


def test_the_six_symbols_are_exported():
    lib = C.CDLL(abi.LIB_PATH)
    missing = [n for n in SYMBOLS if not hasattr(lib, n)]
    assert not missing, missing
    assert set(SYMBOLS) <= set(abi.SIGNATURES)


def test_a_null_context_is_refused():
    lib = abi.lib()
    p = abi.XrtRenderParams()
    st = abi.XrtStats()
    assert lib.xrt_progressive_begin(None, C.byref(p), 0) != 0
    assert lib.xrt_progressive_begin(None, None, abi.XRT_PROGRESSIVE_VARIANCE) != 0
    assert lib.xrt_progressive_add(None, 1, C.byref(st)) != 0
    assert lib.xrt_progressive_frame(None, None, None) != 0
    assert lib.xrt_progressive_frame_device(None, None, None, None) != 0
    assert lib.xrt_progressive_end(None) != 0
    s = abi.XrtProgressiveState()
    assert lib.xrt_progressive_query(None, C.byref(s)) != 0


def test_the_state_struct_has_the_header_layout():
    # four uint32 then one uint64: 24 bytes, path_slots at 16
    assert C.sizeof(abi.XrtProgressiveState) == 24
    assert abi.XrtProgressiveState.path_slots.offset == 16
