"""The averaged map as the map ICP correction's model (vors_trackers_enable_map_icp_means, vors_trackers_map_icp_means,
vors_tracker_enable_map_icp_means, vors_tracker_read_map_icp_means): what needs no GPU. The four symbols and their ctypes
signatures, the refusal of a NULL handle by each (checked before any HIP call, so it is answered on a machine without a device), the
record's size and its decoder, and the argument checks of the Python layer."""
import ctypes as C

import numpy as np
import pytest

import vors_amd as V

ENTRIES = {
    "vors_trackers_enable_map_icp_means": ([C.c_void_p, C.c_uint32, C.c_uint32], "enable_map_icp_means"),
    "vors_trackers_map_icp_means": ([C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)], "map_icp_means"),
    "vors_tracker_enable_map_icp_means": ([C.c_void_p, C.c_uint32, C.c_uint32], "enable_map_icp_means"),
    "vors_tracker_read_map_icp_means": ([C.c_void_p, C.c_void_p], "read_map_icp_means"),
}


def test_symbols_and_signatures():
    lib = V.lib()
    for name, (argtypes, _) in ENTRIES.items():
        assert name in V.EXPORTED_SYMBOLS and hasattr(lib, name), name
        assert list(getattr(lib, name).argtypes) == argtypes, name


def test_null_handle_is_refused_by_name():
    lib = V.lib()
    for name, (argtypes, who) in ENTRIES.items():
        args = [None] + [2 if a is C.c_uint32 else None for a in argtypes[1:]]
        assert getattr(lib, name)(*args) == -1, name   # VORS_ERR_INVALID_ARGUMENT
        assert lib.vors_last_error() == f"{who}: the handle t is NULL".encode(), name


def test_record_size_and_decoder():
    assert C.sizeof(V.vors_map_icp_means_record) == 8 and V.MAP_ICP_MEANS_RECORD_DTYPE.itemsize == 8
    assert V.MAP_ICP_MEANS_RECORD_DTYPE.names == ("resolved", "kept")
    rec = V.vors_map_icp_means_record(resolved=70000, kept=0xFFFFFFFE)
    raw = np.frombuffer(bytes(rec), np.uint8).reshape(1, 8)
    out = V.decode_map_icp_means_records(raw)
    assert out.shape == (1,) and out[0]["resolved"] == 70000 and out[0]["kept"] == 0xFFFFFFFE
    assert out.tobytes() == bytes(rec)
    two = V.decode_map_icp_means_records(np.arange(16, dtype=np.uint8).reshape(2, 8))
    assert two["resolved"].tolist() == [0x03020100, 0x0B0A0908] and two["kept"].tolist() == [0x07060504, 0x0F0E0D0C]


def test_python_argument_checks():
    assert V._map_icp_means_args(None) is None
    assert V._map_icp_means_args(2) == (2, 0) and V._map_icp_means_args((2, 1)) == (2, 1) and V._map_icp_means_args([3]) == (3, 0)
    for bad in ((), (1, 2, 3)):
        with pytest.raises(V.VorsError, match="map_icp_means"):
            V._map_icp_means_args(bad)
    with pytest.raises(V.VorsError, match="min_count must be in 0..2\\^32 - 1"):
        V._map_icp_means_args((-1, 0))
    with pytest.raises(V.VorsError, match="min_span must be in 0..2\\^32 - 1"):
        V._map_icp_means_args((1, 1 << 32))
