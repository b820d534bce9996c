"""Argument plumbing of the trackers' keyframe map that needs no device: the map tuple of Tracker / Trackers.enable_map, the exported
symbols, the NULL-handle refusals and the size of the segment record."""
import ctypes

import numpy as np
import pytest

import vors_amd as V

NEW = ("vors_trackers_enable_map", "vors_trackers_map", "vors_tracker_enable_map", "vors_tracker_read_map")


def test_map_tuple_defaults_and_shapes():
    f = V._map_args
    assert f(None) is None
    assert f((0, 1000, 8)) == (0, 1000, 8, 0) and f([1, 1000, 8, 3]) == (1, 1000, 8, 3)
    t = f((np.int64(0), np.int32(5), 2, np.uint8(9)))
    assert t == (0, 5, 2, 9) and all(type(v) is int for v in t)
    assert f((-1, 0, 0, 256)) == (-1, 0, 0, 256)   # values are judged by the library, once for every caller
    for bad in ((), (0,), (0, 1000), (0, 1000, 8, 0, 1), "abc", (0, 1000.0, 8), (0, 1000, None), (0, 1000, 8, True), (0, 2 ** 31, 8), 5, object()):
        with pytest.raises(V.VorsError, match="map"):
            f(bad)


def test_a_bad_tuple_is_refused_before_any_handle_is_created():
    img, depth = np.zeros((60, 80), np.uint8), np.zeros((60, 80), np.uint16)
    with pytest.raises(V.VorsError, match="map"):
        V.Tracker(V.Config(nb_levels=3), 0.0, depth, 0.0, img, map=(0, 1000))
    with pytest.raises(V.VorsError, match="map"):
        V.Tracker(V.Config(nb_levels=3), 0.0, depth, 0.0, img, map=(0, 1000, 8, 2.0))


def test_symbols_exported_and_null_handles_refused():
    lib = V.lib()
    for name in NEW:
        assert hasattr(lib, name) and name in V.EXPORTED_SYMBOLS
    assert lib.vors_trackers_enable_map(None, 0, 100, 4, 0) == -1 and b"NULL" in lib.vors_last_error()
    assert lib.vors_trackers_map(None, None, None, None, None, None, None) == -1 and b"NULL" in lib.vors_last_error()
    assert lib.vors_tracker_enable_map(None, 0, 100, 4, 0) == -1 and b"NULL" in lib.vors_last_error()
    assert lib.vors_tracker_read_map(None, 0, None, None, None, None, 0, None, None) == -1 and b"NULL" in lib.vors_last_error()


def test_segment_record_is_40_bytes():
    assert ctypes.sizeof(V.vors_map_segment) == 40 and V.MAP_SEGMENT_DTYPE.itemsize == 40
    assert [(n, V.MAP_SEGMENT_DTYPE.fields[n][1]) for n in V.MAP_SEGMENT_DTYPE.names] == [
        (n, getattr(V.vors_map_segment, n).offset) for n, _ in V.vors_map_segment._fields_]
    raw = np.arange(2 * 3 * 40, dtype=np.uint8).reshape(2, 3, 40)
    seg = V.decode_map_segments(raw)
    assert seg.shape == (2, 3) and seg[1, 2]["frame"] == int(raw[1, 2, :4].view("<i4")[0])
