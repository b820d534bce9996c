"""Argument plumbing of the trackers' depth filter that needs no device: the depth_filter tuple of Tracker / Trackers.enable_depth_filter,
the exported symbols and the NULL-handle refusals."""
import numpy as np
import pytest

import vors_amd as V

NEW = ("vors_trackers_enable_depth_filter", "vors_trackers_keyframe_depth", "vors_trackers_workspace_bytes", "vors_tracker_enable_depth_filter")


def test_depth_filter_tuple_defaults_and_shapes():
    f = V._depth_filter_args
    assert f(None) is None
    assert f(0.05) == (0.05, 255, 0) and f((0.05,)) == (0.05, 255, 0)
    assert f((0.05, 9)) == (0.05, 9, 0) and f([0.05, 9, 2]) == (0.05, 9, 2)
    assert f((np.float32(0.5), np.int64(7), 1)) == (0.5, 7, 1)
    t = f((1, 2, 3))
    assert t == (1.0, 2, 3) and isinstance(t[0], float) and isinstance(t[1], int)
    assert f((-1.0, 0, 256)) == (-1.0, 0, 256)   # values are judged by the library, once for every caller
    for bad in ((), (0.05, 255, 0, 1), "abc", (0.05, 2.5), (0.05, 255, None), (0.05, True), ("x",), object()):
        with pytest.raises(V.VorsError, match="depth_filter"):
            f(bad)


def test_a_bad_tuple_is_refused_before_any_handle_is_created():
    img, depth = np.zeros((60, 80), np.uint8), np.zeros((60, 80), np.uint16)
    with pytest.raises(V.VorsError, match="depth_filter"):
        V.Tracker(V.Config(nb_levels=3), 0.0, depth, 0.0, img, depth_filter=(0.05, 1, 2, 3))


def test_symbols_exported_and_null_handles_refused():
    lib = V.lib()
    for name in NEW:
        assert hasattr(lib, name) and name in V.EXPORTED_SYMBOLS
    assert lib.vors_trackers_enable_depth_filter(None, 0.01, 255, 0) == -1 and b"NULL" in lib.vors_last_error()
    assert lib.vors_trackers_keyframe_depth(None, None, None) == -1 and b"NULL" in lib.vors_last_error()
    assert lib.vors_trackers_workspace_bytes(None, None) == -1
    assert lib.vors_tracker_enable_depth_filter(None, 0.01, 255, 0) == -1 and b"NULL" in lib.vors_last_error()
