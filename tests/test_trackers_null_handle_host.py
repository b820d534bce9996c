"""The sentence every option entry of the sequence handles answers a NULL handle with (vors_trackers_* and vors_tracker_*: the depth
filter, the keyframe map and everything on it), pinned byte for byte: VORS_ERR_INVALID_ARGUMENT and vors_last_error. No device is
opened: each entry refuses before it touches one. Every other argument is NULL or zero."""
import ctypes as C

import pytest

import vors_amd as V

INVALID_ARGUMENT = -1   # VORS_ERR_INVALID_ARGUMENT (include/vors_hip.h)
HANDLE = "the handle t is NULL"
SENTENCES = {
    "vors_trackers_enable_depth_filter": "enable_depth_filter: " + HANDLE,
    "vors_trackers_keyframe_depth": "keyframe_depth: " + HANDLE,
    "vors_trackers_workspace_bytes": "NULL argument",
    "vors_trackers_enable_map": "enable_map: " + HANDLE,
    "vors_trackers_map": "map: " + HANDLE,
    "vors_trackers_enable_map_voxels": "enable_map_voxels: " + HANDLE,
    "vors_trackers_map_voxels": "map_voxels: " + HANDLE,
    "vors_trackers_enable_map_voxel_stats": "enable_map_voxel_stats: " + HANDLE,
    "vors_trackers_map_voxel_stats": "map_voxel_stats: " + HANDLE,
    "vors_trackers_map_voxel_means": "map_voxel_means: " + HANDLE,
    "vors_trackers_enable_map_normals": "enable_map_normals: " + HANDLE,
    "vors_trackers_map_normals": "map_normals: " + HANDLE,
    "vors_trackers_enable_map_icp": "enable_map_icp: " + HANDLE,
    "vors_trackers_map_icp": "map_icp: " + HANDLE,
    "vors_trackers_enable_map_icp_joint": "enable_map_icp_joint: " + HANDLE,
    "vors_trackers_map_icp_joint": "map_icp_joint: " + HANDLE,
    "vors_trackers_enable_map_icp_means": "enable_map_icp_means: " + HANDLE,
    "vors_trackers_map_icp_means": "map_icp_means: " + HANDLE,
    "vors_trackers_render_map": "render_map: " + HANDLE,
    "vors_trackers_icp_map": "icp_map: " + HANDLE,
    "vors_trackers_icp_map_robust": "icp_map: " + HANDLE,
    "vors_trackers_icp_map_joint": "icp_map: " + HANDLE,
    "vors_tracker_enable_depth_filter": "enable_depth_filter: " + HANDLE,
    "vors_tracker_enable_map": "enable_map: " + HANDLE,
    "vors_tracker_read_map": "read_map: " + HANDLE,
    "vors_tracker_enable_map_voxels": "enable_map_voxels: " + HANDLE,
    "vors_tracker_read_map_voxels": "read_map_voxels: " + HANDLE,
    "vors_tracker_enable_map_voxel_stats": "enable_map_voxel_stats: " + HANDLE,
    "vors_tracker_read_map_voxel_stats": "read_map_voxel_stats: " + HANDLE,
    "vors_tracker_map_voxel_means": "map_voxel_means: " + HANDLE,
    "vors_tracker_render_map": "render_map: " + HANDLE,
    "vors_tracker_enable_map_normals": "enable_map_normals: " + HANDLE,
    "vors_tracker_read_map_normals": "read_map_normals: " + HANDLE,
    "vors_tracker_enable_map_icp": "enable_map_icp: " + HANDLE,
    "vors_tracker_read_map_icp": "read_map_icp: " + HANDLE,
    "vors_tracker_enable_map_icp_joint": "enable_map_icp_joint: " + HANDLE,
    "vors_tracker_read_map_icp_joint": "read_map_icp_joint: " + HANDLE,
    "vors_tracker_enable_map_icp_means": "enable_map_icp_means: " + HANDLE,
    "vors_tracker_read_map_icp_means": "read_map_icp_means: " + HANDLE,
}
SCALARS = (C.c_int, C.c_uint32, C.c_size_t, C.c_float, C.c_double)


def test_the_table_names_every_option_entry():
    """Every exported enable / map / read / render / icp_map entry of the two handles is in the table (a new one must be added here)."""
    option = [s for s in V.EXPORTED_SYMBOLS
              if s.startswith(("vors_trackers_enable_", "vors_trackers_map", "vors_trackers_render_map", "vors_trackers_icp_map",
                               "vors_tracker_enable_", "vors_tracker_read_", "vors_tracker_map", "vors_tracker_render_map"))
              and s != "vors_trackers_enable_kernel_timing"]   # (not an option of the map or the filter: "NULL handle", with the state entries)
    assert sorted(option) == sorted(s for s in SENTENCES if s not in ("vors_trackers_keyframe_depth", "vors_trackers_workspace_bytes"))


@pytest.mark.parametrize("name", sorted(SENTENCES))
def test_null_handle_sentence(name):
    fn = getattr(V.lib(), name)
    args = [0 if a in SCALARS else None for a in fn.argtypes[1:]]
    assert fn(None, *args) == INVALID_ARGUMENT
    assert V.lib().vors_last_error() == SENTENCES[name].encode()
