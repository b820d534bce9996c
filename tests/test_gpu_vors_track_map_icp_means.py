"""`vors_track --map FILE --map-voxel SIZE_M --map-normals ... --map-icp ... --map-icp-means MIN_COUNT[,MIN_SPAN]` end to end on the GPU:
the small synthetic TUM-format sequence of tests/test_gpu_vors_track_map_voxel_means.py through the CLI, its summary line on stderr, and
its trajectory against Tracker(map_icp_means=...) with the same settings, bit for bit (the printed poses are the same text). Malformed,
or without --map-voxel / --map-icp: the usage and status 2."""
import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import vors_amd as V
from oracle import oracle as O
from test_gpu_vors_track_map_voxel_means import SLOTS, _cli, _write_png

# --map-icp's defaults (host/vors_track.cpp) with DIST_M 0.05 and ITERS 6
CLI_ICP = dict(dist_m=0.05, iters=6, step_eps=1e-5, min_points=6, normal_gate=1, min_cos=0.9, huber_m=0.0, last_keyframes=0, min_match_ratio=0.3,
               max_rms=0.01, max_trans_m=0.05, max_rot_rad=0.05)


def test_cli_map_icp_means_summary_and_trajectory(tmp_path):
    rows, cols, n = 240, 320, 8
    intr = O.INTRINSICS_FR1
    os.makedirs(tmp_path / "depth")
    os.makedirs(tmp_path / "rgb")
    step = 4 * np.array([0.010, -0.004, 0.003, 0.0015, -0.002, 0.001])
    frames, lines = [], []
    for k in range(n):
        g, d = O.synth_frame(4242, step * k, rows, cols, intr, frame_salt=k)
        td, tc = 1305031102.160407 + 0.033 * k, 1305031102.175304 + 0.033 * k
        _write_png(str(tmp_path / "depth" / f"{td:.6f}.png"), d)
        _write_png(str(tmp_path / "rgb" / f"{tc:.6f}.png"), g)
        lines.append(f"{td:.6f} depth/{td:.6f}.png {tc:.6f} rgb/{tc:.6f}.png")
        frames.append((float(f"{td:.6f}"), d, float(f"{tc:.6f}"), g))
    assoc = tmp_path / "associations.txt"
    assoc.write_text("\n".join(lines) + "\n")
    ply, spec, voxel = tmp_path / "map.ply", "0,100000,16", 0.05
    cmd = [_cli(), "fr1", str(assoc), "--quiet", "--map", f"{ply},{spec}", "--map-voxel", f"{voxel},{SLOTS}", "--map-normals", "1,0.05",
           "--map-icp", "0.05,6", "--map-icp-means", "2,1"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0 and len(r.stdout.strip().splitlines()) == n - 1, r.stderr
    line = re.search(r"^map-icp-means: attempted (\d+) accepted (\d+) kept / resolved ([0-9.]+)$", r.stderr, re.M)
    assert line, r.stderr
    assert re.search(r"^map-icp: attempted (\d+) accepted (\d+)$", r.stderr, re.M), r.stderr   # the correction's own line stays
    cfg = V.Config(nb_levels=6, intrinsics=V.Intrinsics(intr[:2], intr[2:4], intr[4]))
    one = V.Tracker(cfg, frames[0][0], frames[0][1], frames[0][2], frames[0][3], map=tuple(int(x) for x in spec.split(",")),
                    map_voxels=(voxel, SLOTS), map_voxel_stats=True, map_normals=(1, 0.05), map_icp=CLI_ICP, map_icp_means=(2, 1))
    out, shares = [], []
    for td, d, tc, g in frames[1:]:
        one.track(td, d, tc, g)
        t, pose = one.current_frame()
        out.append(np.asarray(pose, np.float32))
        m = one.read_map_icp_means()
        if m["resolved"]:
            shares.append(m["kept"] / m["resolved"])
    totals = one.read_map_icp()["totals"]
    assert (int(line.group(1)), int(line.group(2))) == (int(totals[0]), int(totals[1])) and int(line.group(1)) >= 2
    assert line.group(3) == f"{np.mean(shares):.4f}" and 0.0 < float(line.group(3)) < 1.0
    # the same trajectory, bit for bit: the CLI prints `timestamp tx ty tz qx qy qz qw` with enough digits to round-trip a float32
    cli = np.array([[float(x) for x in l.split()[1:]] for l in r.stdout.strip().splitlines()], np.float64).astype(np.float32)
    want = np.stack(out)
    assert cli.shape == want.shape == (n - 1, 7)
    assert cli.tobytes() == want.tobytes(), f"the CLI's trajectory differs from the Python Tracker's by {np.abs(cli - want).max()}"


@pytest.mark.parametrize("flags, word", [
    (["--map", "M.ply", "--map-voxel", "0.05", "--map-normals", "1", "--map-icp", "0.05", "--map-icp-means", "abc"], "Malformed --map-icp-means"),
    (["--map", "M.ply", "--map-voxel", "0.05", "--map-normals", "1", "--map-icp", "0.05", "--map-icp-means", "2,1,0"], "Malformed --map-icp-means"),
    (["--map", "M.ply", "--map-voxel", "0.05", "--map-normals", "1", "--map-icp", "0.05", "--map-icp-means"], "Malformed --map-icp-means"),
    (["--map", "M.ply", "--map-normals", "1", "--map-icp", "0.05", "--map-icp-means", "2,1"], "--map-icp-means needs --map-voxel"),
    (["--map", "M.ply", "--map-voxel", "0.05", "--map-normals", "1", "--map-icp-means", "2,1"], "--map-icp-means needs --map-icp")],
    ids=["not_a_number", "three_fields", "no_value", "without_map_voxel", "without_map_icp"])
def test_cli_refuses_a_bad_map_icp_means_with_the_usage(tmp_path, flags, word):
    """Status 2 and the usage on stderr, before any file is read or any device touched: the associations file does not even exist."""
    flags = [f.replace("M.ply", str(tmp_path / "never.ply")) for f in flags]
    r = subprocess.run([_cli(), "fr1", str(tmp_path / "no_such_associations.txt")] + flags, capture_output=True, text=True)
    assert r.returncode == 2 and "Usage: ./vors_track" in r.stderr and word in r.stderr and r.stdout == ""
    assert not os.path.exists(tmp_path / "never.ply")
