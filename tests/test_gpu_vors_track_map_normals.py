"""`vors_track --map ... --map-normals` end to end on the GPU: the PLY the CLI writes carries, vertex for vertex, the points of
Tracker(map=..., map_normals=...).read_map() and the normals of read_map_normals() on the same frames, byte for byte, and the trajectory
is the one printed without the flag."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import vors_amd as V
from oracle import oracle as O
from test_gpu_vors_track_map import _write_png

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "visual-odometry-rs_amd", "host")
WITH = np.dtype([("xyz", "<f4", (3,)), ("n", "<f4", (3,)), ("i", "u1")])


def test_cli_ply_carries_the_handles_normals(tmp_path):
    if not os.path.exists(os.path.join(HOST, "vors_track")):
        subprocess.check_call(["make", "-C", HOST, "-s"])
    rows, cols, n = 240, 320, 6   # (the CLI's configuration has 6 levels: the coarsest is 7x10)
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
    ply = tmp_path / "map.ply"
    base = [os.path.join(HOST, "vors_track"), "fr1", str(assoc), "--quiet"]
    r = subprocess.run(base + ["--map", f"{ply},0,100000,16", "--map-normals", "2,0.05"], capture_output=True, text=True)
    assert r.returncode == 0 and len(r.stdout.strip().splitlines()) == n - 1, r.stderr
    assert subprocess.run(base, capture_output=True, text=True).stdout == r.stdout   # the normals only read
    cfg = V.Config(nb_levels=6, intrinsics=V.Intrinsics(intr[:2], intr[2:4], intr[4]))
    one = V.Tracker(cfg, frames[0][0], frames[0][1], frames[0][2], frames[0][3], map=(0, 100000, 16), map_normals=(2, 0.05))
    for td, d, tc, g in frames[1:]:
        one.track(td, d, tc, g)
    m, normals = one.read_map(), one.read_map_normals()
    assert m["n_segments"] >= 2 and len(normals) == len(m["gray"]) > 0
    assert 2 * int(normals.any(axis=1).sum()) >= len(normals)
    head, _, payload = open(ply, "rb").read().partition(b"end_header\n")
    text = head.decode().splitlines()
    assert f"element vertex {len(m['gray'])}" in text and "property float nx" in text and "property float nz" in text
    rec = np.frombuffer(payload, WITH)
    assert len(payload) == 25 * len(m["gray"])
    assert rec["xyz"].tobytes() == m["xyz"].tobytes() and rec["i"].tobytes() == m["gray"].tobytes() and rec["n"].tobytes() == normals.tobytes()
