"""`vors_track --map FILE --map-voxel SIZE_M --map-voxel-means MIN_COUNT[,MIN_SPAN]` end to end on the GPU: the small synthetic TUM-format
sequence of tests/test_gpu_vors_track_map.py through the CLI, and the PLY it writes against Tracker(map_voxel_stats=True) on the same
frames: the `obs` property, the vertices = the ranks the Python resolve keeps (centroid, mean grey and observation count byte for byte),
rejected ranks left out, the same trajectory, the normals carried along. Malformed, or without --map-voxel: the usage and status 2."""
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import vors_amd as V
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "visual-odometry-rs_amd", "host")
SLOTS = 65536


def _write_png(path, arr):
    """8-bit grey (uint8) or 16-bit big-endian grey (uint16) PNG, filter 0."""
    h, w = arr.shape
    depth = 16 if arr.dtype == np.uint16 else 8
    raw = arr.astype(">u2").tobytes() if depth == 16 else arr.tobytes()
    stride = len(raw) // h
    scan = b"".join(b"\x00" + raw[y * stride:(y + 1) * stride] for y in range(h))

    def chunk(t, d):
        return struct.pack(">I", len(d)) + t + d + struct.pack(">I", zlib.crc32(t + d) & 0xffffffff)

    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, 0, 0, 0, 0)) +
                chunk(b"IDAT", zlib.compress(scan, 1)) + chunk(b"IEND", b""))


def _cli():
    if not os.path.exists(os.path.join(HOST, "vors_track")):
        subprocess.check_call(["make", "-C", HOST, "-s"])
    return os.path.join(HOST, "vors_track")


def _vertices(path):
    head, _, payload = open(path, "rb").read().partition(b"end_header\n")
    n = [int(l.split()[2]) for l in head.decode().splitlines() if l.startswith("element vertex")][0]
    return n, head.decode().splitlines(), payload


@pytest.mark.parametrize("means, normals", [("1", False), ("2,1", True)], ids=["every_rank", "thresholds_and_normals"])
def test_cli_map_voxel_means_equals_the_python_resolve(tmp_path, means, normals):
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
    ply, ply_first = tmp_path / "means.ply", tmp_path / "first.ply"
    spec, voxel = "0,100000,16", 0.05
    base = [_cli(), "fr1", str(assoc), "--quiet", "--map-voxel", f"{voxel},{SLOTS}"] + (["--map-normals", "1,0.05"] if normals else [])
    r = subprocess.run(base + ["--map", f"{ply},{spec}", "--map-voxel-means", means], capture_output=True, text=True)
    assert r.returncode == 0 and len(r.stdout.strip().splitlines()) == n - 1, r.stderr
    plain = subprocess.run(base + ["--map", f"{ply_first},{spec}"], capture_output=True, text=True)
    assert plain.returncode == 0 and plain.stdout == r.stdout   # the statistics only read
    args = tuple(int(x) for x in spec.split(","))
    cfg = V.Config(nb_levels=6, intrinsics=V.Intrinsics(intr[:2], intr[2:4], intr[4]))
    one = V.Tracker(cfg, frames[0][0], frames[0][1], frames[0][2], frames[0][3], map=args, map_voxels=(voxel, SLOTS), map_voxel_stats=True,
                    map_normals=(1, 0.05) if normals else None)
    for td, d, tc, g in frames[1:]:
        one.track(td, d, tc, g)
    mc, ms = (int(x) for x in (means.split(",") + ["0"])[:2])
    m, res, st = one.read_map(), one.map_voxel_means(mc, ms), one.read_map_voxel_stats()
    keep = np.isfinite(res["xyz_mean"][:, 0])
    assert m["n_segments"] >= 3 and res["kept"] == int(keep.sum()) > 0
    count, text, payload = _vertices(ply)
    count_first, _, _ = _vertices(ply_first)
    assert "property uint obs" in text and text.index("property uint obs") == text.index("property uchar intensity") + 1
    assert count == res["kept"] and count_first == m["count"]
    assert (count == count_first) if means == "1" else (count < count_first), f"{count} vertices of {count_first} ranks"
    assert len([l for l in text if l.startswith("comment segment")]) == len(m["segments"])
    fields = [("xyz", "<f4", (3,))] + ([("n", "<f4", (3,))] if normals else []) + [("i", "u1"), ("obs", "<u4")]
    rec = np.frombuffer(payload, np.dtype(fields))
    assert len(payload) == rec.dtype.itemsize * count
    assert rec["xyz"].tobytes() == res["xyz_mean"][keep].tobytes() and rec["i"].tobytes() == res["gray_mean"][keep].tobytes()
    assert rec["obs"].tobytes() == st["obs"][keep, 0].tobytes() and (rec["obs"] >= max(mc, 1)).all()
    if normals:
        assert rec["n"].tobytes() == one.read_map_normals()[keep].tobytes()


@pytest.mark.parametrize("flags", [["--map", "M.ply", "--map-voxel", "0.02", "--map-voxel-means", "abc"],
                                   ["--map", "M.ply", "--map-voxel", "0.02", "--map-voxel-means", "2,"],
                                   ["--map", "M.ply", "--map-voxel", "0.02", "--map-voxel-means", "2,1,0"],
                                   ["--map", "M.ply", "--map-voxel", "0.02", "--map-voxel-means", "-1"],
                                   ["--map", "M.ply", "--map-voxel", "0.02", "--map-voxel-means"],
                                   ["--map", "M.ply", "--map-voxel-means", "2"]],
                         ids=["not_a_number", "empty_span", "three_fields", "negative", "no_value", "without_map_voxel"])
def test_cli_refuses_a_bad_map_voxel_means_with_the_usage(tmp_path, flags):
    """Status 2 and the usage on stderr, before any file is read or any device touched: the associations file does not even exist."""
    flags = [f.replace("M.ply", str(tmp_path / "never.ply")) for f in flags]
    r = subprocess.run([_cli(), "fr1", str(tmp_path / "no_such_associations.txt")] + flags, capture_output=True, text=True)
    assert r.returncode == 2 and "Usage: ./vors_track" in r.stderr and "--map-voxel-means" in r.stderr and r.stdout == ""
    assert not os.path.exists(tmp_path / "never.ply")
