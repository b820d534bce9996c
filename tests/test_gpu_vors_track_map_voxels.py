"""`vors_track --map FILE --map-voxel SIZE_M[,TABLE_SLOTS]` end to end on the GPU: the small synthetic TUM-format sequence of
tests/test_gpu_vors_track_map.py through the CLI, and the PLY it writes against Tracker(map=..., map_voxels=...).read_map() on the same
frames — vertex count, segment lines and the payload byte for byte; fewer vertices than without the flag; the same trajectory. A malformed
--map-voxel, or one without --map, prints the usage and exits with status 2."""
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
DEFAULT_TABLE_SLOTS = 8 << 20   # vors_track.cpp MAP_VOXEL_DEFAULT_TABLE_SLOTS


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


@pytest.mark.parametrize("voxel, slots", [("0.02", None), ("0.05,65536", 65536)], ids=["default_table", "explicit_table"])
def test_cli_map_voxel_equals_read_map(tmp_path, voxel, slots):
    rows, cols, n = 240, 320, 8   # (the CLI's configuration has 6 levels: the coarsest is 7x10)
    intr = O.INTRINSICS_FR1
    os.makedirs(tmp_path / "depth")
    os.makedirs(tmp_path / "rgb")
    step = 4 * np.array([0.010, -0.004, 0.003, 0.0015, -0.002, 0.001])   # fast enough for several promotions in 7 frames
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
    ply, ply_all = tmp_path / "map.ply", tmp_path / "all.ply"
    spec = "0,100000,16"
    base = [_cli(), "fr1", str(assoc), "--quiet"]
    r = subprocess.run(base + ["--map", f"{ply},{spec}", "--map-voxel", voxel], capture_output=True, text=True)
    assert r.returncode == 0 and len(r.stdout.strip().splitlines()) == n - 1, r.stderr
    assert "voxel table" not in r.stderr   # no overflow warning
    unfiltered = subprocess.run(base + ["--map", f"{ply_all},{spec}"], capture_output=True, text=True)
    assert unfiltered.returncode == 0 and unfiltered.stdout == r.stdout   # the filter only reads
    args = tuple(int(x) for x in spec.split(","))
    cfg = V.Config(nb_levels=6, intrinsics=V.Intrinsics(intr[:2], intr[2:4], intr[4]))
    one = V.Tracker(cfg, frames[0][0], frames[0][1], frames[0][2], frames[0][3], map=args,
                    map_voxels=(float(voxel.split(",")[0]), DEFAULT_TABLE_SLOTS if slots is None else slots))
    for td, d, tc, g in frames[1:]:
        one.track(td, d, tc, g)
    m, v = one.read_map(), one.read_map_voxels()
    assert m["n_segments"] >= 3, "the sequence must promote at least twice"
    assert v == dict(occupied=m["count"], overflow=0) and m["count"] <= args[1]
    count, text, payload = _vertices(ply)
    count_all, _, _ = _vertices(ply_all)
    assert count == len(m["gray"]) == m["count"] and 0 < count < count_all, f"{count} vertices with the filter, {count_all} without"
    seg = [l.split()[2:] for l in text if l.startswith("comment segment")]
    assert len(seg) == len(m["segments"])
    for got, want in zip(seg, m["segments"]):
        assert [int(x) for x in got[:3]] == [int(want["frame"]), int(want["first"]), int(want["count"])]
        assert np.array([float(x) for x in got[3:]], np.float32).tobytes() == want["pose7"].tobytes()
    rec = np.frombuffer(payload, np.dtype([("xyz", "<f4", (3,)), ("i", "u1")]))
    assert len(payload) == 13 * count and rec["xyz"].tobytes() == m["xyz"].tobytes() and rec["i"].tobytes() == m["gray"].tobytes()


@pytest.mark.parametrize("flags", [["--map", "M.ply", "--map-voxel", "abc"], ["--map", "M.ply", "--map-voxel", "0.02,"],
                                   ["--map", "M.ply", "--map-voxel", "0.02,64,1"], ["--map", "M.ply", "--map-voxel", "0.02x"],
                                   ["--map", "M.ply", "--map-voxel"], ["--map-voxel", "0.02"], ["--map-voxel", "0.02,65536", "--quiet"]],
                         ids=["not_a_number", "empty_slots", "three_fields", "trailing_text", "no_value", "without_map", "without_map_2"])
def test_cli_refuses_a_bad_map_voxel_with_the_usage(tmp_path, flags):
    """Status 2 and the usage on stderr, before any file is read or any device touched: the associations file does not even exist."""
    flags = [f.replace("M.ply", str(tmp_path / "never.ply")) for f in flags]
    r = subprocess.run([_cli(), "fr1", str(tmp_path / "no_such_associations.txt")] + flags, capture_output=True, text=True)
    assert r.returncode == 2 and "Usage: ./vors_track" in r.stderr and "--map-voxel" in r.stderr and r.stdout == ""
    assert not os.path.exists(tmp_path / "never.ply")
