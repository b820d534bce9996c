"""`vors_track --map` end to end on the GPU: a small synthetic TUM-format sequence through the CLI, and the PLY it writes against
Tracker(map=...).read_map() on the same frames — header counts, one comment line per segment with the record's values, and the payload
(x y z float32 little-endian + intensity) byte for byte. Without the flag the CLI prints the same trajectory."""
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


@pytest.mark.parametrize("spec, depth_filter", [("0,100000,16", None), ("1,500,2", None), ("0,100000,16,2", "0.02,255,1")],
                         ids=["level0", "level1_clipped", "filtered_min_weight_2"])
def test_cli_map_equals_read_map(tmp_path, spec, depth_filter):
    if not all(os.path.exists(os.path.join(HOST, b)) for b in ("ply_io_test", "vors_track")):
        subprocess.check_call(["make", "-C", HOST, "-s"])
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
    ply = tmp_path / "map.ply"
    base = [os.path.join(HOST, "vors_track"), "fr1", str(assoc), "--quiet"] + (["--depth-filter", depth_filter] if depth_filter else [])
    r = subprocess.run(base + ["--map", f"{ply},{spec}"], capture_output=True, text=True)
    assert r.returncode == 0 and len(r.stdout.strip().splitlines()) == n - 1, r.stderr
    plain = subprocess.run(base, capture_output=True, text=True)
    assert plain.stdout == r.stdout   # the map only reads
    args = tuple(int(x) for x in spec.split(","))
    cfg = V.Config(nb_levels=6, intrinsics=V.Intrinsics(intr[:2], intr[2:4], intr[4]))
    one = V.Tracker(cfg, frames[0][0], frames[0][1], frames[0][2], frames[0][3],
                    depth_filter=tuple(float(x) if i == 0 else int(x) for i, x in enumerate(depth_filter.split(","))) if depth_filter else None, map=args)
    for td, d, tc, g in frames[1:]:
        one.track(td, d, tc, g)
    m = one.read_map()
    assert m["n_segments"] >= 3, "the sequence must promote at least twice"
    clipped = m["count"] > args[1]
    assert clipped == (spec == "1,500,2")
    assert ("capacity" in r.stderr) == clipped and ("segment records" in r.stderr) == (m["n_segments"] > args[2])
    data = open(ply, "rb").read()
    head, _, payload = data.partition(b"end_header\n")
    text = head.decode().splitlines()
    assert f"element vertex {len(m['gray'])}" in text
    seg = [l.split()[2:] for l in text if l.startswith("comment segment")]
    assert len(seg) == len(m["segments"])
    for got, want in zip(seg, m["segments"]):
        assert [int(x) for x in got[:3]] == [int(want["frame"]), int(want["first"]), int(want["count"])]
        assert np.array([float(x) for x in got[3:]], np.float32).tobytes() == want["pose7"].tobytes()
    rec = np.frombuffer(payload, np.dtype([("xyz", "<f4", (3,)), ("i", "u1")]))
    assert len(payload) == 13 * len(m["gray"]) and rec["xyz"].tobytes() == m["xyz"].tobytes() and rec["i"].tobytes() == m["gray"].tobytes()
