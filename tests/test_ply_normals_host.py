"""The PLY writer's overload with normals (host/ply_io.hpp; needs no device): host/ply_normals_test.cpp writes one cloud through both
overloads of write_map and checks header and payload itself; the two files it leaves are read again here, independently. The existing
overload's bytes are pinned: they are the ones its own self-test (tests/test_ply_host.py) describes."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "visual-odometry-rs_amd", "host")
PLAIN = np.dtype([("xyz", "<f4", (3,)), ("i", "u1")])
WITH = np.dtype([("xyz", "<f4", (3,)), ("n", "<f4", (3,)), ("i", "u1")])


def test_ply_writer_with_normals(tmp_path):
    if not os.path.exists(os.path.join(HOST, "ply_normals_test")):
        subprocess.check_call(["make", "-C", HOST, "-s", "ply_normals_test"])
    out = subprocess.run([os.path.join(HOST, "ply_normals_test"), str(tmp_path)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert "ply_normals_test: ok" in out.stdout
    plain_head, _, plain = open(tmp_path / "plain.ply", "rb").read().partition(b"end_header\n")
    head, _, payload = open(tmp_path / "normals.ply", "rb").read().partition(b"end_header\n")
    lines, plain_lines = head.decode().splitlines(), plain_head.decode().splitlines()
    props = [l for l in lines if l.startswith("property")]
    assert props == ["property float x", "property float y", "property float z", "property float nx", "property float ny", "property float nz",
                     "property uchar intensity"]
    assert [l for l in lines if not l.startswith("property float n")] == plain_lines   # everything else is the old header
    assert "element vertex 5" in lines and len([l for l in lines if l.startswith("comment segment")]) == 2
    # the old overload: 13 bytes per vertex, properties x y z intensity, as before
    assert [l for l in plain_lines if l.startswith("property")] == ["property float x", "property float y", "property float z", "property uchar intensity"]
    assert len(plain) == 5 * 13 and plain[:4] == b"\x00\x00\x80\x3f" and plain[12] == 0 and plain[-1] == 255
    old, new = np.frombuffer(plain, PLAIN), np.frombuffer(payload, WITH)
    assert len(payload) == 5 * 25
    assert new["xyz"].tobytes() == old["xyz"].tobytes() and new["i"].tobytes() == old["i"].tobytes()
    want = np.array([[0, 0, -1], [0.6, 0, -0.8], [0, 0, 0], [-1, 0, 0], [0, 0.8, -0.6]], np.float32)
    assert new["n"].tobytes() == want.tobytes()
