"""The host side of `vors_track --map` that needs no device: the PLY writer's stand-alone self-test (host/ply_io_test.cpp: two segments,
header and payload parsed back, byte counts, little-endian floats, comment lines, the file without points) and the flag's argument
errors, which print the usage and exit non-zero before any device is touched."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "visual-odometry-rs_amd", "host")
USAGE = "Usage: ./vors_track [fr1|fr2|fr3|icl] associations_file"


def _ensure_host_built():
    if not all(os.path.exists(os.path.join(HOST, b)) for b in ("ply_io_test", "vors_track")):
        subprocess.check_call(["make", "-C", HOST, "-s"])


def test_ply_writer_selftest(tmp_path):
    _ensure_host_built()
    out = subprocess.run([os.path.join(HOST, "ply_io_test"), str(tmp_path)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert "ply_io_test: ok" in out.stdout
    # the file it left behind, read independently: header in text, 13 bytes per vertex
    data = open(tmp_path / "two_segments.ply", "rb").read()
    head, _, payload = data.partition(b"end_header\n")
    lines = head.decode().splitlines()
    assert lines[:2] == ["ply", "format binary_little_endian 1.0"] and "element vertex 5" in lines
    assert [l.split()[2:5] for l in lines if l.startswith("comment segment")] == [["0", "0", "3"], ["7", "3", "2"]]
    assert len(payload) == 5 * 13 and payload[:4] == b"\x00\x00\x80\x3f" and payload[12] == 0 and payload[-1] == 255


@pytest.mark.parametrize("args, word", [
    (["--map"], "Malformed --map"),                                   # no value
    (["--map", ""], "Malformed --map"),                               # empty file name
    (["--map", ",0"], "Malformed --map"),
    (["--map", "m.ply,"], "Malformed --map"),                         # a comma and nothing after it
    (["--map", "m.ply,0,12x"], "Malformed --map"),                    # not a number
    (["--map", "m.ply,0,100,4,0,9"], "Malformed --map"),              # a sixth field
    (["--map", "m.ply,0,99999999999"], "Malformed --map"),            # does not fit an int
    (["--map", "m.ply,0,100,4,2"], "needs --depth-filter"),           # MIN_WEIGHT >= 2 without the filter
    (["--quiet", "--map", "m.ply,0,100,4,255", "--arith", "fused"], "needs --depth-filter"),
])
def test_cli_map_argument_errors(args, word, tmp_path):
    _ensure_host_built()
    r = subprocess.run([os.path.join(HOST, "vors_track"), "fr1", "/nonexistent/assoc.txt"] + args, capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode != 0 and USAGE in r.stderr and word in r.stderr and r.stdout == ""
    assert not os.path.exists(tmp_path / "m.ply")


def test_cli_well_formed_map_flag_reaches_the_reference_checks(tmp_path):
    """A well-formed --map (with the filter where MIN_WEIGHT asks for it) is accepted: the next check is the reference's own."""
    _ensure_host_built()
    for args in (["--map", "m.ply"], ["--map", "m.ply,1,5000,8"], ["--depth-filter", "0.02", "--map", "m.ply,0,5000,8,2"],
                 ["--map", "m.ply,0,5000,8,2", "--depth-filter", "0.02"]):
        r = subprocess.run([os.path.join(HOST, "vors_track"), "fr1", "/nonexistent/assoc.txt"] + args, capture_output=True, text=True, cwd=tmp_path)
        assert r.returncode == 0 and "The association file does not exist or is not reachable" in r.stderr and r.stdout == ""
