"""`vors_track --map-icp-joint PHOTO_SCALE_M[,PHOTO_HUBER_GREY[,MAX_DILUTION_T[,MAX_DILUTION_R]]]`: malformed input or a missing --map-icp
prints the usage and exits with status 2 before any device is touched; a well-formed flag reaches the reference's own checks. Needs no GPU."""
import pytest

from test_normals_args import USAGE, vors_track

BASE = ["--map", "m.ply", "--map-normals", "2"]


@pytest.mark.parametrize("args, word", [
    (BASE + ["--map-icp", "0.05", "--map-icp-joint"], "Malformed --map-icp-joint"),            # no value
    (BASE + ["--map-icp", "0.05", "--map-icp-joint", ""], "Malformed --map-icp-joint"),
    (BASE + ["--map-icp", "0.05", "--map-icp-joint", "x"], "Malformed --map-icp-joint"),       # not a number
    (BASE + ["--map-icp", "0.05", "--map-icp-joint", "0.0005,"], "Malformed --map-icp-joint"),  # a comma and nothing after it
    (BASE + ["--map-icp", "0.05", "--map-icp-joint", "0.0005,10,80,70,1"], "Malformed --map-icp-joint"),  # a fifth field
    (BASE + ["--map-icp", "0.05", "--map-icp-joint", "0.0005,10m"], "Malformed --map-icp-joint"),
    (BASE + ["--map-icp-joint", "0.0005"], "--map-icp-joint needs --map-icp"),
    (["--map-icp-joint", "0.0005,10", "--quiet"], "--map-icp-joint needs --map-icp"),
])
def test_cli_map_icp_joint_argument_errors(args, word, tmp_path):
    r = vors_track(args, tmp_path)
    assert r.returncode == 2 and USAGE in r.stderr and word in r.stderr and r.stdout == ""


def test_cli_well_formed_map_icp_joint_reaches_the_reference_checks(tmp_path):
    for args in (BASE + ["--map-icp", "0.05", "--map-icp-joint", "0.0005"], BASE + ["--map-icp-joint", "0,0,80,70", "--map-icp", "0.05,6,0,0.9,0.002"],
                 BASE + ["--map-icp", "0.05", "--map-icp-joint", "0.0005,10,80,70"]):
        r = vors_track(args, tmp_path)
        assert r.returncode == 0 and "The association file does not exist or is not reachable" in r.stderr and r.stdout == ""
