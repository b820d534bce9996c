"""The header's promises about threads, for the entries that need no handle, on the CPU: csrc/host_threads_check.cpp (its own main) runs
eight std::threads through vors_lm_step, vors_icp_points_joint_host, vors_render_points_host, vors_voxel_stats_host +
vors_voxel_means_host, vors_depth_normals_host and vors_icp_condition_from_sums with refused calls in between, and compares every
status, output byte and vors_last_error() with the same calls made serially first.

Built twice: plainly, and with -fsanitize=thread on the host side of operators.cpp and of the program. Both are run with --host-only
here: then vors_lm_solve, a device entry, is called for its refusals only and no device is opened (its valid calls from eight threads
are tests/test_gpu_threads.py's, marked gpu). Both are stand-alone executables run as child programs: nothing sanitised is loaded into
Python.

What the sanitizer half can and cannot see: it instruments operators.cpp (the thread-local last error and every host twin). The
process-wide VORS_PYRAMID_FUSED setting lives in kernels.hip behind launch_pyramid, which only a handle's step reaches, after a device
was required: no host-only program gets there, so that read is covered by tests/test_gpu_threads.py's fresh-process case and by reading.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "visual-odometry-rs_amd", "csrc")


def run_check(name, *args):
    out = subprocess.run([os.path.join(CSRC, name), *args], capture_output=True, text=True, timeout=300)
    report = out.stdout + out.stderr
    assert "ThreadSanitizer" not in report, report
    assert out.returncode == 0 and "host_threads_check: ok (8 threads" in out.stdout, report
    return out.stdout


def test_eight_threads_equal_the_serial_run():
    subprocess.check_call(["make", "-C", CSRC, "-s", "host_threads_check"])
    assert "host only" in run_check("host_threads_check", "--host-only")


def thread_sanitizer_link_failure(tmp_path):
    """Link a trivial program with the sanitizer, by the compiler and the flags of the Makefile -> None, or the linker's message."""
    hipcc, arch = [subprocess.run(["make", "-C", CSRC, "-s", "print-" + v], capture_output=True, text=True, check=True).stdout.strip()
                   for v in ("HIPCC", "ARCH")]
    src = tmp_path / "probe.cpp"
    src.write_text("#include <thread>\nint main() { std::thread t([] {}); t.join(); return 0; }\n")
    probe = subprocess.run([hipcc, "-x", "hip", f"--offload-arch={arch}", "-Xarch_host", "-fsanitize=thread", str(src), "-o", str(tmp_path / "probe"),
                            "-pthread"], capture_output=True, text=True)
    return None if probe.returncode == 0 else (probe.stderr.strip() or probe.stdout.strip() or f"exit status {probe.returncode}")


def test_eight_threads_under_the_thread_sanitizer(tmp_path):
    """A stand-alone program built with -fsanitize=thread. Skipped only where a trivial program does not link with the sanitizer, with the
    linker's message; once that links, whatever goes wrong in the real build is a failure."""
    message = thread_sanitizer_link_failure(tmp_path)
    if message is not None:
        pytest.skip("no compiler here links -fsanitize=thread: " + message.splitlines()[-1])
    subprocess.check_call(["make", "-C", CSRC, "-s", "host_threads_check_tsan"])
    assert "host only" in run_check("host_threads_check_tsan", "--host-only")
