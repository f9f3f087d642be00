"""The grid arithmetic behind the point walks' stacks (point_walk_grid, csrc/tirt_point_walk.h) without a device: tools/point_walk_grid_check.cpp, a
stand-alone program, built for the host alone with the address and undefined-behaviour sanitizers and run.  The kernels index the spill buffer as
[entry][grid * CP_BLOCK]: a grid larger than the buffer was sized for is a write out of bounds on the device, so the sizes are held here, where a
mistake costs nothing -- stack sizes 1, 16, 17 and 4096, one block of work and 2^20, both entry sizes."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_grid_and_tails_under_the_host_sanitizers(tmp_path):
    exe = str(tmp_path / "point_walk_grid_check")
    subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--cuda-host-only", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=undefined,address",
                    "-fno-sanitize-recover=all", os.path.join(ROOT, "tools", "point_walk_grid_check.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "128 cases, 0 failed" in run.stdout, run.stdout
