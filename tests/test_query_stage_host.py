"""The layout of the queries' host staging (stage_layout, csrc/tirt_query_stage.h) without a device: tools/query_stage_check.cpp, a stand-alone program,
built for the host alone with the address and undefined-behaviour sanitizers and run.  The host entries copy their arrays into one device buffer whose size
is the layout's total: a column that ends behind it is a write out of bounds on the device, so offsets, alignment and total are held here, where a
mistake costs nothing -- the column lists of all seven routes, n in {1, 2, 3, 255, 256, 257}, k in {0, 1, 3, 64}, pair capacities {0, 1, 7}."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_layout_of_every_host_route_under_the_host_sanitizers(tmp_path):
    exe = str(tmp_path / "query_stage_check")
    subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--cuda-host-only", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", os.path.join(ROOT, "tools", "query_stage_check.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "228 cases, 0 failed" in run.stdout, run.stdout
