"""The rounding of the sphere sweep's float32 definition against its float64 evaluation on the two input sets of tests/test_sweep_host.py
(tests/sweep_expected.py: ACCURACY_SETS), through the host entry point -- no GPU involved.
   python tools/sweep_accuracy.py > profiles/sweep_accuracy.txt
The maxima printed here are the `measured` fields of ACCURACY_SETS; the test allows twice as much."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sweep_expected as SE                      # noqa: E402
from ti_raytrace_amd import _native             # noqa: E402

print("# tirt_kat_sweep_host (float32, the library's text compiled for the host) against tests/sweep_expected.py in float64, B = 1, segments with end points in")
print("# [-0.2, 1.2]^3, triangles in the unit box with edges below 0.4; a query is left out where some triangle's closest approach to the segment is")
print("# within r (1 +- 2^-8) (grazing); err = |T32 - T64| |d| over the kept queries with a contact; disagree = kept queries whose prim differs (a miss is -1)")
print("%-8s %5s %6s %9s %9s %8s %9s %12s" % ("set", "tris", "r", "segments", "left out", "kept", "contacts", "max err"))
for name, cfg in SE.ACCURACY_SETS.items():
    m = SE.accuracy_measure(name, _native.kat_sweep_host)
    print("%-8s %5d %6.3f %9d %8.2f%% %8d %9d %12.4e   disagree %d" % (name, cfg["ntri"], cfg["r"], cfg["nseg"], 100.0 * m["left_out"], m["n_kept"], m["contacts"],
                                                                  m["max_err"], m["disagree"]))
