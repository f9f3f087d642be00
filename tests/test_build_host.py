"""csrc/Makefile against the directory it builds, without a device: every translation unit is in SRC, every header in HDR (a rule's prerequisite: an
edit rebuilds what includes it), and neither names a file that is not there.  A .hip file that SRC forgets still builds a library -- one that fails
to load with an undefined symbol, on the machine that has the GPU."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ti_raytrace_amd", "csrc")


def _make_list(name):
    text = open(os.path.join(CSRC, "Makefile")).read().replace("\\\n", " ")
    found = re.findall(r"^%s\s*=(.*)$" % name, text, flags=re.M)
    assert len(found) == 1, "%s is assigned %d times in csrc/Makefile" % (name, len(found))
    return found[0].split()


def _on_disk(pattern):
    return sorted(os.path.basename(p) for p in glob.glob(os.path.join(CSRC, pattern)))


def test_every_translation_unit_is_in_SRC():
    src = _make_list("SRC")
    assert len(src) == len(set(src)), "SRC names a file twice"
    assert sorted(src) == _on_disk("*.hip")


def test_every_header_is_in_HDR():
    hdr = _make_list("HDR")
    assert len(hdr) == len(set(hdr)), "HDR names a file twice"
    assert sorted(h for h in hdr if "/" not in h) == _on_disk("*.h")


def test_SRC_and_HDR_name_files_that_exist():
    missing = [f for f in _make_list("SRC") + _make_list("HDR") if not os.path.isfile(os.path.join(CSRC, f))]
    assert not missing, missing
