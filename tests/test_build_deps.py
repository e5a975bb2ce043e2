"""build.py's dependency lists against what the compiler sees: a header a unit includes and UNIT_DEPS does not name means
that an edit of the header leaves the unit's stale object in the library, silently."""
import os
import re
import shutil
import subprocess

import pytest

from amplipy_amd import build

ROOT = os.path.realpath(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.isfile("/opt/rocm/bin/hipcc") else None)
OURS = (os.path.join(ROOT, "amplipy_amd", "csrc") + os.sep, os.path.join(ROOT, "include") + os.sep)


def _real(paths):
    return {os.path.realpath(p) for p in paths}


@pytest.mark.skipif(HIPCC is None, reason="hipcc reports the includes")
@pytest.mark.parametrize("unit", build.UNITS)
def test_unit_deps_name_every_header_the_unit_includes(unit):
    src = os.path.join(build.CSRC, unit)
    rule = subprocess.check_output([HIPCC] + build.FLAGS + ["--cuda-host-only", "-MM", src], text=True, stderr=subprocess.DEVNULL)
    # a make rule: "unit.o: file file \" over several lines
    files = _real(re.sub(r"\\\n", " ", rule).split(":", 1)[1].split())
    ours = {f for f in files if f.startswith(OURS)}
    assert os.path.realpath(src) in ours
    missing = ours - _real(build.UNIT_DEPS[unit]) - {os.path.realpath(src)}
    assert not missing, "%s includes %s: not in build.UNIT_DEPS" % (unit, sorted(missing))


def test_every_unit_and_dependency_triggers_a_build():
    assert set(build.UNIT_DEPS) == set(build.UNITS)
    deps = _real(build.DEPS)
    for unit in build.UNITS:
        assert os.path.realpath(os.path.join(build.CSRC, unit)) in deps, unit
        for d in build.UNIT_DEPS[unit]:
            assert os.path.isfile(d), d
            assert os.path.realpath(d) in deps, "%s of %s is not in build.DEPS" % (d, unit)
