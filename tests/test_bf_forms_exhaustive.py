"""The branch-free closed forms of a read's trims (amplipy_amd/csrc/amp_bf.hpp, what k_fast, k_fast5 and k_fast7 run) against the
branchy forms of amp_read.hpp over a COMPLETE small domain: tests/hostsim/bf_forms_main.cpp walks every shape
[S a][M m1]([I|D k][M m2])[S c] with a query of at most 12 bases -- the shapes a clip leaves behind included: m1 = 0, m2 = 0, the read
that is one soft clip -- under every clip amount from -2 to 14 with both flavours of bf_clip_left, both coordinate maps at every
offset, and the whole trim with either table entry absent or present at every offset, both strands, paired or not, the
template-length test on and off, and EVERY outcome of the window scan.  Field for field: the five lengths, kind, op, punt, the
position, the flags, the reference advance.  (tests/test_hostsim_golden.py::test_branch_free_closed_forms fuzzes the same pair on
reads of real lengths; the branchy forms are fuzzed against the generic code there.)

The program has its own main and is host code only: it is built with -fsanitize=address,undefined and run as a child process.
No GPU needed."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostsim", "bf_forms_main.cpp")
QMAX = 12


def _domain_size(qmax):
    """Shapes bf_forms_main.cpp visits, counted from its rules: parts (a, m1, [k, m2,] c) with a query of 1..qmax bases; insertions of
    1..8 (they are query bases), deletions of 1, 2 and 16; no indel between two clips; one soft clip is written [S a]; the op '=' on
    the shapes whose clips sum to a multiple of 3."""
    n = 0
    for kind in (0, 1, 2):
        for a in range(qmax + 1):
            for m1 in range(qmax + 1 - a):
                for k in ((0,) if kind == 0 else range(1, 9) if kind == 1 else (1, 2, 16)):
                    for m2 in range((qmax if kind else 0) + 1):
                        for c in range(qmax + 1):
                            q = a + m1 + (k if kind == 1 else 0) + m2 + c
                            if not 1 <= q <= qmax or (kind and m1 == 0 and m2 == 0) or (not kind and m1 == 0 and c):
                                continue
                            n += 1 if (a + c) % 3 else 2
    return n


def test_closed_forms_over_the_complete_small_domain(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "bf_forms")
    # (the headers under test are HIP headers: the host half of a HIP compile, nothing for the device)
    subprocess.check_call([hipcc, "-x", "hip", "--cuda-host-only", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, SRC])
    r = subprocess.run([exe, str(QMAX)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert not r.stderr
    words = r.stdout.split()
    assert words[:2] == ["bf_forms", "ok"], r.stdout
    shapes, clips, maps, trims, qtrims, punted = (int(w) for w in words[2:])
    assert shapes == _domain_size(QMAX)
    # every shape under 17 primer clips, 15 quality clips and 14 clips behind the leading soft clip
    assert clips == shapes * (17 + 15 + 14)
    # the whole trim runs on the input shapes alone, 8 flag combinations each, and every one that is not punted is followed by
    # its quality trims, one per scan outcome
    assert trims % 8 == 0 and trims > 10 ** 7 and qtrims > 2 * trims and maps > 20 * shapes
    assert 0 < punted < clips
