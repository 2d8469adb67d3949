"""CPU test of the destuffing core (spdl_amd/csrc/hj_destuff.h, no GPU): the
word-parallel classification, the marker look-ahead and the register
compaction the destuff kernels are built from, against a byte-loop
restatement of the rule (tests/native/destuff_sweep.cpp), built with ASan and
UBSan as a program of its own.

The sweep: every 3-byte pattern over {00, FF, D0, D7, D9, 5A} at every
position of the 18-byte window (byte before, 16-byte group, byte after), on
every filler of that alphabet; fill 0xFF runs of every length leaving the
group; every start / end cut inside the group and the file ending at every
byte of it; 1 M random groups with 0xFF at probability 1/8.  The keep mask,
the restart bits, the terminator position and the compacted bytes are equal.
"""

import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_destuff_core_sweep_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    # (runtimes linked statically: the program then runs whatever the environment preloads)
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
           "-static-libubsan"]
    probe_src = tmp_path / "probe.cpp"
    probe_src.write_text("int main() { return 0; }\n")
    if subprocess.run([cxx, *san, str(probe_src), "-o", str(tmp_path / "probe")],
                      capture_output=True).returncode:
        pytest.skip("the compiler has no sanitizer runtime")
    exe = str(tmp_path / "destuff_sweep")
    subprocess.run([cxx, "-std=c++17", "-O2", "-g", "-DHJ_HD=", *san,
                    os.path.join(ROOT, "tests", "native", "destuff_sweep.cpp"), "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("groups ") and not r.stderr, r.stdout + r.stderr
    groups, windows, random = (int(r.stdout.split()[i]) for i in (1, 3, 5))
    assert windows >= 6 * 16 * 6 ** 3 and random == 1_000_000 and groups > 700 * windows
