"""CPU test of the one-pass destuffing walk (spdl_amd/csrc/hj_destuff_tile.h, no
GPU): the per-group step destuff_image_kernel takes -- classify, carry in,
kept count, carry out -- the cut at the terminator and the running offset over
tiles, against a byte loop over the whole scan
(tests/native/destuff_tile_sweep.cpp), built with ASan and UBSan as a program
of its own.

The sweep, at tiles of 1, 2, 3 and 8 groups: FF 00, FF FF .. FF 00, FF .. Dn,
FF D9 and a lone last FF at each of the 34 byte positions around a tile
boundary, for every scan_start % 16 and with the file ending at every byte
after the pattern; scans of 1, tile - 1, tile, tile + 1 and 2 tiles +- 1
bytes; scans of FF 00 pairs alone; 200 k random scans of up to five tiles.
The data bytes, the segment starts, the restart count and the scan end are
equal.
"""

import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_destuff_tile_walk_sweep_under_sanitizers(tmp_path):
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
    exe = str(tmp_path / "destuff_tile_sweep")
    subprocess.run([cxx, "-std=c++17", "-O2", "-g", "-DHJ_HD=", *san,
                    os.path.join(ROOT, "tests", "native", "destuff_tile_sweep.cpp"), "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("scans ") and not r.stderr, r.stdout + r.stderr
    scans, patterns, random = (int(r.stdout.split()[i]) for i in (1, 3, 5))
    assert patterns >= 4 * 16 * 17 * 4 * 5 and random == 200_000 and scans > 10 * patterns
