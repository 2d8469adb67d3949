"""CPU test of idct_kernel's block index function (spdl_amd/csrc/hj_common.h:
idct_block_pos -- block j of an image -> component, block column and row in
the component's plane -- with the multiply-and-correct division idct_divmod,
no GPU): the function the kernel calls, compiled for the host, against plain
/ and % (tests/native/idct_index_sweep.cpp), built with ASan and UBSan as a
program of its own.

The sweep: bpm in {1, 2, 3, 4, 6, 8, 10} x mcux in {1, 2, 3, 5, 41, 80, 255,
256, 257, 4096, 8192}, each image as tall as nblocks < 2^24 allows; every j
below min(nblocks, 2^20) and the last 2^16 values below 2^24.  The division
alone also on divisors and dividends up to 2^32 - 1.
"""

import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_idct_block_index_sweep_under_sanitizers(tmp_path):
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
    exe = str(tmp_path / "idct_index_sweep")
    subprocess.run([cxx, "-std=c++17", "-O2", "-g", "-DHJ_HD=", *san,
                    os.path.join(ROOT, "tests", "native", "idct_index_sweep.cpp"), "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("images ") and not r.stderr, r.stdout + r.stderr
    images, positions = (int(r.stdout.split()[i]) for i in (1, 3))
    assert images == 7 * 11
    # 2^16 top values per image, and every j of the images below 2^20 blocks
    assert positions >= images * (1 << 16) + 70 * (1 << 20)
