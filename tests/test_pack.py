"""CPU tests of the pinned-staging copier as a unit (spdl_amd/csrc/hj_pack.cpp,
no HIP): the copier pool, the split pack and the split pread, swept by
tests/native/pack_sweep.cpp -- pools of 1, 2, 4 and 8 workers reused over 50
rounds, item lists on both sides of the 4 MiB threshold, every packed buffer
against a single-threaded pack -- once under ASan and UBSan and once under
TSan.  The pool is the project's only multi-threaded code.
"""

import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZERS = {
    # (runtimes linked statically: the program then runs whatever the environment preloads)
    "asan_ubsan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                   "-static-libubsan"],
    "tsan": ["-fsanitize=thread", "-static-libtsan"],
}


@pytest.mark.parametrize("kind", sorted(SANITIZERS))
def test_pack_sweep_under_sanitizers(tmp_path, kind):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    san = SANITIZERS[kind]
    probe_src = tmp_path / "probe.cpp"
    probe_src.write_text("int main() { return 0; }\n")
    if subprocess.run([cxx, *san, str(probe_src), "-o", str(tmp_path / "probe")],
                      capture_output=True).returncode:
        pytest.skip("the compiler has no sanitizer runtime")
    exe = str(tmp_path / "pack_sweep")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-pthread", *san,
                    os.path.join(ROOT, "tests", "native", "pack_sweep.cpp"),
                    os.path.join(ROOT, "spdl_amd", "csrc", "hj_pack.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe, str(tmp_path / "scratch.bin")], capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert not r.stderr, r.stderr[-4000:]
    assert r.stdout.split() == ["rounds", "50", "cases", "6"], r.stdout
