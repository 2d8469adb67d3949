"""CPU tests of the batch planner (spdl_amd/csrc/hj_layout.cpp, no GPU): the
descriptors, table pool and work list it makes of a fixed table of
submissions, byte for byte against tests/golden/layout_dump.txt -- the lines
the planner printed while it still lived inside hj_host.cpp -- as a
stand-alone program under ASan and UBSan.

Reading a failure: the first differing line names its case
(tests/native/layout_dump.cpp).  A differing rc / err / status is a changed
rule; a differing scalar or hash with the same rc is a changed byte on its way
to the device.  The golden changes only with a change that means to alter
those bytes (a new descriptor field, say), and then for every case at once.
"""

import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spdl_amd", "csrc")
DUMP = os.path.join(ROOT, "tests", "native", "layout_dump.cpp")
GOLDEN = os.path.join(ROOT, "tests", "golden", "layout_dump.txt")
HIP_INCLUDE = re.compile(r'#\s*include\s*[<"](hip/|hj_launch\.h|hj_probe\.h)')


def test_layout_matches_golden_under_sanitizers(tmp_path):
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
    exe = str(tmp_path / "layout_dump")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-DHJ_HD=", *san, DUMP,
                    os.path.join(CSRC, "hj_layout.cpp"), os.path.join(CSRC, "hj_sws.cpp"),
                    "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    assert not r.stderr, r.stderr
    got, want = r.stdout.splitlines(), open(GOLDEN).read().splitlines()
    for g, w in zip(got, want):
        assert g == w, f"case {w.split(' ', 1)[0]}:\n  got  {g}\n  want {w}"
    assert len(got) == len(want), f"{len(got)} cases printed, {len(want)} in the golden"
    assert len(want) >= 100


def test_planner_includes_no_hip_header():
    """hj_layout.h / .cpp stay free of HIP (and of the headers that pull it
    in), and the dump program sees the planner through hj_layout.h alone.
    The same holds for the other two host-only units, the tar walk and the
    staging copier, which include nothing of the project but their own header;
    and the kernels' file includes neither."""
    planner = {"../../include/spdl_hipjpeg.h", "hj_common.h", "hj_sws.h", "hj_sws_tile.h",
               "hj_views.h", "hj_layout.h"}
    allowed = {"hj_layout.h": planner, "hj_layout.cpp": planner,
               "hj_tar.h": set(), "hj_tar.cpp": {"hj_tar.h"},
               "hj_pack.h": set(), "hj_pack.cpp": {"hj_pack.h"}}
    for name, ok in allowed.items():
        src = open(os.path.join(CSRC, name)).read()
        assert not HIP_INCLUDE.search(src), name
        assert set(re.findall(r'#\s*include\s*"([^"]+)"', src)) <= ok, name
    kernels = open(os.path.join(CSRC, "hj_kernels.hip")).read()
    assert not re.search(r'#\s*include\s*"hj_(tar|pack)\.h"', kernels)
    src = open(DUMP).read()
    assert re.findall(r'#\s*include\s*"([^"]+)"', src) == ["../../spdl_amd/csrc/hj_layout.h"]
    assert not HIP_INCLUDE.search(src)


def test_no_ab_switch_in_the_native_sources():
    """The only HJ_* names a preprocessor conditional of spdl_amd/csrc may test
    are the host / device qualifier, the IDCT header's guard and the
    diagnostic builds (instruments that bench.py, tools/ and the tests use)."""
    allowed = {"HJ_HD", "HJ_DC_BIAS_DEFINED", "HJ_ABLATIONS", "HJ_OWN_CHECK", "HJ_PARSE_PROF",
               "HJ_MS_PROF", "HJ_MS_COUNT", "HJ_MS_COUNT2"}
    found = set()
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".hip", ".h", ".cpp")):
            for line in open(os.path.join(CSRC, name)):
                if re.match(r"\s*#\s*(if|ifdef|ifndef|elif)\b", line):
                    found |= set(re.findall(r"\bHJ_\w+", line))
    assert found == allowed, (
        f"conditionals on {sorted(found - allowed)} added, on {sorted(allowed - found)} gone: "
        "an A/B switch does not stay in the tree -- decide it, record the measurement under "
        "profiles/ and remove the switch with the losing arm")
