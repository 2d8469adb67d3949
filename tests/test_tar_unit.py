"""CPU tests of the tar member walk as a unit (spdl_amd/csrc/hj_tar.cpp, no
HIP): tests/native/tar_sweep.cpp under ASan and UBSan against Python's
``tarfile`` on ustar, GNU and pax archives, then on every truncation of them,
with names buffers too small for a name, and from a start past the end.
tests/test_tar.py keeps testing the same walk through the library.
"""

import io
import os
import shutil
import subprocess
import tarfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spdl_amd", "csrc")
FORMATS = {"ustar": tarfile.USTAR_FORMAT, "gnu": tarfile.GNU_FORMAT, "pax": tarfile.PAX_FORMAT}
# 150 characters: past the 100-byte name field (ustar splits it at the slash
# into prefix and name; GNU writes an 'L' record, pax an 'x' path record)
LONG = "p" * 60 + "/" + "n" * 85 + ".jpg"
ENTRIES = [
    ("a.jpg", b"x" * 100),
    ("dir", None),
    ("dir/b.jpg", bytes(range(256)) * 4),  # exactly 1024 bytes: no padding
    ("link", "a.jpg"),
    ("empty.txt", b""),
    (LONG, b"\xff\xd8" + b"\x01" * 700),
    ("c/d/e.bin", b"\xff\xd8" + b"\x00" * 511),  # 513 bytes
]


def _make_tar(fmt) -> bytes:
    b = io.BytesIO()
    with tarfile.open(fileobj=b, mode="w", format=fmt) as t:
        for name, data in ENTRIES:
            ti = tarfile.TarInfo(name)
            if data is None:
                ti.type = tarfile.DIRTYPE
                t.addfile(ti)
            elif isinstance(data, str):
                ti.type = tarfile.SYMTYPE
                ti.linkname = data
                t.addfile(ti)
            else:
                ti.size = len(data)
                t.addfile(ti, io.BytesIO(data))
    return b.getvalue()


def _ref(data: bytes):
    """tarfile's own view: (payload offset, size, name) of the regular files."""
    with tarfile.open(fileobj=io.BytesIO(data)) as t:
        return [(m.offset_data, m.size, m.name) for m in t.getmembers() if m.isfile()]


@pytest.fixture(scope="module")
def tar_sweep(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    tmp = tmp_path_factory.mktemp("tar_sweep")
    # (runtimes linked statically: the program then runs whatever the environment preloads)
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
           "-static-libubsan"]
    probe_src = tmp / "probe.cpp"
    probe_src.write_text("int main() { return 0; }\n")
    if subprocess.run([cxx, *san, str(probe_src), "-o", str(tmp / "probe")],
                      capture_output=True).returncode:
        pytest.skip("the compiler has no sanitizer runtime")
    exe = str(tmp / "tar_sweep")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", *san,
                    os.path.join(ROOT, "tests", "native", "tar_sweep.cpp"),
                    os.path.join(CSRC, "hj_tar.cpp"), "-o", exe], check=True)

    def run(path, *args):
        r = subprocess.run([exe, str(path), *map(str, args)], capture_output=True, text=True,
                           timeout=120)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr
        assert not r.stderr, r.stderr
        return r.stdout.splitlines()

    return run


def _members(lines):
    """([(offset, size, name)], next_pos) of one walk's lines."""
    assert lines and lines[-1].startswith("next_pos "), lines
    out = []
    for ln in lines[:-1]:
        off, size, name = ln.split(" ", 2)
        out.append((int(off), int(size), name))
    return out, int(lines[-1].split()[1])


@pytest.fixture(scope="module", params=sorted(FORMATS))
def archive(request, tmp_path_factory):
    data = _make_tar(FORMATS[request.param])
    path = tmp_path_factory.mktemp("tar") / f"{request.param}.tar"
    path.write_bytes(data)
    return path, data


def test_members_match_tarfile(tar_sweep, archive):
    path, data = archive
    want = _ref(data)
    assert [n for _, _, n in want] == [n for n, d in ENTRIES if isinstance(d, bytes)]
    got, next_pos = _members(tar_sweep(path))
    assert got == want
    assert next_pos == len(data)
    for (off, size, name), (_, payload) in zip(got, [e for e in ENTRIES
                                                     if isinstance(e[1], bytes)]):
        assert data[off:off + size] == payload, name


def test_every_truncation_stays_inside_the_buffer(tar_sweep, archive):
    path, data = archive
    want = _ref(data)
    lines = tar_sweep(path, "--truncate")
    limits, walks = [], []
    for ln in lines:
        if ln.startswith("limit "):
            limits.append(int(ln.split()[1]))
            walks.append([])
        else:
            walks[-1].append(ln)
    expect = sorted({n for m in range(0, len(data) + 2, 512) for n in (m - 1, m, m + 1)
                     if 0 <= n <= len(data)})
    assert limits == expect
    for limit, w in zip(limits, walks):
        got, next_pos = _members(w)
        assert all(off + size <= limit for off, size, _ in got), (limit, got)
        # (the walk moves in whole blocks: past a last member's padding it may
        # stand up to 511 bytes behind a cut that spared the payload)
        assert next_pos <= -(-limit // 512) * 512
        # what a truncated archive still shows are the first members of the whole one
        assert got == want[:len(got)], limit
    assert _members(walks[-1])[0] == want


@pytest.mark.parametrize("cap", [1, 16, 64])
def test_a_small_names_buffer_resumes_at_the_entry(tar_sweep, archive, cap):
    """A name that does not fit ends the call before its entry, which the
    next call takes up with an empty buffer; one that never fits (the
    150-character name, or any name in a 1-byte buffer) ends the walk there."""
    path, data = archive
    want = _ref(data)
    got, next_pos = _members(tar_sweep(path, "--cap", cap))
    fit = 0
    while fit < len(want) and len(want[fit][2]) + 1 <= cap:
        fit += 1
    assert got == want[:fit]
    assert next_pos <= len(data)
    assert all(off + size <= len(data) for off, size, _ in got)


def test_a_start_past_the_end_finds_nothing(tar_sweep, archive):
    path, data = archive
    for start in (len(data), len(data) + 1, len(data) + 5000):
        got, next_pos = _members(tar_sweep(path, "--start", start))
        assert got == [] and next_pos == len(data)
