#!/usr/bin/env python3
"""Digests of a --save-temps assembly listing, to compare two builds.

    make -C spdl_amd/csrc asm
    python tools/isa_digest.py spdl_amd/lib/asm/hj_kernels-hip-amdgcn-amd-amdhsa-gfx950.s

Prints a sha256 of every function in the listing (its `.type NAME,@function`
line to its `.size NAME,` line: the code and, for a kernel, its descriptor)
and one of the whole file.  Takes the device listing or the host one.

What is not code is taken out first, so that two sources which differ only
in text the compiler drops give equal digests:
  - the compilation-unit id (__hip_cuid_<hex>, a hash of the source text;
    the host side names its module handle after it), replaced by a fixed word;
  - comments: they name basic blocks after the inlined functions' signatures
    and the compiler's value numbers;
  - in a host listing, the embedded device bundle: it is the linked code
    object, whose symbol hash tables are ordered by the id's name.  The device
    code is compared by its own listing.
"""
import hashlib
import re
import sys


def normalise(text):
    m = re.search(r"__hip_cuid_([0-9a-f]+)", text)
    if m:
        text = text.replace(m.group(1), "CUID")
    text = re.sub(r'(?m)^\s*\.asciz\s+"__CLANG_OFFLOAD_BUNDLE__.*$', "\t.asciz\tBUNDLE", text)
    # (a line that holds a string keeps its comment: the mark may be in the string)
    return re.sub(r'(?m)^([^"\n]*?)[ \t]*[;#][^"\n]*$', r"\1", text)


def digests(text):
    text = normalise(text)
    out, name, body = [], None, []
    for line in text.splitlines(keepends=True):
        m = re.match(r"\s*\.type\s+(\S+),@function", line)
        if m and name is None:
            name, body = m.group(1), []
        if name is not None:
            body.append(line)
            if re.match(r"\s*\.size\s+" + re.escape(name) + ",", line):
                out.append((name, hashlib.sha256("".join(body).encode()).hexdigest()))
                name = None
    return out, hashlib.sha256(text.encode()).hexdigest()


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    with open(sys.argv[1], encoding="latin-1") as f:
        funcs, whole = digests(f.read())
    for name, h in funcs:
        print(h, name)
    print(whole, "(whole file, %d functions)" % len(funcs))


if __name__ == "__main__":
    main()
