"""Streams for tests/test_gpu_destuff.py, written with tests/jpeg_writer.py:
scans a little over two destuff chunks (2 x 4096 bytes) whose stuffed pairs,
restart markers and fill bytes can be moved over every boundary of the
destuff kernels -- the 16-byte group of a thread and the 4096-byte chunk of a
workgroup -- by padding a COM segment after SOI (chunks start at
scan_start & ~15, so scan_start % 16 is the only thing that moves them).
"""

from __future__ import annotations

import functools

import numpy as np

from tests import jpeg_writer as jw
from tests import jpeg_writer_cases as hw

CHUNK = 4096
GROUP = 16


def scan_extent(data: bytes) -> tuple[int, int]:
    """(first scan byte, position of the EOI marker's 0xFF) of a one-scan file."""
    p = 2
    while True:
        assert data[p] == 0xFF, p
        m, n = data[p + 1], int.from_bytes(data[p + 2:p + 4], "big")
        p += 2 + n
        if m == 0xDA:
            break
    assert data[-2:] == b"\xff\xd9"
    return p, len(data) - 2


def aligned(data: bytes, k: int) -> bytes:
    """`data` with a COM segment after SOI sized so that scan_start % 16 == k."""
    s0, _ = scan_extent(data)
    out = data[:2] + jw._seg(0xFE, b"." * ((k - s0 - 4) % 16)) + data[2:]
    assert scan_extent(out)[0] % 16 == k
    return out


def chunk_pos(data: bytes, j: int) -> int:
    """Offset of file byte j in its destuff chunk."""
    s, _ = scan_extent(data)
    return (j - (s & ~15)) % CHUNK


def _gray(name, w, h, seed, **kw) -> hw.Stream:
    rng = np.random.default_rng(seed)
    levels = hw.moderate_levels(rng, hw._grid_shapes(w, h, [(1, 1)]))
    return hw._write(name, w, h, [(1, 1)], levels, hw._small_q(rng, (0,)), [0], jw.std_tables(),
                     [0], [0], **kw)


@functools.lru_cache(maxsize=None)
def case(name: str) -> hw.Stream:
    if name == "stuffed":  # 8-9 KB of ordinary entropy-coded data, some 500 stuffed pairs
        return _gray(name, 200, 200, 13)
    if name == "rst_every_block":  # an RSTn every 10 bytes or so
        return _gray(name, 184, 184, 13, restart_interval=1)
    if name == "rst_fill":  # 0xFF 0xFF 0xFF 0xFF RSTn
        return _gray(name, 184, 176, 13, restart_interval=2, rst_fill=3)
    if name == "all_ones":
        # every block two 1-bits: every scan byte 0xFF and stuffed, eight drops
        # in every group, 0xFF 0x00 directly before EOI; 130 x 128 blocks
        lv = np.zeros((128, 130, 64), np.int32)
        return hw._write(name, 1040, 1024, [(1, 1)], [lv], {0: np.full(64, 4)}, [0],
                         jw.short_table(inverted=True), [0], [0])
    raise KeyError(name)


NAMES = ("stuffed", "rst_every_block", "rst_fill", "all_ones")
