"""Frames at the format's limits, shared by the CPU tests (test_extreme.py)
and the GPU tests (test_gpu_extreme.py): one side of 32767 .. 65535 pixels,
the other of 1 .. 17, both orientations, six samplings.  Every file is a few
KB to a few hundred KB, built on demand and cached.

Encoders:
  pil / pilp  Pillow (libjpeg) at q90, baseline / progressive, from a seeded
              noise image enlarged with Image.resize.  libjpeg's
              JPEG_MAX_DIMENSION is 65500, so these stop there -- and are the
              files libjpeg itself can pin (lj_read_coefs, Pillow's luma).
  hw          tests/jpeg_writer.py from levels: a seeded DC walk, one AC level
              in about one block of eight, the standard Huffman tables.  The
              only encoder for 65501 .. 65535, and for 4:4:0 and 4:1:1 (which
              Pillow does not write).

`SOURCES` is what the CPU tests walk: every (long, short, orientation) size
with two of the six samplings, rotating, so that every sampling meets every
long side in both orientations.  `RESTART`, `MULTISCAN` and `HEADER_ONLY` are
the special layouts.  `pick(samp, tall)` is the GPU tests' one source per
(sampling, orientation).
"""

from __future__ import annotations

import functools
import io
from dataclasses import dataclass

import numpy as np

from tests import jpeg_writer as jw

LONG = (32767, 32768, 32769, 65500, 65535)
SHORT = (1, 8, 16, 17)
LIBJPEG_MAX = 65500  # JPEG_MAX_DIMENSION

SAMPLINGS = {
    "gray": [(1, 1)],
    "444": [(1, 1), (1, 1), (1, 1)],
    "422": [(2, 1), (1, 1), (1, 1)],
    "420": [(2, 2), (1, 1), (1, 1)],
    "440": [(1, 2), (1, 1), (1, 1)],
    "411": [(4, 1), (1, 1), (1, 1)],
}
# (Pillow's "4:1:1" is its old name of 4:2:0)
_PIL_SUB = {"444": "4:4:4", "422": "4:2:2", "420": "4:2:0"}


@dataclass(frozen=True)
class Source:
    name: str
    enc: str  # "pil", "pilp", "hw"
    samp: str
    w: int
    h: int
    ri: int = 0

    @property
    def tall(self) -> bool:
        return self.h > self.w

    @property
    def libjpeg(self) -> bool:
        """libjpeg (and so Pillow) reads this file."""
        return max(self.w, self.h) <= LIBJPEG_MAX

    @property
    def shifts(self) -> tuple[int, int]:
        """(hsub, vsub) of the chroma planes (0, 0 for gray)."""
        h, v = SAMPLINGS[self.samp][0]
        return h.bit_length() - 1, v.bit_length() - 1

    @property
    def nblocks(self) -> int:
        return sum(bh * bw for (bh, bw), _ in jw.block_grids(self.w, self.h, SAMPLINGS[self.samp]))


def _make(enc, samp, w, h, ri=0) -> Source:
    if enc != "hw" and (max(w, h) > LIBJPEG_MAX or samp not in _PIL_SUB and samp != "gray"):
        enc = "hw"
    if enc == "pilp" and min(w, h) < 8:
        enc = "pil"  # (Pillow sizes a progressive file's buffer by w * h: too small here)
    return Source(f"{enc}_{samp}_{w}x{h}" + (f"_ri{ri}" if ri else ""), enc, samp, w, h, ri)


def _sources():
    out, keys = [], list(SAMPLINGS)
    sizes = [(L, S) for L in LONG for S in SHORT] + [(S, L) for L in LONG for S in SHORT]
    for i, (w, h) in enumerate(sizes):
        # (LONG x SHORT is 20 sizes per orientation: i // 4 walks the long
        # sides, so i + i // 4 gives every long side every sampling)
        for k in ((i + i // 4) % 6, (i + i // 4 + 3) % 6):
            out.append(_make("pilp" if (i + k) % 2 else "pil", keys[k], w, h))
    return out


SOURCES = {s.name: s for s in _sources()}
RESTART = {s.name: s for s in (
    _make("hw", "420", 65535, 8, ri=1),
    _make("hw", "444", 17, 65535, ri=3),  # mcux = 3: one interval per MCU row
    _make("hw", "444", 65535, 72, ri=65535),  # 73728 MCUs: the largest interval ends once
)}
MULTISCAN = {s.name: s for s in (_make("pilp", "420", 65500, 8), _make("pilp", "420", 8, 65500))}
ALL = {**SOURCES, **RESTART, **MULTISCAN}
HANDWRITTEN_65535 = [n for n, s in ALL.items() if s.enc == "hw" and max(s.w, s.h) == 65535]


def pick(samp: str, tall: bool, want=lambda s: True) -> Source:
    """The GPU tests' source of one (sampling, orientation): the largest of
    `SOURCES` that `want` accepts, odd long sides first."""
    c = [s for s in SOURCES.values() if s.samp == samp and s.tall == tall and want(s)]
    return max(c, key=lambda s: (max(s.w, s.h) % 2, max(s.w, s.h), min(s.w, s.h)))


def _levels(rng, w, h, samp):
    """A DC walk folded into +-60 and one AC level (|v| <= 12, zig-zag index
    1 .. 19) in about one block of eight: nothing clamps at q <= 6."""
    out = []
    for (bh, bw), _ in jw.block_grids(w, h, samp):
        lv = np.zeros((bh, bw, 64), np.int32)
        walk = np.cumsum(rng.integers(-20, 21, size=bh * bw))
        lv[..., 0] = (np.abs((walk + 60) % 240 - 120) - 60).reshape(bh, bw)
        ys, xs = np.nonzero(rng.random((bh, bw)) < 0.125)
        lv[ys, xs, rng.integers(1, 20, size=ys.size)] = rng.integers(-12, 13, size=ys.size)
        out.append(lv)
    return out


def _seed(s: Source) -> int:
    return (s.w * 65536 + s.h) * 8 + list(SAMPLINGS).index(s.samp)


def _handwritten(s: Source):
    samp = SAMPLINGS[s.samp]
    rng = np.random.default_rng(_seed(s))
    levels = _levels(rng, s.w, s.h, samp)
    q = {i: rng.integers(1, 7, size=64) for i in (0, 1)}
    ids = [0, 1, 1][:len(samp)]
    data = jw.write_jpeg(s.w, s.h, samp, levels, q, ids, jw.std_tables(), ids, ids,
                         restart_interval=s.ri)
    return data, levels


def _pillow(s: Source) -> bytes:
    from PIL import Image

    rng = np.random.default_rng(_seed(s))
    # noise of one sample per 8 pixels, enlarged: texture in every block, and a
    # file of a few KB per thousand blocks
    sw, sh = max(1, s.w // 8), max(1, s.h // 8)
    small = rng.integers(32, 224, size=(sh, sw) if s.samp == "gray" else (sh, sw, 3), dtype=np.uint8)
    im = Image.fromarray(small, "L" if s.samp == "gray" else "RGB").resize((s.w, s.h), Image.BILINEAR)
    buf = io.BytesIO()
    kw = {} if s.samp == "gray" else {"subsampling": _PIL_SUB[s.samp]}
    im.save(buf, "JPEG", quality=90, progressive=s.enc == "pilp", **kw)
    return buf.getvalue()


@functools.lru_cache(maxsize=None)
def source(name: str) -> bytes:
    s = ALL[name]
    return _handwritten(s)[0] if s.enc == "hw" else _pillow(s)


def written_levels(name: str):
    """Per component [bh, bw, 64] in natural order: what the writer was given
    (hand-written sources only)."""
    out = []
    for lv in _handwritten(ALL[name])[1]:
        nat = np.zeros_like(lv)
        nat[..., jw.NATURAL] = lv
        out.append(nat)
    return out


@functools.lru_cache(maxsize=None)
def header_only() -> bytes:
    """A 65535 x 65535 4:4:4 baseline frame (8192 x 8192 x 3 blocks, past the
    decoder's 2^24) whose scan holds no data: the headers of an 8 x 8 file with
    the frame's size rewritten, the SOS header, EOI.  For the probe and the
    planner only -- nothing may decode it."""
    small = Source("hdr", "hw", "444", 8, 8)
    d = bytearray(_handwritten(small)[0])
    sof = d.index(b"\xff\xc0")
    d[sof + 5:sof + 9] = (65535).to_bytes(2, "big") * 2
    sos = d.index(b"\xff\xda")
    end = sos + 2 + int.from_bytes(d[sos + 2:sos + 4], "big")
    return bytes(d[:end]) + b"\xff\xd9"
