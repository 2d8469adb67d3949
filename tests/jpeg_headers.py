"""Segment editor for JPEG headers, for tests: a file taken apart into its
marker segments, edited as a list and put together again, so that any header
layout an encoder might write (segment order, tables defined twice, fill
bytes, metadata in front of, between and behind the tables) can be made from
one coded image without touching its scan.

A file is SOI, segments, the first SOS, and a tail (the first scan's
entropy-coded bytes and all that follows, EOI included).  `split` returns the
segments up to and including that SOS and the tail; `split_tail` goes on
through the tail of a multi-scan file.  A segment is `(marker, payload)`:

  (0xDB, b"...")   a marker segment; the length field is made by `join`
  (0xD0, None)     a stand-alone marker (TEM, RSTn, EOI): no length, no payload
  (None, b"...")   raw bytes between two segments (garbage, entropy-coded data)

Works on the streams of tests/jpeg_writer.py and on encoder-made files alike.
Plain module: no fixtures, no decoding.
"""

from __future__ import annotations

SOI, EOI, SOS, DQT, DHT, DRI, COM, TEM = 0xD8, 0xD9, 0xDA, 0xDB, 0xC4, 0xDD, 0xFE, 0x01
SOF0, SOF1, SOF2 = 0xC0, 0xC1, 0xC2
APP0, APP1, APP2, APP14 = 0xE0, 0xE1, 0xE2, 0xEE
SOFS = (SOF0, SOF1, SOF2)


def _standalone(m: int) -> bool:
    return m == TEM or 0xD0 <= m <= 0xD9


def split(data: bytes):
    """([(marker, payload), ...] up to and including the first SOS, tail)."""
    assert data[:2] == b"\xff\xd8", "no SOI"
    segs, pos = [], 2
    while True:
        assert data[pos] == 0xFF, f"no marker at {pos}"
        while data[pos + 1] == 0xFF:  # fill bytes
            pos += 1
        m = data[pos + 1]
        if _standalone(m):
            segs.append((m, None))
            pos += 2
            continue
        n = int.from_bytes(data[pos + 2:pos + 4], "big")
        assert n >= 2 and pos + 2 + n <= len(data), f"segment at {pos} runs past the file"
        segs.append((m, bytes(data[pos + 4:pos + 2 + n])))
        pos += 2 + n
        if m == SOS:
            return segs, bytes(data[pos:])


def scan_end(data: bytes, pos: int = 0) -> int:
    """The offset of the first marker in entropy-coded bytes from `pos` on:
    0xFF followed by anything but 0x00, a fill 0xFF or RSTn."""
    while True:
        pos = data.find(b"\xff", pos)
        if pos < 0 or pos + 1 >= len(data):
            return len(data)
        nx = data[pos + 1]
        if nx == 0x00 or 0xD0 <= nx <= 0xD7:
            pos += 2
        elif nx == 0xFF:
            pos += 1
        else:
            return pos


def split_tail(tail: bytes):
    """The tail as items: (None, entropy-coded bytes) after every SOS, the
    segments between the scans, (EOI, None), and (None, bytes) for whatever
    follows EOI."""
    items, pos = [], 0
    while pos < len(tail):
        end = scan_end(tail, pos)
        items.append((None, bytes(tail[pos:end])))
        pos = end
        while pos < len(tail):
            m = tail[pos + 1]
            if m == EOI:
                items.append((EOI, None))
                if pos + 2 < len(tail):
                    items.append((None, bytes(tail[pos + 2:])))
                return items
            if _standalone(m):
                items.append((m, None))
                pos += 2
                continue
            n = int.from_bytes(tail[pos + 2:pos + 4], "big")
            items.append((m, bytes(tail[pos + 4:pos + 2 + n])))
            pos += 2 + n
            if m == SOS:
                break
    return items


def serialise(segments, fill=0, only=None) -> bytes:
    """The segments as bytes (no SOI).  `fill`: extra 0xFF bytes in front of
    each marker -- of every kind, or of the kinds in `only`."""
    out = bytearray()
    for m, payload in segments:
        if m is None:
            out += payload
            continue
        out += b"\xff" * (fill if only is None or m in only else 0) + bytes([0xFF, m])
        if payload is not None:
            assert len(payload) <= 65533, "a segment holds at most 65533 payload bytes"
            out += (len(payload) + 2).to_bytes(2, "big") + payload
    return bytes(out)


def join(segments, tail: bytes, fill=0, only=None) -> bytes:
    """SOI, the segments, the tail."""
    return b"\xff\xd8" + serialise(segments, fill, only) + bytes(tail)


# ---- editing ----------------------------------------------------------------

def index(segments, marker, nth=0) -> int:
    """The position of the nth segment of kind `marker` (a marker or a tuple
    of markers); nth = -1: the last."""
    kinds = marker if isinstance(marker, tuple) else (marker,)
    found = [i for i, (m, _) in enumerate(segments) if m in kinds]
    assert found, f"no segment {marker}"
    return found[nth]


def edit(segments, *, drop=None, insert=None, before=None, after=None, at=None, move=None,
         replace=None, nth=0):
    """A copy of the list with one change:
      drop=marker                      without the nth such segment
      insert=[segs], before=marker     (or after=marker; or at=position in the list)
      move=marker, before=marker       the nth `move` segment taken out and put there
      replace=marker, insert=[segs]    the nth such segment replaced by the new ones
    """
    segs = list(segments)
    new = list(insert or [])
    if move is not None:
        new = [segs.pop(index(segs, move, nth))]
        nth = 0
    if drop is not None:
        del segs[index(segs, drop, nth)]
        return segs
    if replace is not None:
        i = index(segs, replace, nth)
        return segs[:i] + new + segs[i + 1:]
    if at is not None:
        i = at
    elif before is not None:
        i = index(segs, before, 0 if move is not None else nth)
    else:
        assert after is not None
        i = index(segs, after, -1 if move is not None else nth) + 1
    return segs[:i] + new + segs[i:]


def payload(segments, marker, nth=0) -> bytes:
    return segments[index(segments, marker, nth)][1]


def patch(segments, marker, offset: int, value, nth=0):
    """The nth `marker` segment with payload byte(s) at `offset` overwritten."""
    value = bytes([value]) if isinstance(value, int) else bytes(value)
    i = index(segments, marker, nth)
    p = bytearray(segments[i][1])
    p[offset:offset + len(value)] = value
    return list(segments[:i]) + [(marker, bytes(p))] + list(segments[i + 1:])


# ---- table payloads ---------------------------------------------------------

def dqt_tables(payload_: bytes) -> list[bytes]:
    """A DQT payload as its tables (Pq/Tq byte + 64 or 128 bytes each)."""
    out, p = [], 0
    while p < len(payload_):
        n = 1 + 64 * ((payload_[p] >> 4) + 1)
        out.append(payload_[p:p + n])
        p += n
    return out


def dht_tables(payload_: bytes) -> list[bytes]:
    """A DHT payload as its tables (Tc/Th byte, 16 counts, the symbols)."""
    out, p = [], 0
    while p < len(payload_):
        n = 17 + sum(payload_[p + 1:p + 17])
        out.append(payload_[p:p + n])
        p += n
    return out


def all_tables(segments, marker) -> list[bytes]:
    """Every table of every `marker` (DQT or DHT) segment, in file order."""
    cut = dqt_tables if marker == DQT else dht_tables
    return [t for m, p in segments if m == marker for t in cut(p)]


def without(segments, marker):
    return [s for s in segments if s[0] != marker]


def dqt_as(table: bytes, pq: int, tq: int | None = None) -> bytes:
    """One DQT table rewritten at precision `pq` (its values must fit)."""
    tq = table[0] & 15 if tq is None else tq
    if table[0] >> 4:
        vals = [int.from_bytes(table[1 + 2 * i:3 + 2 * i], "big") for i in range(64)]
    else:
        vals = list(table[1:65])
    if pq:
        return bytes([0x10 | tq]) + b"".join(v.to_bytes(2, "big") for v in vals)
    assert max(vals) < 256
    return bytes([tq]) + bytes(vals)
