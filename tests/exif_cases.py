"""Hand-made Exif APP1 segments, for tests: the TIFF structure spelt out byte
by byte, so that every layout spdl_hj_get_orientation's rules name -- both byte
orders, the tag anywhere in IFD0, SHORT and LONG, a second Exif segment -- and
every malformed one can be put in front of one coded image with
tests/jpeg_headers.py.  Plain module: no fixtures, no decoding.
"""

from __future__ import annotations

import io

from tests import jpeg_headers as jh

ORIENTATION = 0x0112
BYTE, ASCII, SHORT, LONG = 1, 2, 3, 4
EXIF = b"Exif\x00\x00"


def entry(order: str, tag: int, typ: int, count: int, value) -> bytes:
    """One 12-byte IFD entry; ``value``: an int in the entry's type, left
    justified in the value field as TIFF has it, or the four bytes."""
    if isinstance(value, int):
        size = {BYTE: 1, ASCII: 1, SHORT: 2, LONG: 4}[typ]
        value = value.to_bytes(size, order).ljust(4, b"\x00")
    return tag.to_bytes(2, order) + typ.to_bytes(2, order) + count.to_bytes(4, order) + value


def tiff(order: str, entries, *, ifd_offset: int = 8, magic: int = 42, mark: bytes | None = None,
         count: int | None = None) -> bytes:
    """A TIFF header and IFD0 (``entries``: their 12-byte forms) at
    ``ifd_offset``; ``count``: the IFD's stated entry count, when it lies."""
    mark = mark if mark is not None else (b"II" if order == "little" else b"MM")
    head = mark + magic.to_bytes(2, order) + ifd_offset.to_bytes(4, order)
    n = len(entries) if count is None else count
    ifd = n.to_bytes(2, order) + b"".join(entries) + (0).to_bytes(4, order)
    return head + b"\x00" * max(ifd_offset - 8, 0) + ifd


def orientation(order: str, value: int, typ: int = SHORT, count: int = 1) -> bytes:
    return entry(order, ORIENTATION, typ, count, value)


def other(order: str, tag: int = 0x0100, value: int = 640) -> bytes:
    """Some other tag (ImageWidth by default)."""
    return entry(order, tag, SHORT, 1, value)


def base_jpeg() -> bytes:
    """A small coded image without any APPn segment."""
    from PIL import Image

    img = Image.new("RGB", (16, 8))
    img.putdata([(x * 16, y * 32, (x + y) * 10) for y in range(8) for x in range(16)])
    buf = io.BytesIO()
    img.save(buf, "JPEG", quality=90)
    segs, tail = jh.split(buf.getvalue())
    segs = [s for s in segs if s[0] is None or not 0xE0 <= s[0] <= 0xEF]
    return jh.join(segs, tail)


def with_app1(data: bytes, payloads) -> tuple[bytes, int, int]:
    """``data`` with the APP1 payloads right behind SOI; the file and the byte
    range [lo, hi) of those segments in it."""
    segs, tail = jh.split(data)
    new = [(jh.APP1, p) for p in payloads]
    out = jh.join(jh.edit(segs, insert=new, at=0), tail)
    return out, 2, 2 + len(jh.serialise(new))


def cases() -> list[tuple[str, list[bytes], int]]:
    """(name, APP1 payloads, the orientation the rules give)."""
    L, B = "little", "big"
    out = []
    for order, o in ((L, "ii"), (B, "mm")):
        for v in range(1, 9):
            out.append((f"{o}_short_{v}", [EXIF + tiff(order, [orientation(order, v)])], v))
        out.append((f"{o}_long_6", [EXIF + tiff(order, [orientation(order, 6, LONG)])], 6))
        out.append((f"{o}_not_first",
                    [EXIF + tiff(order, [other(order), other(order, 0x0101, 480),
                                         orientation(order, 8), other(order, 0x0128, 2)])], 8))
        out.append((f"{o}_ifd_further_in",
                    [EXIF + tiff(order, [orientation(order, 3)], ifd_offset=20)], 3))
        # ---- malformed: each is orientation 1 with return 0 ----
        out.append((f"{o}_value_0", [EXIF + tiff(order, [orientation(order, 0)])], 1))
        out.append((f"{o}_value_9", [EXIF + tiff(order, [orientation(order, 9)])], 1))
        out.append((f"{o}_long_65542", [EXIF + tiff(order, [orientation(order, 65536 + 6, LONG)])], 1))
        out.append((f"{o}_type_byte", [EXIF + tiff(order, [orientation(order, 6, BYTE)])], 1))
        out.append((f"{o}_count_2", [EXIF + tiff(order, [orientation(order, 6, SHORT, 2)])], 1))
        out.append((f"{o}_count_0", [EXIF + tiff(order, [orientation(order, 6, SHORT, 0)])], 1))
        out.append((f"{o}_magic_43", [EXIF + tiff(order, [orientation(order, 6)], magic=43)], 1))
        out.append((f"{o}_offset_outside",
                    [EXIF + tiff(order, [orientation(order, 6)])[:4] + (4000).to_bytes(4, order)
                     + tiff(order, [orientation(order, 6)])[8:]], 1))
        out.append((f"{o}_offset_at_end",
                    [EXIF + tiff(order, [])[:4] + (8).to_bytes(4, order)], 1))
        whole = EXIF + tiff(order, [other(order), orientation(order, 6)])
        out.append((f"{o}_truncated_in_entry", [whole[:6 + 8 + 2 + 12 + 7]], 1))
        out.append((f"{o}_truncated_in_count", [whole[:6 + 8 + 1]], 1))
        out.append((f"{o}_truncated_in_header", [whole[:6 + 5]], 1))
        out.append((f"{o}_count_lies",
                    [EXIF + tiff(order, [other(order)], count=40)], 1))
        out.append((f"{o}_no_tag", [EXIF + tiff(order, [other(order)])], 1))
    out.append(("mark_mixed", [EXIF + tiff(L, [orientation(L, 6)], mark=b"IM")], 1))
    out.append(("mm_mark_ii_bytes", [EXIF + tiff(L, [orientation(L, 6)], mark=b"MM")], 1))
    out.append(("no_app1", [], 1))
    out.append(("xmp_app1", [b"http://ns.adobe.com/xap/1.0/\x00<x:xmpmeta/>"], 1))
    out.append(("exif_prefix_short", [b"Exif\x00"], 1))
    out.append(("exif_one_nul", [b"Exif\x00\x01" + tiff(L, [orientation(L, 6)])], 1))
    # the first Exif APP1 wins -- over a second one, and behind an XMP one
    out.append(("second_exif", [EXIF + tiff(L, [orientation(L, 6)]),
                                EXIF + tiff(B, [orientation(B, 3)])], 6))
    out.append(("first_exif_without_tag", [EXIF + tiff(L, [other(L)]),
                                           EXIF + tiff(B, [orientation(B, 3)])], 1))
    out.append(("xmp_then_exif", [b"http://ns.adobe.com/xap/1.0/\x00<x/>",
                                  EXIF + tiff(B, [orientation(B, 8)])], 8))
    return out
