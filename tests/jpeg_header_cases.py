"""Header-structure cases: one coded image, many headers (tests/jpeg_headers.py
edits the segments; tests/jpeg_writer.py writes the sources).  Shared by the
CPU tests (test_jpeg_headers.py: the oracle against libjpeg 9 and Pillow, the
host probe against the oracle, the sanitised native sweep) and the GPU parity
tests (test_gpu_headers.py).

A case is (source, edited bytes, expected class):

  "same"     decodes to exactly what the unedited source decodes to: levels,
             dequantised coefficients and RGB (`reordered`: the scan lists the
             components in another order, so the MCU-order coefficients are
             not compared)
  "ok"       decodes, to something else than the source (`other`, where set,
             is the stream a decoder that took the wrong table would have
             decoded: the case must differ from it)
  "oracle"   whatever the oracle does (the three "ends" cases)
  an int     the status both sides return (SPDL_HJ_ERR_* == JO_ERR_*)

Sources are the smallest frames that still have every table: 16x16 and 24x16
from jpeg_writer_cases.moderate_levels (4:2:0, 4:4:4, gray, 4-component Adobe;
baseline, "spectral" and "per_component" scans), and the committed q90_420 and
prog_420 for real encoder tables.

REFUSED is keyed by the source text of the condition in parse_headers (and in
multiscan_kernel's marker walk, "ms:") that refuses the case, so the rows can
be ticked off against spdl_amd/csrc/hj_kernels.hip.
"""

from __future__ import annotations

import functools
import os
from dataclasses import dataclass

import numpy as np

from tests import jpeg_headers as jh
from tests import jpeg_writer as jw
from tests import jpeg_writer_cases as hw

NOT_JPEG, UNSUPPORTED, BAD_HEADER, BAD_HUFFMAN, TRUNCATED, BAD_RESTART = 1, 2, 3, 4, 5, 6
GOLD_JPEG = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg")

S420 = [(2, 2), (1, 1), (1, 1)]
S444 = [(1, 1)] * 3


@dataclass(frozen=True)
class Case:
    name: str
    source: str          # key of SOURCES
    data: bytes
    expect: object       # "same" | "ok" | "oracle" | status
    family: str
    key: str = ""        # refused: the refusing condition's source text
    other: bytes | None = None
    reordered: bool = False
    libjpeg: bool = True  # legal: libjpeg 9 reads it (False: the oracle alone pins it)
    pillow: bool = True
    probe: int = 0       # refused: what the host probe returns (0: it cannot see the fault)
    layout: bool = False  # refused: the probe accepts the frame, the host's batch layout does not


# ---- sources ----------------------------------------------------------------

def _levels(seed, w, h, samp, own_only=False):
    rng = np.random.default_rng(seed)
    grids = jw.block_grids(w, h, samp)
    levels = hw.moderate_levels(rng, [g[0] for g in grids])
    if own_only:  # non-interleaved scans code the component's own grid
        for lv, (_, own) in zip(levels, grids):
            lv[own[0]:] = 0
            lv[:, own[1]:] = 0
    return levels, {0: rng.integers(1, 7, size=64), 1: rng.integers(1, 7, size=64)}


def _ids(nc):
    return [0, 1, 1, 0][:nc]


def _write(w, h, samp, seed=7, own_only=False, q=None, levels=None, tq=None, dht=None, td=None,
           ta=None, **kw) -> bytes:
    lv, q0 = _levels(seed, w, h, samp, own_only or kw.get("scans") in ("spectral", "per_component",
                                                                       "script"))
    ids = _ids(len(samp))
    return jw.write_jpeg(w, h, samp, lv if levels is None else levels, q0 if q is None else q,
                         ids if tq is None else tq, jw.std_tables() if dht is None else dht,
                         ids if td is None else td, ids if ta is None else ta, **kw)


def _gold(name) -> bytes:
    with open(os.path.join(GOLD_JPEG, name + ".jpg"), "rb") as f:
        return f.read()


@functools.lru_cache(maxsize=None)
def source(name: str) -> bytes:
    if name == "b420":       # baseline 4:2:0, two MCUs, a restart between them
        return _write(24, 16, S420, restart_interval=1)
    if name == "b420n":      # no restarts, DRI 0 written
        return _write(24, 16, S420, emit_dri=True)
    if name == "b444":
        return _write(16, 16, S444, seed=8, emit_dri=True)
    if name == "gray":
        return _write(16, 16, [(1, 1)], seed=9, emit_dri=True)
    if name == "ycck":       # 4 components, Adobe transform 2
        return _write(16, 16, [(1, 1)] * 4, seed=10, adobe=2, emit_dri=True)
    if name == "sp420":      # SOF2, a DC scan and two AC bands per component, restarts
        return _write(24, 16, S420, scans="spectral", restart_interval=1)
    if name == "sp420n":
        return _write(24, 16, S420, scans="spectral")
    if name == "pc420":      # SOF0, one scan per component
        return _write(24, 16, S420, scans="per_component", restart_interval=2)
    if name == "pcycck":
        return _write(16, 16, [(1, 1)] * 4, seed=10, own_only=True, adobe=2, scans="per_component")
    if name == "win":        # the LDS-window source: single table segments, a Pq 1 table, APP14
        d = _write(24, 16, S420, restart_interval=1, pq=1, table_segments="single", adobe=1)
        segs, tail = jh.split(d)
        i = jh.index(segs, jh.DQT, 1)  # the second table at 8 bits: both precisions in one file
        segs[i] = (jh.DQT, jh.dqt_as(segs[i][1], 0))
        return jh.join(segs, tail)
    if name == "sc420":      # SOF2 by a scan script: DC, then one AC scan per component
        return _script420(False)
    if name == "nh":         # the nh-edge source: 13 bytes from its last table to the end
        return _nh_source()
    if name in ("q90_420", "prog_420"):
        return _gold(name)
    raise KeyError(name)


def _script420(replaced: bool) -> bytes:
    """replaced: a DHT in front of the third scan redefines AC 1 (the chroma
    scans then use it) in one segment with AC 3, which no scan uses."""
    lv, q = _levels(7, 24, 16, S420, True)
    more = {"dht": {("ac", 3): jw.flat_table(jw.AC_SYMBOLS), ("ac", 1): jw.deep_table(jw.AC_SYMBOLS)}}
    script = [([0, 1, 2], 0, 0, 0, 0), ([0], 1, 63, 0, 0),
              ([1], 1, 63, 0, 0, more) if replaced else ([1], 1, 63, 0, 0), ([2], 1, 63, 0, 0)]
    ids = _ids(3)
    return jw.write_jpeg(24, 16, S420, lv, q, ids, jw.std_tables(), ids, ids, scans="script",
                         script=script)


def _nh_source() -> bytes:
    """Gray 8x8, one block with a DC level alone; the DC table is the last
    segment before SOS and the symbol the block uses is its last value: SOS
    (10 bytes), the scan (2) and EOI (2) are 14 bytes, so the 15 bytes that
    size & ~15 can leave out of the LDS window reach that value."""
    lv = [np.zeros((1, 1, 64), np.int32)]
    lv[0][0, 0, 0] = 5
    dht = {("ac", 0): jw.std_tables()[("ac", 0)],
           ("dc", 0): jw.flat_table(list(range(12))[::-1][:-4] + [0, 1, 2, 3], 4)}
    assert dht[("dc", 0)][1][-1] == 3  # category 3: the DC difference 5
    d = jw.write_jpeg(8, 8, [(1, 1)], lv, {0: np.arange(2, 66)}, [0], dht, [0], [0],
                      table_segments="single")
    segs, tail = jh.split(d)
    segs = jh.edit(segs, move=jh.DHT, before=jh.SOS)  # (DC 0 is written first: now the last)
    assert segs[-2][1][0] == 0x00 and len(tail) == 4
    return jh.join(segs, tail)


BASELINE = ["b420", "b420n", "b444", "gray", "ycck", "q90_420", "win", "nh"]
MULTISCAN = ["sp420", "sp420n", "pc420", "pcycck", "sc420", "prog_420"]
SOURCES = BASELINE + MULTISCAN

_cases: dict[str, Case] = {}


def _add(name, src, data, expect, family, **kw):
    assert name not in _cases, name
    _cases[name] = Case(name, src, bytes(data), expect, family, **kw)


def _seg(marker, payload=b""):
    return (marker, bytes(payload))


def _thumbnail() -> bytes:
    """A complete small JPEG of other dimensions (8x8 gray) to embed."""
    return _write(8, 8, [(1, 1)], seed=11)


def _ff_blob(seed: int, n: int) -> bytes:
    """n bytes, every other one 0xFF followed by a byte that would read as a
    marker outside a segment (as tests/cases._ff_blob)."""
    rng = np.random.default_rng(seed)
    nx = rng.choice(np.array([0xC0, 0xC2, 0xC4, 0xD9, 0xDA, 0xDB, 0xE1], np.uint8), size=n // 2)
    out = np.empty(2 * (n // 2), np.uint8)
    out[0::2] = 0xFF
    out[1::2] = nx
    return out.tobytes()


def _adobe(transform, n=12):
    return _seg(jh.APP14, (b"Adobe" + bytes([0, 100, 0, 0, 0, 0, transform]))[:n])


def _between_scans(tail: bytes, new, which=1, fill=0) -> bytes:
    """The tail with segments put in front of the which-th later SOS
    (1 = the second scan's; -1: in front of EOI, after the last scan)."""
    items = jh.split_tail(tail)
    if which == -1:
        i = max(k for k, (m, _) in enumerate(items) if m == jh.EOI)
    else:
        i = [k for k, (m, _) in enumerate(items) if m == jh.SOS][which - 1]
        while i > 0 and items[i - 1][0] is not None:  # ahead of that scan's own tables
            i -= 1
    return jh.serialise(items[:i] + list(new) + items[i:], fill)


# ---- legal layouts ----------------------------------------------------------

def _order():
    for src in ("b420", "b444", "ycck", "sp420", "pc420"):
        segs, tail = jh.split(source(src))
        fam = "order"
        _add(f"order_dht_before_dqt_{src}", src,
             jh.join(jh.edit(segs, move=jh.DHT, before=jh.DQT), tail), "same", fam)
        _add(f"order_dqt_after_sof_{src}", src,
             jh.join(jh.edit(segs, move=jh.DQT, after=jh.SOFS), tail), "same", fam)
        _add(f"order_dri_before_sof_{src}", src,
             jh.join(jh.edit(segs, move=jh.DRI, before=jh.SOFS), tail), "same", fam)
        _add(f"order_dri_first_{src}", src, jh.join(jh.edit(segs, move=jh.DRI, at=0), tail),
             "same", fam)
        # DRI as the last segment before SOS, the tables behind the SOF in
        # front of it: SOF, DHT, DQT, DRI, SOS
        s2 = jh.edit(jh.edit(segs, move=jh.DRI, before=jh.SOS), move=jh.DQT, before=jh.DRI)
        _add(f"order_dri_last_{src}", src, jh.join(s2, tail), "same", fam)
        # every table in its own segment, in reverse id order
        dq = [_seg(jh.DQT, t) for t in reversed(jh.all_tables(segs, jh.DQT))]
        dh = [_seg(jh.DHT, t) for t in reversed(jh.all_tables(segs, jh.DHT))]
        s3 = jh.edit(jh.edit(segs, replace=jh.DQT, insert=dq), replace=jh.DHT, insert=dh)
        _add(f"order_single_reversed_{src}", src, jh.join(s3, tail), "same", fam)
    for src in ("q90_420", "prog_420"):  # an encoder's layout: DQT DQT SOF DHT x4 SOS
        segs, tail = jh.split(source(src))
        dq = [_seg(jh.DQT, t) for t in reversed(jh.all_tables(segs, jh.DQT))]
        dh = [_seg(jh.DHT, b"".join(reversed(jh.all_tables(segs, jh.DHT))))]
        rest = [s for s in segs if s[0] not in (jh.DQT, jh.DHT, jh.SOS)]
        _add(f"order_dht_first_merged_{src}", src,
             jh.join(dh + rest + dq + [segs[-1]], tail), "same", "order")


def _redefine():
    fam = "redefine"
    for src in ("b420", "sp420", "q90_420"):
        segs, tail = jh.split(source(src))
        tabs = jh.all_tables(segs, jh.DQT)
        t0 = next(t for t in tabs if t[0] & 15 == 0)
        # a different, valid table for id 0 (every entry + 1), at 8 bits
        vals = [min(v + 1, 255) for v in jh.dqt_as(t0, 0)[1:]]
        wrong = bytes([0]) + bytes(vals)
        right = jh.dqt_as(t0, 0)
        first = jh.index(segs, jh.DQT)
        last = jh.index(segs, jh.DQT, -1) + 1
        good = jh.join(segs[:first] + [_seg(jh.DQT, wrong)] + segs[first:], tail)
        bad = jh.join(segs[:last] + [_seg(jh.DQT, wrong)] + segs[last:], tail)
        _add(f"redef_dqt_later_wins_{src}", src, good, "same", fam, other=bad)
        _add(f"redef_dqt_other_table_{src}", src, bad, "ok", fam, other=source(src))
        # the same id at both precisions: Pq 1 (other values) then Pq 0, and the reverse
        _add(f"redef_dqt_pq1_then_pq0_{src}", src,
             jh.join(segs[:first] + [_seg(jh.DQT, jh.dqt_as(wrong, 1))] + segs[first:last]
                     + [_seg(jh.DQT, right)] + segs[last:], tail), "same", fam)
        _add(f"redef_dqt_pq0_then_pq1_{src}", src,
             jh.join(segs[:first] + [_seg(jh.DQT, wrong)] + segs[first:last]
                     + [_seg(jh.DQT, jh.dqt_as(right, 1))] + segs[last:], tail), "same", fam)
        # a Huffman slot defined twice: AC 0 first as the table of AC 1
        hts = jh.all_tables(segs, jh.DHT)
        ac1 = next(t for t in hts if t[0] == 0x11)
        hfirst = jh.index(segs, jh.DHT)
        hlast = jh.index(segs, jh.DHT, -1) + 1
        wrong_h = _seg(jh.DHT, bytes([0x10]) + ac1[1:])
        _add(f"redef_dht_later_wins_{src}", src,
             jh.join(segs[:hfirst] + [wrong_h] + segs[hfirst:], tail), "same", fam,
             other=jh.join(segs[:hlast] + [wrong_h] + segs[hlast:], tail))
        # one segment holding the slot twice
        both = _seg(jh.DHT, wrong_h[1] + b"".join(hts))
        _add(f"redef_dht_twice_in_one_segment_{src}", src,
             jh.join(jh.edit(jh.without(segs, jh.DHT), insert=[both], before=jh.SOS), tail),
             "same", fam)
    segs, tail = jh.split(source("b420n"))  # coded without restarts: DRI 5 then DRI 0
    _add("redef_dri_nonzero_then_zero", "b420n",
         jh.join(jh.edit(segs, insert=[_seg(jh.DRI, b"\x00\x05")], before=jh.DQT), tail), "same", fam)
    for src in ("b420", "sp420", "pc420"):  # coded with restarts: DRI 0 first
        segs, tail = jh.split(source(src))
        _add(f"redef_dri_zero_then_nonzero_{src}", src,
             jh.join(jh.edit(segs, insert=[_seg(jh.DRI, b"\x00\x00")], before=jh.DQT), tail),
             "same", fam)


def _fill():
    fam = "fill"
    for src in ("b420", "ycck", "sp420", "pc420", "q90_420", "prog_420"):
        segs, tail = jh.split(source(src))
        items = jh.split_tail(tail)
        for n in (1, 2, 15):
            _add(f"fill_{n}_every_marker_{src}", src,
                 b"\xff\xd8" + jh.serialise(segs + items, n), "same", fam)
        if src in ("q90_420", "prog_420"):
            continue
        kinds = sorted({m for m, p in segs + items if m is not None})
        for m in kinds:
            _add(f"fill_2_marker_{m:02x}_{src}", src,
                 b"\xff\xd8" + jh.serialise(segs + items, 2, only=(m,)), "same", fam)
    for src in ("b420", "sp420", "pc420"):
        segs, tail = jh.split(source(src))
        i = jh.index(segs, jh.SOFS)
        _add(f"garbage_between_segments_{src}", src,
             jh.join(segs[:i] + [(None, b"\x00\x12\x34\xd8\xda\x7f")] + segs[i:], tail), "same", fam)
        # (Pillow's own marker scan, ahead of libjpeg, stops at FF 01)
        _add(f"tem_between_segments_{src}", src,
             jh.join(segs[:i] + [(jh.TEM, None)] + segs[i:], tail), "same", fam, pillow=False)
        _add(f"stray_rst0_between_segments_{src}", src,
             jh.join(segs[:i] + [(0xD0, None)] + segs[i:], tail), "same", fam)
    for src in ("sp420", "pc420"):  # the same between the segments ahead of a later scan
        segs, tail = jh.split(source(src))
        com = _seg(jh.COM, b"between")
        for name, thing in (("garbage", (None, b"\x00\x12\x34\xd8\xda\x7f")),
                            ("tem", (jh.TEM, None)), ("stray_rst0", (0xD0, None))):
            _add(f"{name}_between_scans_{src}", src,
                 jh.join(segs, _between_scans(tail, [com, thing, com])), "same", fam)


def _metadata():
    fam = "metadata"
    thumb = _thumbnail()
    big = (bytes(range(256)) * 256)[:65533]
    kinds = {
        "app1_jpeg": [_seg(jh.APP1, b"Exif\x00\x00" + thumb)],
        "app0_jfxx_jpeg": [_seg(jh.APP0, b"JFXX\x00\x10" + thumb)],
        "app2_jpeg_in_three": [_seg(jh.APP2, b"ICC_PROFILE\x00" + bytes([k + 1, 3]) + part)
                               for k, part in enumerate((thumb[:40], thumb[40:200], thumb[200:]))],
        "com_empty": [_seg(jh.COM, b"")],
        "com_65535": [_seg(jh.COM, big)],
        "app14_too_short": [_adobe(0, n=11)],
    }
    for src in ("b420", "b444", "sp420", "pc420", "q90_420", "prog_420"):
        segs, tail = jh.split(source(src))
        multi = src in MULTISCAN
        for kname, new in kinds.items():
            if src in ("q90_420", "prog_420", "b444") and kname not in ("app1_jpeg", "com_65535"):
                continue
            places = {"front": jh.join(new + segs, tail),
                      "before_sof": jh.join(jh.edit(segs, insert=new, before=jh.SOFS), tail),
                      "before_sos": jh.join(jh.edit(segs, insert=new, before=jh.SOS), tail)}
            if multi:
                places["between_scans"] = jh.join(segs, _between_scans(tail, new))
                places["after_last_scan"] = jh.join(segs, _between_scans(tail, new, -1))
            for place, data in places.items():
                _add(f"meta_{kname}_{place}_{src}", src, data, "same", fam)
    # APP14: the flag that counts is the last one before the SOF
    for src in ("b420", "sp420"):  # no APP14: YCbCr; a transform 0 behind the SOF must not apply
        segs, tail = jh.split(source(src))
        # (the colour model is FFmpeg's, decided at the SOF; libjpeg decides at the
        # first SOS and would take this flag, as Pillow does: the oracle alone pins it.
        # libjpeg's levels carry no colour model, so its coefficient check still runs)
        _add(f"meta_app14_after_sof_{src}", src,
             jh.join(jh.edit(segs, insert=[_adobe(0)], after=jh.SOFS), tail), "same", fam,
             pillow=False)
        rgb = jh.join(jh.edit(segs, insert=[_adobe(0)], before=jh.SOFS), tail)
        _add(f"meta_app14_before_sof_{src}", src, rgb, UNSUPPORTED, "refused", probe=UNSUPPORTED,
             key="!frame_color(nf, in.comp_h, in.comp_v, comp_id, adobe, &in.color)")
    for src in ("ycck", "pcycck"):  # transform 2 in the file
        segs, tail = jh.split(source(src))
        _add(f"meta_app14_twice_last_wins_{src}", src, jh.join([_adobe(0)] + segs, tail), "same", fam,
             other=jh.join(jh.edit(segs, insert=[_adobe(0)], after=jh.APP14), tail))
        _add(f"meta_app14_twice_other_last_{src}", src,
             jh.join(jh.edit(segs, insert=[_adobe(0)], after=jh.APP14), tail), "ok", fam,
             other=source(src))
        _add(f"meta_app14_after_sof_{src}", src,
             jh.join(jh.edit(segs, insert=[_adobe(0)], after=jh.SOFS), tail), "same", fam)
        _add(f"meta_app14_too_short_after_{src}", src,
             jh.join(jh.edit(segs, insert=[_adobe(0, n=11)], after=jh.APP14), tail), "same", fam)


def _multiscan_only():
    fam = "multiscan"
    # DRI changed between scans: the scans of two writes of the same levels
    for name, first, then, seg in (("to_zero", "sp420", "sp420n", b"\x00\x00"),
                                   ("to_one", "sp420n", "sp420", b"\x00\x01")):
        segs, tail = jh.split(source(first))
        a, b = jh.split_tail(tail), jh.split_tail(jh.split(source(then))[1])
        assert [m for m, _ in a] == [m for m, _ in b]
        sos = [k for k, (m, _) in enumerate(a) if m == jh.SOS]
        cut = sos[2]  # the DC scan and two AC scans by the first interval
        _add(f"ms_dri_{name}_between_scans", first,
             jh.join(segs, jh.serialise(a[:cut] + [_seg(jh.DRI, seg)] + b[cut:])), "same", fam)
    # (another interval: 1 -> 2, the later scans written with 2)
    two = _write(24, 16, S420, scans="spectral", restart_interval=2)
    segs, tail = jh.split(source("sp420"))
    a, b = jh.split_tail(tail), jh.split_tail(jh.split(two)[1])
    cut = [k for k, (m, _) in enumerate(a) if m == jh.SOS][2]
    _add("ms_dri_to_two_between_scans", "sp420",
         jh.join(segs, jh.serialise(a[:cut] + [_seg(jh.DRI, b"\x00\x02")] + b[cut:])), "same", fam)
    _add("ms_dht_replaced_between_scans", "sc420", _script420(True), "same", fam)
    # more marker-like pairs than the multi-scan walk's candidate list holds
    blob = [_seg(jh.APP2, _ff_blob(40, 3000))]
    for src in ("sp420", "pc420"):
        segs, tail = jh.split(source(src))
        _add(f"ms_ff_blob_front_{src}", src, jh.join(blob + segs, tail), "same", fam)
        _add(f"ms_ff_blob_between_scans_{src}", src, jh.join(segs, _between_scans(tail, blob, 2)),
             "same", fam)
        _add(f"ms_ff_blob_after_last_scan_{src}", src, jh.join(segs, _between_scans(tail, blob, -1)),
             "same", fam)


def _ids_and_selectors():
    fam = "ids"
    for src, kw in (("b420", dict(restart_interval=1)),
                    ("sp420", dict(scans="spectral", restart_interval=1)),
                    ("pc420", dict(scans="per_component", restart_interval=2))):
        for tag, cids in (("0_1_2", (0, 1, 2, 3)), ("10_200_255", (10, 200, 255, 4)),
                          ("Y_C_c", (ord("Y"), ord("C"), ord("c"), 4))):
            _add(f"ids_{tag}_{src}", src, _write(24, 16, S420, comp_ids=cids, **kw), "same", fam)
        # every component its own quantiser table, id 3 among them
        _, q = _levels(7, 24, 16, S420)
        _add(f"ids_tq_0_1_3_{src}", src,
             _write(24, 16, S420, q={0: q[0], 1: q[1], 3: q[1]}, tq=[0, 1, 3], **kw), "same", fam)
        # all components on one DC and one AC table
        one = {("dc", 0): jw.std_tables()[("dc", 0)], ("ac", 0): jw.std_tables()[("ac", 0)]}
        _add(f"ids_one_dc_one_ac_{src}", src,
             _write(24, 16, S420, dht=one, td=[0, 0, 0], ta=[0, 0, 0], **kw), "same", fam)
    _, q = _levels(10, 16, 16, [(1, 1)] * 4)
    _add("ids_tq_0_1_2_3_ycck", "ycck",
         _write(16, 16, [(1, 1)] * 4, seed=10, adobe=2, emit_dri=True,
                q={0: q[0], 1: q[1], 2: q[1], 3: q[0]}, tq=[0, 1, 2, 3]), "same", fam)
    # SOF1 (extended sequential) with Huffman table ids 2 and 3
    std = jw.std_tables()
    hi = {("dc", 2): std[("dc", 0)], ("ac", 2): std[("ac", 0)],
          ("dc", 3): std[("dc", 1)], ("ac", 3): std[("ac", 1)]}
    for src, kw in (("b420", dict(restart_interval=1)),
                    ("pc420", dict(scans="per_component", restart_interval=2))):
        d = _write(24, 16, S420, dht=hi, td=[2, 3, 3], ta=[2, 3, 3], **kw)
        segs, tail = jh.split(d)
        i = jh.index(segs, jh.SOF0)
        segs[i] = (jh.SOF1, segs[i][1])
        _add(f"ids_sof1_tables_2_3_{src}", src, jh.join(segs, tail), "same", fam)
    # the SOS lists the frame's components in another order than the SOF
    # (4:4:4: the MCU is one block per component, in the scan's order): the
    # stream is written with the first two components exchanged, then the SOF
    # is put back in the usual order
    lv, q = _levels(8, 16, 16, S444)
    d = jw.write_jpeg(16, 16, S444, [lv[1], lv[0], lv[2]], q, [1, 0, 1], jw.std_tables(), [1, 0, 1],
                      [1, 0, 1], comp_ids=(2, 1, 3, 4), emit_dri=True)
    segs, tail = jh.split(d)
    p = bytearray(jh.payload(segs, jh.SOF0))
    p[6:9], p[9:12] = p[9:12], p[6:9]
    segs[jh.index(segs, jh.SOF0)] = (jh.SOF0, bytes(p))
    # (libjpeg 9 reads it; libjpeg-turbo, behind Pillow, calls the stream broken)
    _add("ids_sos_order_differs_b444", "b444", jh.join(segs, tail), "same", fam, reordered=True,
         pillow=False)


def _ends():
    fam = "ends"
    for src in ("b420", "sp420", "pc420"):
        d = source(src)
        assert d[-2:] == b"\xff\xd9"
        _add(f"end_bytes_after_eoi_{src}", src, d + b"\x00\xff\xd8\xff\xc0trailing", "oracle", fam)
        # (Pillow's file layer reports a missing EOI as a truncated file)
        _add(f"end_no_eoi_{src}", src, d[:-2], "oracle", fam, pillow=False)
        _add(f"end_eoi_replaced_by_com_{src}", src, d[:-2] + b"\xff\xfe\x00\x04ab", "oracle", fam,
             pillow=False)


# ---- the LDS window ---------------------------------------------------------

@functools.lru_cache(maxsize=None)
def window_streams():
    """[(name, bytes)]: the "win" source with a COM pad right behind SOI, of
    every length that puts file offset 4096 (the end of the parse kernel's LDS
    window) on each byte of the header behind it -- APP14, both DQTs (one with
    16-bit entries), SOF, the four DHTs, DRI, SOS -- and on the first bytes of
    the scan."""
    d = source("win")
    segs, tail = jh.split(d)
    hdr = len(jh.serialise(segs))
    out = []
    for j in range(0, hdr + 3):  # offset 4096 is byte j behind the pad
        n = 4096 - 2 - 4 - j
        out.append((f"win_4096_on_{j}", jh.join([_seg(jh.COM, bytes(n))] + segs, tail)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def nh_streams():
    """[(name, bytes)]: the "nh" source (under 4096 bytes) with a COM pad of
    0..15 bytes behind SOI: every size % 16, so the window's end size & ~15
    falls on each of the file's last 15 bytes -- EOI, the scan, the SOS
    header and the last value of the DC table."""
    segs, tail = jh.split(source("nh"))
    out = [(f"nh_pad{n}", jh.join([_seg(jh.COM, bytes(n))] + segs, tail)) for n in range(16)]
    assert {len(d) % 16 for _, d in out} == set(range(16)) and all(len(d) < 4096 for _, d in out)
    return tuple(out)


def _nh_edge():
    """A header that ends in the file's last 15 bytes: the scan replaced by a
    file that stops right behind a table.  Refused (no scan), by both sides;
    the table's bytes are read through the far path."""
    d = source("win")
    segs, _ = jh.split(d)
    body = [s for s in segs if s[0] != jh.SOS]
    for pad in range(16):
        data = jh.join([_seg(jh.COM, bytes(pad))] + body, b"")
        _add(f"nh_table_at_end_pad{pad}", "win", data, BAD_HEADER, "refused", key="pos >= size")


# ---- refused headers --------------------------------------------------------

def _refused():
    fam = "refused"
    src = "b420"
    d = source(src)
    segs, tail = jh.split(d)

    def add(name, key, data, status=BAD_HEADER, s=src, seen=False, layout=False):
        # seen: the host probe looks at the faulty field and returns the status itself
        _add("bad_" + name, s, data, status, fam, key=key, probe=status if seen else 0,
             layout=layout)

    def patched(marker, off, val, nth=0):
        return jh.join(jh.patch(segs, marker, off, val, nth), tail)

    def cut(marker, n):  # the segment's payload cut to n bytes
        i = jh.index(segs, marker)
        return jh.join(segs[:i] + [(marker, segs[i][1][:n])] + segs[i + 1:], tail)

    # file and segment
    add("three_bytes", "size < 4 || d[0] != 0xFF || d[1] != 0xD8", d[:3], NOT_JPEG, seen=True)
    add("no_soi", "size < 4 || d[0] != 0xFF || d[1] != 0xD8", b"\xff\xd9" + d[2:], NOT_JPEG, seen=True)
    add("ends_before_sos", "pos >= size", jh.join(segs[:-1], b""))
    add("eoi_before_sos", "m == 0xD9", jh.join(segs[:-1] + [(jh.EOI, None)] + segs[-1:], tail))
    add("ends_in_marker", "pos + 2 > size", jh.join(segs[:-1], b"\xff\xdb\x00"))
    i = jh.index(segs, jh.DHT)
    head = jh.join(segs[:i], b"")
    rest = jh.serialise(segs[i + 1:]) + tail
    add("segment_length_0", "len < 2 || pos + len > size", head + b"\xff\xfe\x00\x00" + rest)
    add("segment_length_1", "len < 2 || pos + len > size", head + b"\xff\xfe\x00\x01" + rest)
    add("segment_past_the_end", "len < 2 || pos + len > size",
        jh.join(segs[:-1], b"\xff\xfe\x10\x00" + bytes(100)))
    # DQT
    add("dqt_tq_4", "tq > 3 || pq > 1", patched(jh.DQT, 0, 0x04))
    add("dqt_pq_2", "tq > 3 || pq > 1", patched(jh.DQT, 0, 0x20))
    add("dqt_short_pq0", "n < need", cut(jh.DQT, 65 + 64))
    w = jh.split(source("win"))
    wi = jh.index(w[0], jh.DQT)
    add("dqt_short_pq1", "n < need",
        jh.join(w[0][:wi] + [(jh.DQT, w[0][wi][1][:128])] + w[0][wi + 1:], w[1]), s="win")
    # DHT
    add("dht_tc_2", "tc > 1 || th > 3", patched(jh.DHT, 0, 0x20))
    add("dht_th_4", "tc > 1 || th > 3", patched(jh.DHT, 0, 0x04))
    over1 = bytes([0x00, 3] + [0] * 15) + bytes(3)
    over16 = bytes([0x00] + [1] * 15 + [3]) + bytes(18)
    many = bytes([0x10] + [0] * 7 + [200, 100] + [0] * 7) + bytes(300)
    for name, key, tab in (("dht_overflow_length_1", "code > (1 << l)", over1),
                           ("dht_overflow_length_16", "code > (1 << l)", over16),
                           ("dht_over_256_symbols", "total > 256 || n < 17 + total", many),
                           ("dht_shorter_than_counts", "total > 256 || n < 17 + total",
                            bytes([0x00, 0, 2] + [0] * 14) + bytes(1)),
                           ("dht_under_17", "n < 17", bytes([0x00] + [0] * 10))):
        add(name, key, jh.join(jh.edit(segs, insert=[_seg(jh.DHT, tab)], before=jh.SOS), tail))
    # SOF
    k_sof = "n < 6"
    add("sof_under_6", k_sof, cut(jh.SOF0, 5), seen=True)
    add("sof_precision_12", "p[0] != 8", patched(jh.SOF0, 0, 12), UNSUPPORTED, seen=True)
    add("sof_height_0", "in.height == 0", patched(jh.SOF0, 1, b"\x00\x00"), UNSUPPORTED, seen=True)
    add("sof_width_0", "in.width == 0", patched(jh.SOF0, 3, b"\x00\x00"), seen=True)
    add("sof_nf_2", "nf != 1 && nf != 3 && nf != 4", patched(jh.SOF0, 5, 2), UNSUPPORTED, seen=True)
    add("sof_nf_5", "nf != 1 && nf != 3 && nf != 4", patched(jh.SOF0, 5, 5), UNSUPPORTED, seen=True)
    add("sof_shorter_than_nf", "n < 6 + 3 * nf", cut(jh.SOF0, 6 + 8), seen=True)
    k_samp = ("in.comp_h[c] < 1 || in.comp_h[c] > 4 || in.comp_v[c] < 1 || in.comp_v[c] > 4 || "
              "comp_tq[c] > 3")
    add("sof_sampling_0", k_samp, patched(jh.SOF0, 7, 0x02), seen=True)
    add("sof_sampling_5", k_samp, patched(jh.SOF0, 10, 0x15), seen=True)
    add("sof_tq_4", k_samp, patched(jh.SOF0, 8, 4))
    k_sofn = ("m == 0xC3 || (m >= 0xC5 && m <= 0xC7) || (m >= 0xC9 && m <= 0xCB) || "
              "(m >= 0xCD && m <= 0xCF)")
    for m in (0xC3, 0xC5, 0xC9, 0xCD):
        s2 = list(segs)
        i = jh.index(s2, jh.SOF0)
        s2[i] = (m, s2[i][1])
        add(f"sof{m - 0xC0}", k_sofn, jh.join(s2, tail), UNSUPPORTED, seen=True)
    ids = jh.patch(jh.patch(jh.patch(segs, jh.SOF0, 6, ord("R")), jh.SOF0, 9, ord("G")), jh.SOF0, 12,
                   ord("B"))
    ids = jh.patch(jh.patch(jh.patch(ids, jh.SOS, 1, ord("R")), jh.SOS, 3, ord("G")), jh.SOS, 5,
                   ord("B"))
    add("sof_rgb_ids_sampled", "!frame_color(nf, in.comp_h, in.comp_v, comp_id, adobe, &in.color)",
        jh.join(ids, tail), UNSUPPORTED, seen=True)
    # DRI
    add("dri_length_3", "n < 2", cut(jh.DRI, 1))
    # SOS
    add("sos_before_sof", "!have_sof", jh.join(jh.edit(segs, move=jh.SOF0, after=jh.SOS), tail), seen=True)
    add("sos_empty_last_bytes", "n < 1", jh.join(segs[:-1], b"\xff\xda\x00\x02"))
    add("sos_ns_0", "ns < 1 || ns > in.ncomp", patched(jh.SOS, 0, 0))
    add("sos_ns_4", "ns < 1 || ns > in.ncomp", patched(jh.SOS, 0, 4))
    add("sos_shorter_than_list", "n < 1 + 2 * ns + 3", cut(jh.SOS, 9))
    add("sos_unknown_id", "c < 0", patched(jh.SOS, 3, 9))
    add("sos_td_4", "in.dc_tab[c] > 3 || in.ac_tab[c] > 3", patched(jh.SOS, 2, 0x40))
    k_base = "!in.multiscan && (ss != 0 || se != 63 || ahal != 0)"
    add("sos_baseline_ss_1", k_base, patched(jh.SOS, 7, 1), UNSUPPORTED)
    add("sos_baseline_se_62", k_base, patched(jh.SOS, 8, 62), UNSUPPORTED)
    add("sos_baseline_ahal_10", k_base, patched(jh.SOS, 9, 0x10), UNSUPPORTED)
    add("sof_factor_not_dividing", "hmax % in.comp_h[c] || vmax % in.comp_v[c]",
        jh.join(jh.patch(jh.patch(segs, jh.SOF0, 7, 0x31), jh.SOF0, 10, 0x21), tail), UNSUPPORTED,
        layout=True)
    add("sof_over_10_blocks", "b >= kMaxBpm", patched(jh.SOF0, 7, 0x44), UNSUPPORTED, layout=True)
    # tables
    k_tab = ("!s.qhave[comp_tq[c]] || (!in.multiscan && (!s.have[in.dc_tab[c]] || "
             "!s.have[4 + in.ac_tab[c]]))")
    dq = jh.all_tables(segs, jh.DQT)
    dh = jh.all_tables(segs, jh.DHT)
    add("no_quantiser_table", k_tab,
        jh.join(jh.edit(segs, replace=jh.DQT, insert=[_seg(jh.DQT, dq[0])]), tail))
    add("no_dc_table", k_tab,
        jh.join(jh.edit(segs, replace=jh.DHT,
                        insert=[_seg(jh.DHT, b"".join(t for t in dh if t[0] != 0x01))]), tail))
    add("no_ac_table", k_tab,
        jh.join(jh.edit(segs, replace=jh.DHT,
                        insert=[_seg(jh.DHT, b"".join(t for t in dh if t[0] != 0x11))]), tail))
    # the two decisions: a quantiser table behind the first SOS comes too late
    for s in ("sp420", "pc420"):
        sg, tl = jh.split(source(s))
        late = [x for x in sg if x[0] == jh.DQT]
        add(f"dqt_after_first_sos_{s}", k_tab,
            jh.join(jh.without(sg, jh.DQT), _between_scans(tl, late)), s=s)

    # ---- the scans of a multi-scan file (multiscan_kernel's marker walk) ----
    for s in ("sp420", "pc420"):
        sg, tl = jh.split(source(s))
        items = jh.split_tail(tl)
        sos = [k for k, (m, _) in enumerate(items) if m == jh.SOS]

        def later(k, off, val, items=items, sos=sos, sg=sg):
            it = list(items)
            p = bytearray(it[sos[k]][1])
            p[off] = val
            it[sos[k]] = (jh.SOS, bytes(p))
            return jh.join(sg, jh.serialise(it))

        add(f"ms_second_scan_unknown_id_{s}", "ms: c < 0 || sc.td[i] > 3 || sc.ta[i] > 3",
            later(0, 1, 77), s=s)
        add(f"ms_second_scan_ta_4_{s}", "ms: c < 0 || sc.td[i] > 3 || sc.ta[i] > 3",
            later(0, 2, 0x04), s=s)
        add(f"ms_later_ns_0_{s}",
            "ms: sc.ns < 1 || sc.ns > in.ncomp || p + 1 + 2 * sc.ns + 3 > seg_end",
            later(0, 0, 0), s=s)
        add(f"ms_later_sos_short_{s}",
            "ms: sc.ns < 1 || sc.ns > in.ncomp || p + 1 + 2 * sc.ns + 3 > seg_end",
            jh.join(sg, jh.serialise(items[:sos[0]] + [(jh.SOS, items[sos[0]][1][:4])]
                                     + items[sos[0] + 1:])), s=s)
        add(f"ms_later_sos_empty_last_bytes_{s}", "ms: sc.ns = p < seg_end ? d[p] : 0",
            jh.join(sg, jh.serialise(items[:sos[0]]) + b"\xff\xda\x00\x02"), s=s)
        short_dht = _seg(jh.DHT, bytes([0x10, 0, 2] + [0] * 14) + bytes(1))
        add(f"ms_dht_between_scans_short_{s}",
            "ms: tc > 1 || th > 3 || total > 256 || p + 17 + total > seg_end",
            jh.join(sg, _between_scans(tl, [short_dht])), s=s)
        add(f"ms_dht_between_scans_th_4_{s}",
            "ms: tc > 1 || th > 3 || total > 256 || p + 17 + total > seg_end",
            jh.join(sg, _between_scans(tl, [_seg(jh.DHT, bytes([0x14]) + dh[3][1:])])), s=s)
        add(f"ms_segment_length_1_between_scans_{s}", "ms: len < 2 || pos + len > size",
            jh.join(sg, jh.serialise(items[:sos[0]]) + b"\xff\xfe\x00\x01"
                    + jh.serialise(items[sos[0]:])), s=s)
        add(f"ms_segment_past_the_end_{s}", "ms: len < 2 || pos + len > size",
            jh.join(sg, jh.serialise(items[:sos[0]]) + b"\xff\xfe\x40\x00" + bytes(50)), s=s)
        add(f"ms_ends_in_marker_{s}", "ms: pos + 2 > size",
            jh.join(sg, jh.serialise(items[:sos[0]]) + b"\xff\xc4\x00"), s=s)
        # a scan that selects a Huffman table no DHT has defined (ms_decode_scan)
        for tab, what in ((0x01, "dc"), (0x11, "ac")):
            hd = [t for t in jh.all_tables(sg, jh.DHT) if t[0] != tab]
            add(f"ms_no_{what}_table_{s}", "ms scan: o < 0",
                jh.join(jh.edit(jh.without(sg, jh.DHT), insert=[_seg(jh.DHT, b"".join(hd))],
                                before=jh.SOS), tl), s=s)
        k_prog = ("ms: prog ? (sc.ss > sc.se || sc.se > 63 || sc.al > 13 || (sc.ss == 0 && "
                  "sc.se != 0) || (sc.ss > 0 && sc.ns != 1)) : (sc.ss != 0 || sc.se != 63 || "
                  "sc.ah || sc.al)")
        n1 = 1 + 2 * items[sos[0]][1][0]  # offset of Ss in the second scan's header
        if s == "sp420":
            add("ms_ss_above_se", k_prog, later(0, n1, 9), s=s)          # band 1..5 -> 9..5
            add("ms_se_64", k_prog, later(1, n1 + 1, 64), s=s)           # band 6..63 -> 6..64
            add("ms_al_14", k_prog, later(0, n1 + 2, 14), s=s)
            add("ms_dc_scan_se_5", k_prog, jh.join(jh.patch(sg, jh.SOS, 8, 5), tl), s=s)
            add("ms_interleaved_ac_scan", k_prog,
                jh.join(jh.patch(jh.patch(sg, jh.SOS, 7, 1), jh.SOS, 8, 5), tl), s=s)
        else:
            add("ms_sequential_ss_1", k_prog, later(0, n1, 1), s=s)
            add("ms_sequential_se_62", k_prog, later(0, n1 + 1, 62), s=s)
            add("ms_sequential_al_1", k_prog, later(0, n1 + 2, 0x01), s=s)


# rows of the walk that no test of this table runs: where they are pinned
ELSEWHERE = {
    "ms: ns >= kMsMaxScans": "tests/test_gpu_handwritten.py::test_scan_limit (scr_scans_65: "
                             "unsupported on the device, decoded by the oracle)",
    "ms: err == kOk && ns == 0": "not reachable: parse_headers has accepted the first SOS the "
                                 "walk then meets",
}


def _truncations():
    """One baseline and one progressive source cut at every segment boundary
    and in the middle of every segment, the scans' segments included.  Both
    are coded without restarts, so a cut inside entropy-coded bytes can only
    run the reader dry (with restarts it may instead lose the next RSTn)."""
    fam = "truncated"
    for src in ("b420n", "sp420n"):
        d = source(src)
        segs, tail = jh.split(d)
        items = segs + jh.split_tail(tail)
        first_sos = jh.index(items, jh.SOS)
        sof_end = 2 + len(jh.serialise(items[:jh.index(items, jh.SOFS) + 1]))
        pos, cuts = 2, []
        for k, (m, p) in enumerate(items):
            n = len(jh.serialise([(m, p)]))
            kind = "ecs" if m is None else f"{m:02x}"
            if n > 1:
                cuts.append((f"{k}_{kind}_mid", pos + n // 2, k, True))
            cuts.append((f"{k}_{kind}_end", pos + n, k, False))
            pos += n
        assert pos == len(d)
        for tag, at, k, mid in cuts[:-1]:  # (the last cut is the whole file)
            if k <= first_sos and not (k == first_sos and not mid):
                want = BAD_HEADER  # the header ends early
            elif items[k][0] is None and mid:
                want = TRUNCATED   # inside entropy-coded bytes
            elif k == first_sos or (items[k][0] == jh.SOS and not mid):
                want = TRUNCATED   # a scan header with no data behind it
            elif src == "b420n":
                want = "oracle"    # behind the scan: only EOI is missing
            elif mid and items[k][0] is not None and items[k][1] is not None:
                want = BAD_HEADER  # a later scan's segment runs past the end
            else:
                want = "oracle"    # between two scans: what was decoded stands
            seen = NOT_JPEG if at < 4 else BAD_HEADER if at < sof_end else 0
            _add(f"trunc_{src}_{tag}", src, d[:at], NOT_JPEG if at < 4 else want, fam,
                 key="truncated" if isinstance(want, int) else "", probe=seen)


def _two_sofs():
    """Two SOF segments of different sizes: the frame is the second (the last
    before the first SOS).  The source is the 24x16 stream; the first SOF
    claims 16x16, 4:4:4."""
    for src in ("b420", "sp420", "pc420"):
        segs, tail = jh.split(source(src))
        sof = segs[jh.index(segs, jh.SOFS)]
        p = bytearray(sof[1])
        p[1:5] = b"\x00\x10\x00\x10"
        p[7] = 0x11
        _add(f"two_sofs_last_wins_{src}", src,
             jh.join(jh.edit(segs, insert=[(sof[0], bytes(p))], before=jh.DQT), tail), "same",
             "two_sofs", libjpeg=False, pillow=False)


@functools.lru_cache(maxsize=None)
def table() -> dict:
    if not _cases:
        _order()
        _redefine()
        _fill()
        _metadata()
        _multiscan_only()
        _ids_and_selectors()
        _ends()
        _two_sofs()
        _refused()
        _nh_edge()
        _truncations()
    return _cases


def names(*, legal: bool | None = None, family: str | None = None) -> list[str]:
    out = []
    for n, c in table().items():
        is_legal = not isinstance(c.expect, int)
        if legal is not None and is_legal != legal:
            continue
        if family is not None and c.family != family:
            continue
        out.append(n)
    return out


def case(name: str) -> Case:
    return table()[name]
