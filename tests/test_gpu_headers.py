"""GPU parity on the header-structure cases (tests/jpeg_header_cases.py): one
coded image under many headers -- segment orders, tables defined twice, fill
bytes and garbage, metadata that holds whole JPEGs, ids and selectors, files
without EOI, headers that cross the parse kernel's LDS window -- and every
refusal of the device parser and of the multi-scan marker walk.

Bar, legal cases: bit-exact vs the oracle on the four surfaces of
test_gpu_handwritten.py (debug_entropy coefficients, planes with both IDCTs,
full-resolution rgb24 on the three output paths, a 32x32 resize).  Refused
cases: the oracle's status from the device, alone and between two good images
that stay bit-exact, and a good decode afterwards.

The CPU side of the same table (test_jpeg_headers.py) pins the oracle to
libjpeg 9 and Pillow and runs the sanitised native sweep over every stream
that goes to the device here; the mutation sweep stays on the CPU.
"""

import ctypes

import numpy as np
import pytest
import torch

from spdl_amd import _lib
from spdl_amd._lib import Output
from tests import jpeg_header_cases as hc
from tests.test_gpu_handwritten import (RESIZE32, _decode, check_coefs, check_planes, check_resize,
                                        check_rgb)

pytestmark = pytest.mark.gpu

LEGAL = hc.names(legal=True)
REFUSED = hc.names(legal=False)
OUT32 = Output(pix_fmt="rgb24", resize=True, **RESIZE32)


def _probe(data):
    info = _lib.ImageInfo()
    addr, size, keep = _lib.buffer_address(data)
    rc = _lib.lib().spdl_hj_get_image_info(addr, size, ctypes.byref(info))
    del keep
    return rc, info


def _oracle_status(oracle, d):
    try:
        oracle.decode_rgb(d)
        return 0
    except oracle.OracleError as e:
        return e.code


def _pack_tight(datas):
    """The files at 256-byte aligned offsets (the interface's rule) with no
    slack: each gap is filled with the next file's first bytes, so the byte
    behind a file is an SOI and what follows reads as a header."""
    offs, total = [], 0
    for d in datas:
        offs.append(total)
        total += (len(d) + 255) // 256 * 256
    host = np.zeros(total + 512, np.uint8)  # (slack behind the last file alone)
    for i, (o, d) in enumerate(zip(offs, datas)):
        host[o:o + len(d)] = np.frombuffer(d, np.uint8)
        end = offs[i + 1] if i + 1 < len(datas) else total
        gap = end - (o + len(d))
        nxt = np.frombuffer(datas[(i + 1) % len(datas)], np.uint8)
        host[o + len(d):end] = np.resize(nxt, gap) if gap else []
    return host, offs


def _decode_device(dec, datas, infos, out: Output, shape, check=True):
    host, offs = _pack_tight(datas)
    dev = torch.from_numpy(host).to("cuda:0")
    t = torch.zeros((len(datas),) + tuple(shape), dtype=torch.uint8, device="cuda:0")
    st = dec.decode_batch_device(dev.data_ptr(), dev.numel(), offs, [len(d) for d in datas],
                                 (_lib.ImageInfo * len(datas))(*infos), out, t.data_ptr(), t.numel(),
                                 stream=torch.cuda.current_stream(), check=check)
    return st, t.cpu().numpy()


# ---- legal layouts ----------------------------------------------------------

@pytest.mark.parametrize("name", LEGAL)
def test_legal_headers(decoder, oracle, name):
    d = hc.case(name).data
    check_coefs(decoder, oracle, d)
    check_planes(decoder, oracle, d)
    check_rgb(decoder, oracle, d)
    check_resize(decoder, oracle, d)


def test_multiscan_cases_in_a_mixed_batch(decoder, oracle):
    """Every legal multi-scan case in one batch, a baseline case after each
    (the multi-scan walk beside the baseline path, as
    test_gpu_multiscan.test_mixed_batch_pad224)."""
    multi = [n for n in LEGAL if hc.case(n).source in hc.MULTISCAN and len(hc.case(n).data) < 20000]
    base = [n for n in LEGAL if hc.case(n).source in hc.BASELINE and len(hc.case(n).data) < 20000]
    assert len(multi) > 80 and len(base) > 80
    names = [n for pair in zip(multi, base * 2) for n in pair]
    datas = [hc.case(n).data for n in names]
    hyp = _decode(decoder, datas, OUT32, (32, 32, 3))
    refs = {}
    for i, (n, d) in enumerate(zip(names, datas)):
        if n not in refs:
            refs[n] = oracle.decode_resize(d, oracle.Resize(**RESIZE32), pix_fmt="rgb24")
        np.testing.assert_array_equal(hyp[i], refs[n], strict=True, err_msg=n)


# ---- the LDS window ---------------------------------------------------------

def _yuv_ref(oracle, d, idct):
    return np.concatenate([p.reshape(-1) for p in oracle.decode_planes(d, idct=idct)])


def _sweep_surfaces(oracle, src):
    """(Output, per-image shape, the unpadded source's reference) per surface."""
    d = hc.source(src)
    n = _yuv_ref(oracle, d, oracle.IDCT_SIMPLE).size
    info = oracle.parse(d)
    own = dict(resize=True, fit_w=info.width, fit_h=info.height)  # scaled to its own size: the planes
    return [
        (Output(pix_fmt="yuv", idct="simple", **own), (n,), _yuv_ref(oracle, d, oracle.IDCT_SIMPLE)),
        (Output(pix_fmt="yuv", idct="islow", **own), (n,), _yuv_ref(oracle, d, oracle.IDCT_ISLOW)),
        (Output(pix_fmt="rgb24"), (info.height, info.width, 3),
         oracle.decode_rgb(d, oracle.IDCT_SIMPLE, "rgb24")),
        (OUT32, (32, 32, 3), oracle.decode_resize(d, oracle.Resize(**RESIZE32), pix_fmt="rgb24")),
    ]


SWEEPS = [pytest.param("win", hc.window_streams, id="win"), pytest.param("nh", hc.nh_streams, id="nh")]


@pytest.mark.parametrize("src,streams", SWEEPS)
@pytest.mark.parametrize("path", ["host", "device_tight"])
def test_lds_window_sweep(decoder, oracle, src, streams, path):
    """Offset 4096 (the end of the parse kernel's LDS window) on every byte of
    the header in turn, and size & ~15 on each of a small file's last 15
    bytes: one batch per surface, image i against the unpadded source's
    reference.  device_tight: the same through decode_batch_device, the files
    packed without slack (the bytes behind a file are its neighbour's SOI and
    header, not padding)."""
    names, datas = zip(*streams())
    infos = [_probe(d)[1] for d in datas]
    for out, shape, ref in _sweep_surfaces(oracle, src):
        if path == "host":
            hyp = _decode(decoder, datas, out, shape)
        else:
            st, hyp = _decode_device(decoder, datas, infos, out, shape)
            assert not any(st), st
        for i, n in enumerate(names):
            np.testing.assert_array_equal(hyp[i].reshape(ref.shape), ref, strict=True,
                                          err_msg=f"{n} {out.pix_fmt} {out.idct}")


@pytest.mark.parametrize("src,streams", SWEEPS)
def test_lds_window_sweep_coefficients(decoder, oracle, src, streams):
    """The coefficient surface of the sweep (debug_entropy takes one image)."""
    ref, _ = oracle.decode_coefs(hc.source(src))
    for n, d in streams():
        hyp, _, diag = decoder.debug_entropy(d, ref.shape[0])
        assert diag["status"] == 0, (n, diag)
        np.testing.assert_array_equal(hyp, ref, strict=True, err_msg=n)


# ---- refused headers --------------------------------------------------------

def _good(oracle):
    out = []
    for src in ("b420", "sp420"):
        d = hc.source(src)
        out.append((d, _probe(d)[1],
                    oracle.decode_resize(d, oracle.Resize(**RESIZE32), pix_fmt="rgb24")))
    return out


@pytest.mark.parametrize("name", REFUSED)
def test_refused_headers(decoder, oracle, name):
    """The oracle's status from the device: alone through decode_batch (the
    host probe refuses what it can see, the device parser the rest), then
    between a baseline and a multi-scan image through decode_batch_device,
    where the device parser meets every file itself -- a file the host would
    turn away with the whole call (the probe refuses it, or the batch layout
    refuses the sampling factors the probe read) travels with its source's
    probe, which the parser must then contradict with the same status.  The
    neighbours stay bit-exact, and the decoder decodes a good batch
    afterwards."""
    c = hc.case(name)
    want = _oracle_status(oracle, c.data)
    assert want == c.expect
    t = torch.empty((32, 32, 3), dtype=torch.uint8, device="cuda:0")
    st = decoder.decode_batch([c.data], OUT32, t.data_ptr(), t.numel(),
                              stream=torch.cuda.current_stream(), check=False)
    assert st == [want]
    rc, info = _probe(c.data)
    assert rc == c.probe
    if rc or c.layout:
        info = _probe(hc.source(c.source))[1]
    (g0, i0, r0), (g1, i1, r1) = _good(oracle)
    st, hyp = _decode_device(decoder, [g0, c.data, g1], [i0, info, i1], OUT32, (32, 32, 3),
                             check=False)
    assert st == [0, want, 0]
    np.testing.assert_array_equal(hyp[0], r0, strict=True)
    np.testing.assert_array_equal(hyp[2], r1, strict=True)
    hyp = _decode(decoder, [g1, g0], OUT32, (32, 32, 3))
    np.testing.assert_array_equal(hyp[0], r1, strict=True)
    np.testing.assert_array_equal(hyp[1], r0, strict=True)


def test_two_sofs_decode_at_the_second_size(decoder, oracle):
    """Two SOF segments: the frame is the last before the first SOS, for the
    probe (which sizes the buffers), the device parser and the oracle."""
    for name in hc.names(family="two_sofs"):
        d = hc.case(name).data
        info = _lib.get_image_info(d)
        assert (info.width, info.height) == (24, 16)
        ref = oracle.decode_rgb(d, oracle.IDCT_SIMPLE, "rgb24")
        assert ref.shape == (16, 24, 3)
        np.testing.assert_array_equal(_decode(decoder, [d], Output(pix_fmt="rgb24"), ref.shape)[0],
                                      ref, strict=True)
