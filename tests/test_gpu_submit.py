"""GPU test of the submission path (-m gpu): one sequence over the five
decode entry points on a decoder of its own, counting tickets.

``last_ticket`` moves only when a submission has reached the device pipeline;
the ticket counter moves only when a ring slot is taken.  So a submission that
the host refuses before it takes a slot (a failed probe, a planning error)
leaves both alone, and one refused after ``staging_acquire`` gives its slot
back.  The outputs of the three batch entry points are the same bytes, and
those of the oracle.  Nothing here provokes a HIP error: every bad input is
refused on the host.
"""

import ctypes
import os

import numpy as np
import pytest
import torch

from spdl_amd import _lib
from spdl_amd._lib import Decoder, Output

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg")
GUARD = 0xA5
SPEC = dict(fit_w=32, fit_h=32, aspect="decrease", pad_w=32, pad_h=32)
OUT = Output(pix_fmt="rgb24", resize=True, **SPEC)
PER = 32 * 32 * 3


def _image(name):
    with open(os.path.join(GOLD, name + ".jpg"), "rb") as f:
        return f.read()


def _buffer():
    return torch.full((2 * PER + 64,), GUARD, dtype=torch.uint8, device="cuda:0")


def _bytes(t):
    a = t.cpu().numpy()
    assert (a[2 * PER:] == GUARD).all(), "wrote past the batch's output"
    return a[:2 * PER].reshape(2, 32, 32, 3)


def test_ticket_sequence_over_the_entry_points(oracle):
    dec = Decoder(0)
    datas = [_image("tiny_8x8"), _image("odd_444_101x67")]
    assert dec.last_ticket() == 0

    # 1: host bytes
    t = _buffer()
    assert dec.decode_batch(datas, OUT, t.data_ptr(), 2 * PER) == [0, 0]
    assert dec.last_ticket() == 1
    A = _bytes(t)
    rs = oracle.Resize(**SPEC)
    for k, d in enumerate(datas):
        np.testing.assert_array_equal(A[k], oracle.decode_resize(d, rs, "rgb24"), strict=True)

    # 2: the probe refuses the second image: no slot, no ticket, no output
    t = _buffer()
    st = dec.decode_batch([datas[0], bytes(64)], OUT, t.data_ptr(), 2 * PER, check=False)
    assert st[0] == 0 and st[1] != 0, st
    assert dec.last_ticket() == 1
    torch.cuda.synchronize()
    assert bool((t == GUARD).all()), "a refused submission wrote output"

    # 3: the same bytes, device resident: ticket 2, so step 2 took none
    offs, total = [], 0
    for d in datas:
        offs.append(total)
        total += (len(d) + 64 + 255) // 256 * 256
    sizes = [len(d) for d in datas]
    host = np.zeros(total + 512, np.uint8)
    for o, d in zip(offs, datas):
        host[o:o + len(d)] = np.frombuffer(d, np.uint8)
    dev = torch.from_numpy(host).to("cuda:0")
    infos = [_lib.get_image_info(d) for d in datas]
    t = _buffer()
    assert dec.decode_batch_device(dev.data_ptr(), dev.numel(), offs, sizes, infos, OUT,
                                   t.data_ptr(), 2 * PER) == [0, 0]
    assert dec.last_ticket() == 2
    np.testing.assert_array_equal(_bytes(t), A, strict=True)

    # 4: the binding refuses three crops for two images before the native call
    with pytest.raises(ValueError, match="3 crops for a batch of 2 images"):
        dec.decode_batch_device(dev.data_ptr(), dev.numel(), offs, sizes, infos, OUT,
                                t.data_ptr(), 2 * PER, crops=[(0, 0, 8, 8)] * 3)
    assert dec.last_ticket() == 2

    # 5: a staged submission refused on the host gives its slot back
    ptr, ticket = dec.staging_acquire(total)
    assert ticket == 3
    ctypes.memmove(ptr, host.ctypes.data, total)
    t = _buffer()
    with pytest.raises(RuntimeError, match="image 1"):
        dec.decode_staged(ticket, total, offs, [sizes[0], total - offs[1] + 1], OUT, t.data_ptr(),
                          2 * PER)
    assert dec.last_ticket() == 2
    with pytest.raises(RuntimeError, match="unknown"):
        dec.wait(3, 2)
    torch.cuda.synchronize()
    assert bool((t == GUARD).all()), "a refused submission wrote output"

    # 6: staged, asynchronous
    ptr, ticket = dec.staging_acquire(total)
    assert ticket == 4
    dec.staging_fill(ticket, 0, host.ctypes.data, total)
    dec.decode_staged(ticket, total, offs, sizes, OUT, t.data_ptr(), 2 * PER, sync=False)
    assert dec.wait(4, 2) == [0, 0]
    np.testing.assert_array_equal(_bytes(t), A, strict=True)
    assert dec.last_ticket() == 4

    # 7: the two one-image entry points take a ticket each
    want = oracle.decode_planes(datas[0])
    planes = dec.decode_planes(datas[0])
    assert [p.shape for p in planes] == [w.shape for w in want]
    for p, w in zip(planes, want):
        np.testing.assert_array_equal(p, w, strict=True)
    assert dec.last_ticket() == 5
    ref, _ = oracle.decode_coefs(datas[0])
    coefs, _, diag = dec.debug_entropy(datas[0], ref.shape[0])
    assert diag["status"] == 0, diag
    np.testing.assert_array_equal(coefs, ref, strict=True)
    assert dec.last_ticket() == 6
    dec.close()
