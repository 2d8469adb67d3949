"""GPU sweep of the output stage (-m gpu): every entry of the census-driven
case table (tests/sws_sweep_cases.py; tests/test_sws_plan.py says which
kernel and tiler path each entry takes) through the C-ABI, bit-exact against
``oracle.decode_resize`` -- tolerance 0, as everywhere.

Each (spec, filter) cell is a handful of tiny batches, grouped by output size
so that mixed plans take the flat grid and equal ones the 3-D grid; each
batch is decoded in front of a guard image that must stay untouched.
"""

import functools

import numpy as np
import pytest
import torch

from spdl_amd._lib import Output
from tests import sws_sweep_cases as S
from tests import yuv_scale_ref

pytestmark = pytest.mark.gpu

GUARD = 0xA5
GUARD_WORD = 0x5A5A  # 16-bit outputs (a NaN-free, positive int16 pattern)
CELLS = [(s, f) for s in S.SPECS for f in S.FILTERS]


@functools.lru_cache(maxsize=None)
def _ref(name, spec, filt, pix_fmt="rgb24", norm=None):
    """The oracle's output of one table entry, computed once and read-only."""
    from oracle import oracle as O

    kw = dict(normalize=True, norm_dtype=norm) if norm else {}
    a = O.decode_resize(S.source(name), S.resize(O, spec, filt), pix_fmt=pix_fmt, **kw)
    a = a.view(np.uint16) if norm else a
    a.setflags(write=False)
    return a


def _decode(dec, names, out: Output, shape):
    """[n, *shape] of one decode_batch into a guard-filled buffer with one
    image's worth of guard behind the batch (u8, or the 16-bit patterns of a
    normalised output)."""
    n, per = len(names), int(np.prod(shape))
    if out.normalize:
        t = torch.full(((n + 1) * per,), GUARD_WORD, dtype=torch.int16, device="cuda:0")
        want = GUARD_WORD
    else:
        t = torch.full(((n + 1) * per,), GUARD, dtype=torch.uint8, device="cuda:0")
        want = GUARD
    st = dec.decode_batch([S.source(x) for x in names], out, t.data_ptr(),
                          n * per * t.element_size(), stream=torch.cuda.current_stream())
    assert all(s == 0 for s in st)
    a = t.cpu().numpy()
    assert (a[n * per:] == want).all(), "wrote past the batch's output"
    a = a[: n * per].reshape((n,) + tuple(shape))
    return a.view(np.uint16) if out.normalize else a


class _knobs:
    def __init__(self, dec, prepass, cols):
        self.dec, self.v = dec, (prepass, cols)

    def __enter__(self):
        self.dec.set_param("sws_prepass", self.v[0])
        self.dec.set_param("sws_cols", self.v[1])

    def __exit__(self, *exc):
        self.dec.set_param("sws_prepass", -1)
        self.dec.set_param("sws_cols", 256)


def _accepted(group, spec, filt, pre, cols):
    return all(S.probe(x, spec, filt, pre, cols)["rc"] == 0 for x in set(group))


def _sweep(dec, spec, filt, pix_fmt, knob_sets, norm=None):
    done = 0
    for group in S.batches(spec, filt):
        refs = [_ref(x, spec, filt, pix_fmt, norm) for x in group]
        out = S.output(spec, filt, pix_fmt=pix_fmt, normalize=bool(norm),
                       norm_dtype=norm or "float16")
        for pre, cols in knob_sets:
            if not _accepted(group, spec, filt, pre, cols):
                assert pre == 0, "a plan the oracle accepts is refused with the pre-pass allowed"
                continue
            with _knobs(dec, pre, cols):
                hyp = _decode(dec, group, out, refs[0].shape)
            for i, (name, ref) in enumerate(zip(group, refs)):
                np.testing.assert_array_equal(
                    hyp[i], ref, strict=True,
                    err_msg=f"{name}[{i}] {spec} {filt} {pix_fmt} pre={pre} cols={cols}")
            done += 1
    assert done, "the cell has no accepted entry"


@pytest.mark.parametrize("spec,filt", CELLS)
def test_sweep_rgb24(decoder, oracle, spec, filt):
    """Every table entry as rgb24, three ways: the default plan, the
    horizontal pass forced into hscale_kernel, and forced into sws_kernel
    (hpass buckets, hpass_cols_long past 64 taps); narrow tiles where the
    table asks for them."""
    _sweep(decoder, spec, filt, "rgb24", S.knobs(spec))


@pytest.mark.parametrize("i,spec,filt", [(i, s, f) for i, (s, f) in enumerate(CELLS)])
def test_sweep_other_formats(decoder, oracle, i, spec, filt):
    """A rotating subset as rgb, bgr and bgr24 (planar tiles, swapped channels)."""
    _sweep(decoder, spec, filt, S.ROTATION[i % 3], S.KNOBS[:1])


@pytest.mark.parametrize("pix_fmt", ["rgb", "rgb24"])
@pytest.mark.parametrize("norm", ["float16", "bfloat16"])
@pytest.mark.parametrize("filt", S.FILTERS)
@pytest.mark.parametrize("spec", S.NORM_SPECS)
def test_sweep_normalised(decoder, oracle, spec, filt, norm, pix_fmt):
    """The fp16 / bf16 epilogue (straight to HBM, pad pixels included), planar
    and interleaved, on a padded, a multi-chunk and an odd-sized spec: bit
    patterns against the oracle."""
    _sweep(decoder, spec, filt, pix_fmt, S.KNOBS[:1], norm=norm)


REFUSED = [(s, f) for s, f in CELLS if S.refused(s, f)]


@pytest.mark.parametrize("spec,filt", REFUSED)
def test_refused_geometries_raise_and_recover(decoder, oracle, spec, filt):
    """Past the refusal boundary (a scale filter of 256 taps or more): each
    entry in a call of its own raises, and a good decode on the same decoder
    afterwards is exact."""
    good = "tex_444_3x2"
    for name in S.refused(spec, filt):
        t = torch.full((1 << 16,), GUARD, dtype=torch.uint8, device="cuda:0")
        with pytest.raises(RuntimeError, match="scale filter too long"):
            decoder.decode_batch([S.source(name)], S.output(spec, filt), t.data_ptr(), t.numel(),
                                 stream=torch.cuda.current_stream())
        assert (t.cpu().numpy() == GUARD).all(), f"{name}: a refused call wrote output"
        ref = _ref(good, "odd51x37", "bicubic")
        hyp = _decode(decoder, [good], S.output("odd51x37", "bicubic"), ref.shape)
        np.testing.assert_array_equal(hyp[0], ref, strict=True, err_msg=f"after {name}")


# ---- planar output (yuv_planes_kernel): the long-filter and multi-chunk rows ----
# (400 -> 8 lanczos is past the refusal boundary: 272 -> 8 is its four-chunk row)
PLANAR = [(n, s, f) for n, s in (("tex_420_400x24", "w8"), ("tex_gray_400x24", "w8"),
                                 ("tex_420_272x40", "w8"), ("tex_420_400x24", "wide598x10"),
                                 ("tex_gray_400x24", "wide598x10"))
          for f in S.FILTERS if n not in S.refused(s, f)]


@pytest.mark.parametrize("name,spec,filt", PLANAR)
def test_sweep_planar(decoder, oracle, name, spec, filt):
    """pix_fmt="yuv" on 4:2:0 and gray: over 64 taps with the pre-pass (the
    chunk loops of hscale_kernel) and without (hpass_cols_long), and tiles of
    16 columns with a narrower last one; against tests/yuv_scale_ref.py."""
    data = S.source(name)
    want = yuv_scale_ref.scale_packed(data, S.resize(oracle, spec, filt))
    out = S.output(spec, filt, pix_fmt="yuv")
    for pre, cols in (*S.KNOBS, S.NARROW):
        p = S.probe(name, spec, filt, pre, cols, pix_fmt="yuv")
        assert p["rc"] == 0
        if spec == "w8":
            assert p["hl"]["taps"] > 64 and p["pre"] == (pre != 0)
        n = want.size
        t = torch.full((2 * n,), GUARD, dtype=torch.uint8, device="cuda:0")
        with _knobs(decoder, pre, cols):
            st = decoder.decode_batch([data], out, t.data_ptr(), n,
                                      stream=torch.cuda.current_stream())
        assert st == [0]
        a = t.cpu().numpy()
        assert (a[n:] == GUARD).all(), "wrote past the image's planes"
        np.testing.assert_array_equal(a[:n], want, strict=True,
                                      err_msg=f"{name} {spec} {filt} pre={pre} cols={cols}")
