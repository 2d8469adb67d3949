"""Tuning knobs that change launch shapes but must not change a byte
(ADVICE r05): swscale tile width (`sws_cols`), parse_kernel workgroup size
(`parse_threads`), the entropy waves' priority (`entropy_prio`) and the
XCD-aware tile order of swscale / IDCT (`xcd_order`, round 6) and the
multi-scan launch of a batch without multi-scan images (`ms_skip_empty`), each
bit-exact vs the oracle on a few resize cases in one batch; and the fields of
the entropy launch (`warmup_slots`, `min_run_slots`, `chain_after`,
`entropy_prio`) at the ends of their ranges, alone and all together.
"""

import numpy as np
import pytest
import torch

from spdl_amd._lib import Output
from tests import cases

pytestmark = pytest.mark.gpu

NAMES = ["q90_420", "odd_227x333", "gray", "restart_rows", "large_1080p", "optimized"]
SPECS = {
    "pad224": dict(fit_w=224, fit_h=224, aspect="decrease", pad_w=224, pad_h=224),
    "crop224": dict(fit_w=224, fit_h=224, aspect="increase", crop_w=224, crop_h=224),
    "stretch160x120": dict(fit_w=160, fit_h=120),
}


@pytest.mark.parametrize("knob,value", [("sws_cols", 16), ("sws_cols", 64),
                                        ("parse_threads", 128), ("parse_threads", 256),
                                        ("entropy_prio", 3), ("xcd_order", 0), ("xcd_order", 2), ("xcd_order", 3),
                                        ("ms_skip_empty", 1)])
@pytest.mark.parametrize("sk", list(SPECS))
def test_knob_bit_exact(decoder, oracle, knob, value, sk):
    kw = SPECS[sk]
    datas = [cases.case(n) for n in NAMES]
    refs = [oracle.decode_resize(d, oracle.Resize(**kw), pix_fmt="rgb24") for d in datas]
    out = Output(pix_fmt="rgb24", resize=True, **kw)
    h, w = refs[0].shape[:2]
    prev = decoder.get_param(knob)
    decoder.set_param(knob, value)
    try:
        t = torch.empty((len(datas), h, w, 3), dtype=torch.uint8, device="cuda:0")
        st = decoder.decode_batch(datas, out, t.data_ptr(), t.numel(),
                                  stream=torch.cuda.current_stream())
    finally:
        decoder.set_param(knob, prev)
    assert not any(st), st
    hyp = t.cpu().numpy()
    for i, r in enumerate(refs):
        np.testing.assert_array_equal(hyp[i], r, strict=True, err_msg=f"{knob}={value} {NAMES[i]}")


# The entropy launch's fields (hj_common.h EntropyParams): the output does not
# depend on them, and they do not depend on the output shape, so one geometry.
ENTROPY_KNOBS = ("warmup_slots", "min_run_slots", "chain_after", "entropy_prio")


@pytest.fixture(scope="module")
def stretch_batch(oracle):
    kw = SPECS["stretch160x120"]
    datas = [cases.case(n) for n in NAMES]
    refs = [oracle.decode_resize(d, oracle.Resize(**kw), pix_fmt="rgb24") for d in datas]
    return datas, refs, Output(pix_fmt="rgb24", resize=True, **kw)


@pytest.fixture
def own_decoder(decoder):
    """A context of the test's own: warmup_slots and chain_after cannot be set
    back to "by schedule" once set, which would pin the session's decoder."""
    from spdl_amd._lib import Decoder

    dec = Decoder(0)
    yield dec
    dec.close()


def _set_decode_check(dec, batch, params):
    datas, refs, out = batch
    prev = {k: dec.get_param(k) for k in params}
    try:
        for k, v in params.items():
            dec.set_param(k, v)
            assert dec.get_param(k) == v, k
        t = torch.empty((len(datas), 120, 160, 3), dtype=torch.uint8, device="cuda:0")
        st = dec.decode_batch(datas, out, t.data_ptr(), t.numel(),
                              stream=torch.cuda.current_stream())
    finally:
        for k, v in prev.items():
            dec.set_param(k, v)
    assert not any(st), st
    hyp = t.cpu().numpy()
    for i, r in enumerate(refs):
        np.testing.assert_array_equal(hyp[i], r, strict=True, err_msg=f"{params} {NAMES[i]}")


@pytest.mark.parametrize("knob,value", [("warmup_slots", 0), ("warmup_slots", 64),
                                        ("min_run_slots", 4), ("min_run_slots", 64),
                                        ("chain_after", 0), ("chain_after", 15),
                                        ("entropy_prio", 1), ("entropy_prio", 2)])
def test_entropy_field_alone(own_decoder, stretch_batch, knob, value):
    """Each field of the entropy launch alone at both ends of its range:
    get_param reports the value set and the batch stays bit-exact."""
    _set_decode_check(own_decoder, stretch_batch, {knob: value})


@pytest.mark.parametrize("values", [(64, 64, 15, 3), (0, 0, 0, 0), (0, 4, 0, 1)],
                         ids=["maxima", "minima", "low_ends"])
@pytest.mark.parametrize("threads", [256, 128])
def test_entropy_fields_together(own_decoder, stretch_batch, threads, values):
    """All four fields at their maxima at once, then at their minima (the
    range's, and the low ends test_entropy_field_alone takes): a field that
    reached into its neighbour would show here.  128 threads is the smallest
    workgroup, with the most runs per slot."""
    _set_decode_check(own_decoder, stretch_batch,
                      {"entropy_threads": threads, **dict(zip(ENTROPY_KNOBS, values))})


@pytest.mark.parametrize("value", [1])
def test_ms_skip_empty_with_progressive(decoder, oracle, value):
    """A batch that holds progressive images still launches the multi-scan
    decode over every image whatever `ms_skip_empty` says."""
    names = NAMES[:3] + ["prog_420", "prog_gray"]
    kw = SPECS["pad224"]
    datas = [cases.case(n) for n in names]
    refs = [oracle.decode_resize(d, oracle.Resize(**kw), pix_fmt="rgb24") for d in datas]
    out = Output(pix_fmt="rgb24", resize=True, **kw)
    prev = decoder.get_param("ms_skip_empty")
    decoder.set_param("ms_skip_empty", value)
    try:
        t = torch.empty((len(datas), 224, 224, 3), dtype=torch.uint8, device="cuda:0")
        st = decoder.decode_batch(datas, out, t.data_ptr(), t.numel(),
                                  stream=torch.cuda.current_stream())
    finally:
        decoder.set_param("ms_skip_empty", prev)
    assert not any(st), st
    hyp = t.cpu().numpy()
    for i, r in enumerate(refs):
        np.testing.assert_array_equal(hyp[i], r, strict=True, err_msg=names[i])
