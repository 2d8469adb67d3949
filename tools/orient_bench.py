"""Output orientations fused into the decode's store vs the same batch decoded
unoriented and rotated by a torch pass afterwards, GPU.

  python tools/orient_bench.py [steps] [--rounds R] [--sws-cols C] [--json out.jsonl]

The 256 bench images (480x640 q90 4:2:0) resident in HBM, stretched to
224x224 rgb24 u8 [N, 224, 224, 3], at the decoder's default lanes.  Four legs:

  unoriented   no orientation call (sws_kernel<false>)
  eight_codes  the eight codes dealt evenly, image i has code i % 8
               (spdl_hj_set_orients; sws_kernel<true>)
  all_code_5   every image a quarter turn clockwise (EXIF 6)
  torch_after  the unoriented decode, then a torch pass on the caller's
               stream that gives image i the orientation i % 8: per code an
               index_select, the transpose / flips, an index_copy -- the pass
               is per image because only some images are rotated

The legs run interleaved, `rounds` times each in one process; a leg's figure is
the median of its rounds (the minimum is given too).  Writes one JSON line per
leg and a summary line.  ``--sws-cols C`` caps the output tile's column chunk
("sws_cols") on every leg: a narrower chunk gets a taller band, which lands
transposed as fewer, longer output rows.  The first images of the oriented batches are checked
against the oriented oracle.
"""
import argparse
import json
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from spdl_amd import _lib  # noqa: E402
from spdl_amd._lib import Output  # noqa: E402
from spdl_amd.synthetic import synthetic_slice  # noqa: E402

N = 256
OUT = Output(pix_fmt="rgb24", resize=True, fit_w=224, fit_h=224)
SHAPE = (N, 224, 224, 3)
LEGS = ("unoriented", "eight_codes", "all_code_5", "torch_after")


def pack(datas):
    offs, sizes, pos = [], [], 0
    for d in datas:
        offs.append(pos)
        sizes.append(len(d))
        pos += (len(d) + 64 + 255) // 256 * 256
    host = np.zeros(pos, np.uint8)
    for o, d in zip(offs, datas):
        host[o:o + len(d)] = np.frombuffer(d, np.uint8)
    dev = torch.from_numpy(host).to("cuda:0")
    infos = (_lib.ImageInfo * len(datas))(*[_lib.get_image_info(d) for d in datas])
    return dev, np.asarray(offs, np.int64), np.asarray(sizes, np.int64), infos


def oriented(x, code):
    """[n, H, W, 3] under orientation ``code`` (torch)."""
    if code & 4:
        x = x.transpose(1, 2)
    if code & 1:
        x = x.flip(2)
    if code & 2:
        x = x.flip(1)
    return x


class Leg:
    def __init__(self, packed, mode, sws_cols=0):
        self.mode, self.packed = mode, packed
        self.dec = _lib.Decoder(0)
        if sws_cols:
            self.dec.set_param("sws_cols", sws_cols)
        self.inflight = 2
        self.bufs = [torch.empty(SHAPE, dtype=torch.uint8, device="cuda:0")
                     for _ in range(self.inflight + 1)]
        self.turned = [torch.empty_like(b) for b in self.bufs] if mode == "torch_after" else None
        self.codes = {"unoriented": None, "eight_codes": bytes(i % 8 for i in range(N)),
                      "all_code_5": bytes([5] * N), "torch_after": None}[mode]
        self.idx = [torch.arange(c, N, 8, device="cuda:0") for c in range(8)]
        self.stream = torch.cuda.current_stream()
        self.k = 0

    def submit(self):
        dev, offs, sizes, infos = self.packed
        i = self.k % len(self.bufs)
        b = self.bufs[i]
        self.dec.decode_batch_device(dev.data_ptr(), dev.numel(), offs, sizes, infos, OUT,
                                     b.data_ptr(), b.numel(), stream=self.stream, sync=False,
                                     orients=self.codes)
        t = self.dec.last_ticket()
        if self.mode == "torch_after":
            self.dec.stream_wait(t, self.stream)  # (the lanes run on their own streams)
            for c in range(8):
                self.turned[i].index_copy_(0, self.idx[c], oriented(b.index_select(0, self.idx[c]), c))
        self.k += 1
        return t

    def run(self, n):
        pend = []
        for _ in range(n):
            pend.append(self.submit())
            if len(pend) > self.inflight - 1:
                assert not any(self.dec.wait(pend.pop(0), N))
        for t in pend:
            assert not any(self.dec.wait(t, N))

    def timed(self, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        self.run(steps)
        torch.cuda.synchronize()
        return N * steps / (time.perf_counter() - t0)

    def last(self, n):
        res = (self.turned if self.mode == "torch_after" else self.bufs)[(self.k - 1) % len(self.bufs)]
        return res[:n].cpu().numpy()


def check(datas, got, codes):
    """The first images of a batch against the oracle, oriented."""
    from oracle import oracle as O

    for i in range(got.shape[0]):
        want = O.decode_resize(datas[i], O.Resize(fit_w=224, fit_h=224), pix_fmt="rgb24")
        c = codes[i]
        if c & 4:
            want = np.swapaxes(want, 0, 1)
        if c & 1:
            want = np.flip(want, 1)
        if c & 2:
            want = np.flip(want, 0)
        np.testing.assert_array_equal(got[i], want)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("steps", nargs="?", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sws-cols", type=int, default=0)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    datas = synthetic_slice(range(N))
    packed = pack(datas)
    legs = {m: Leg(packed, m, a.sws_cols) for m in LEGS}
    p = _lib.debug_sws_plan(640, 480, 1, 1, "yuv", OUT, **({"max_cols": a.sws_cols} if a.sws_cols else {}))
    tile = {"sws_cols": legs["unoriented"].dec.get_param("sws_cols"), "col_chunk": p["col_chunk"],
            "rb": p["rb"], "chunks": p["chunks"], "bands": p["bands"]}
    for leg in legs.values():
        leg.run(a.warmup)
    torch.cuda.synchronize()
    check(datas, legs["unoriented"].last(2), [0, 0])
    check(datas, legs["eight_codes"].last(8), list(range(8)))
    check(datas, legs["all_code_5"].last(2), [5, 5])
    check(datas, legs["torch_after"].last(8), list(range(8)))
    rates = {m: [] for m in LEGS}
    for _ in range(a.rounds):
        for m in LEGS:
            rates[m].append(legs[m].timed(a.steps))
    lines = []
    for m in LEGS:
        lines.append({"leg": m, "images": N, "steps": a.steps, "rounds": a.rounds,
                      "lanes": legs[m].dec.get_param("lanes"), "tile": tile,
                      "img_per_s_median": round(statistics.median(rates[m]), 1),
                      "img_per_s_min": round(min(rates[m]), 1),
                      "img_per_s_rounds": [round(r, 1) for r in rates[m]]})
    med = {m: statistics.median(rates[m]) for m in LEGS}
    lines.append({"summary": True,
                  "eight_codes_over_unoriented": round(med["eight_codes"] / med["unoriented"], 4),
                  "all_code_5_over_unoriented": round(med["all_code_5"] / med["unoriented"], 4),
                  "torch_after_over_unoriented": round(med["torch_after"] / med["unoriented"], 4),
                  "eight_codes_over_torch_after": round(med["eight_codes"] / med["torch_after"], 4),
                  "checked": "the first images of each leg's warm-up batch bit-exact vs the "
                             "oracle, oriented"})
    for leg in legs.values():
        leg.dec.close()
    for ln in lines:
        print(json.dumps(ln))
    if a.json:
        with open(a.json, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
