"""Reduced-size decode (spdl_hj_set_lowres): what the levels cost and save
against the full decode, per workload, GPU.

  python tools/lowres_bench.py [steps] [--rounds R] [--warmup W] [--json out.jsonl]

256 images resident in HBM, decoded into 224x224 rgb24 u8 (fit 224x224,
decrease, centred pad: the headline chain).  Three workloads, at one lane and
at four:

  bench   the 256 bench images (480x640 q90 4:2:0; "auto" resolves to 1)
  mixed   spdl_amd.synthetic.mixed_batch(256)
  big1    spdl_amd.synthetic.big_batch(256): one 12 MP image among 255 bench
          images ("auto": 3 for that image, 1 for the rest)

Arms of a workload: level 0 (no call), "auto", and every fixed level at which
no image of the workload is decoded below the size it scales to (so no image
is upscaled).  The arms of a workload run interleaved, `rounds` times each in
one process; an arm's rate is the median of its rounds.  After the timed
rounds one profiled submission per arm gives the IDCT and output stages'
times (spdl_hj_set_profiling) and the planes workspace bytes
("planes_bytes").  Writes one JSON line per workload, lane count and arm.
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
from spdl_amd.synthetic import big_batch, mixed_batch, synthetic_slice  # noqa: E402

N = 256
OUT = Output(pix_fmt="rgb24", resize=True, fit_w=224, fit_h=224, aspect="decrease", pad_w=224,
             pad_h=224)
PER = 224 * 224 * 3


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
    infos = [_lib.get_image_info(d) for d in datas]
    return dev, np.asarray(offs, np.int64), np.asarray(sizes, np.int64), infos


class Arm:
    def __init__(self, dec, packed, levels):
        self.dec = dec
        self.dev, self.offs, self.sizes, infos = packed
        self.infos = (_lib.ImageInfo * N)(*infos)
        self.levels = None if levels is None else bytes(levels)
        self.inflight = 2
        self.bufs = [torch.empty(N * PER, dtype=torch.uint8, device="cuda:0")
                     for _ in range(self.inflight + 1)]
        self.stream = torch.cuda.current_stream()
        self.k = 0

    def submit(self, sync=False):
        b = self.bufs[self.k % len(self.bufs)]
        self.k += 1
        self.dec.decode_batch_device(self.dev.data_ptr(), self.dev.numel(), self.offs, self.sizes,
                                     self.infos, OUT, b.data_ptr(), N * PER, stream=self.stream,
                                     sync=sync, lowres=self.levels)
        return self.dec.last_ticket()

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

    def profile(self):
        """(idct us, output us, planes bytes) of one profiled submission."""
        self.dec.set_profiling(True)
        self.submit(sync=True)
        t = self.dec.last_timings()
        self.dec.set_profiling(False)
        return t.get("idct"), t.get("output"), self.dec.get_param("planes_bytes")


def arms_of(infos):
    auto = _lib.lowres_levels("auto", infos, OUT) or [0] * N
    arms = {"0": None, "auto": auto}
    for lv in range(1, min(auto) + 1):  # (a fixed level above an image's "auto" would upscale it)
        arms[str(lv)] = [lv] * N
    return arms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("steps", nargs="?", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    workloads = {"bench": synthetic_slice(range(N)), "mixed": mixed_batch(N), "big1": big_batch(N)}
    dec = _lib.Decoder(0)
    lines = []
    for name, datas in workloads.items():
        packed = pack(datas)
        levels = arms_of(packed[3])
        for lanes in (1, 4):
            dec.set_param("lanes", lanes)
            arms = {k: Arm(dec, packed, v) for k, v in levels.items()}
            for arm in arms.values():
                arm.run(a.warmup)
            rates = {k: [] for k in arms}
            for _ in range(a.rounds):
                for k, arm in arms.items():
                    rates[k].append(arm.timed(a.steps))
            for k, arm in arms.items():
                idct_us, out_us, planes = arm.profile()
                lv = levels[k]
                lines.append({"workload": name, "lanes": lanes, "arm": k,
                              "levels": None if lv is None else
                              {str(x): lv.count(x) for x in sorted(set(lv))},
                              "img_per_s_median": round(statistics.median(rates[k]), 1),
                              "img_per_s_rounds": [round(r, 1) for r in rates[k]],
                              "idct_us": idct_us and round(idct_us, 1),
                              "output_us": out_us and round(out_us, 1), "planes_bytes": planes})
                print(json.dumps(lines[-1]), flush=True)
            del arms
    dec.close()
    if a.json:
        with open(a.json, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
