"""Pillow-exact decode: csc="turbo" against the two other full-resolution
conversions, GPU.

  python tools/turbo_bench.py [steps] [--rounds R] [--warmup W] [--json out.jsonl]

256 images resident in HBM, decoded at full resolution to rgb24 u8.  Five
arms, at one lane and at the lanes the library chooses for the hardware queues
in effect:

  turbo          the 256 bench images (480x640 q90 4:2:0) as one plain batch,
                 csc="turbo": idct_kernel (islow) + turbo_rgb_kernel
  jfif           the same batch, csc="jfif" (islow): idct_kernel + csc_kernel
  swscale        the same batch, csc="swscale": bench.py --workload fullres'
                 path, the fused idct_rgb_kernel
  mixed_turbo    spdl_amd.synthetic.mixed_batch(256) (gray, 4:4:4, 4:2:2, odd
                 and even 4:2:0 of several sizes) as one ragged submission at
                 native sizes, csc="turbo"
  mixed_swscale  ... and csc="swscale" (fused-eligible images through
                 idct_rgb_kernel's flat grid, the rest through sws_kernel)

The arms run interleaved, `rounds` times each in one process; an arm's figure
is the median of its rounds, with the minimum and every round beside it.  A
profiled pass at one lane then gives each arm's "idct" and "output" stage
times per batch (spdl_hj_last_timings, synchronous submissions).  Writes one
JSON line per arm and lane count, and a summary line per lane count.  The
first images of the two turbo arms are checked against Pillow.
"""
import argparse
import ctypes
import io
import json
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from spdl_amd import _lib  # noqa: E402
from spdl_amd._lib import Output  # noqa: E402
from spdl_amd.synthetic import mixed_batch, synthetic_slice  # noqa: E402

N = 256
ARMS = {
    "turbo": ("uniform", Output(pix_fmt="rgb24", csc="turbo")),
    "jfif": ("uniform", Output(pix_fmt="rgb24", csc="jfif", idct="islow")),
    "swscale": ("uniform", Output(pix_fmt="rgb24")),
    "mixed_turbo": ("mixed", Output(pix_fmt="rgb24", csc="turbo")),
    "mixed_swscale": ("mixed", Output(pix_fmt="rgb24")),
}


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
    def __init__(self, dec, packed, out, ragged):
        self.dec, self.out = dec, out
        self.dev, self.offs, self.sizes, infos = packed
        self.infos = (_lib.ImageInfo * N)(*infos)
        if ragged:
            self.out_offs, self.boxes, st = _lib.ragged_layout(infos, out, align=256)
            assert not any(st)
        else:  # (a plain batch: one size, image i at i times its bytes)
            self.boxes = [(i.width, i.height) for i in infos]
            assert len(set(self.boxes)) == 1
            self.out_offs = [k * self.boxes[0][0] * self.boxes[0][1] * 3 for k in range(N + 1)]
        self.nbytes = self.out_offs[N]
        self.ragged = (ctypes.c_int64 * N)(*self.out_offs[:N]) if ragged else None
        self.inflight = 2
        self.bufs = [torch.empty(self.nbytes, dtype=torch.uint8, device="cuda:0")
                     for _ in range(self.inflight + 1)]
        self.stream = torch.cuda.current_stream()
        self.k = 0

    def submit(self, sync=False):
        b = self.bufs[self.k % len(self.bufs)]
        self.k += 1
        self.dec.decode_batch_device(self.dev.data_ptr(), self.dev.numel(), self.offs, self.sizes,
                                     self.infos, self.out, b.data_ptr(), self.nbytes,
                                     stream=self.stream, sync=sync, ragged=self.ragged)
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

    def stages(self, steps):
        """{"idct", "output"}: microseconds per batch, synchronous submissions."""
        self.dec.set_profiling(True)
        tot = {}
        for _ in range(steps):
            self.submit(sync=True)
            for s, v in self.dec.last_timings().items():
                tot[s] = tot.get(s, 0.0) + v
        self.dec.set_profiling(False)
        return {s: round(tot[s] / steps, 1) for s in ("idct", "output") if s in tot}

    def image(self, i):
        b = self.bufs[(self.k - 1) % len(self.bufs)]
        w, h = self.boxes[i]
        return b[self.out_offs[i]:self.out_offs[i] + w * h * 3].cpu().numpy().reshape(h, w, 3)


def check(datas, arm, n=8):
    from PIL import Image, features

    if not features.check_feature("libjpeg_turbo"):
        return "not checked: this Pillow is not linked against libjpeg-turbo"
    for i in range(n):
        want = np.asarray(Image.open(io.BytesIO(datas[i])).convert("RGB"))
        np.testing.assert_array_equal(arm.image(i), want)
    return f"the first {n} images of both turbo arms' warm-up batches byte-exact vs Pillow"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("steps", nargs="?", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    datas = {"mixed": mixed_batch(N), "uniform": synthetic_slice(range(N))}
    packed = {k: pack(v) for k, v in datas.items()}
    dec = _lib.Decoder(0)
    dec.set_param("lanes", 0)  # (the library's choice for the hardware queues in effect)
    default_lanes = dec.get_param("lanes")
    lines = []
    for lanes in dict.fromkeys((1, default_lanes)):
        dec.set_param("lanes", lanes)
        arms = {m: Arm(dec, packed[src], out, src == "mixed") for m, (src, out) in ARMS.items()}
        for arm in arms.values():
            arm.run(a.warmup)
        torch.cuda.synchronize()
        checked = check(datas["uniform"], arms["turbo"], 2)
        checked = check(datas["mixed"], arms["mixed_turbo"])
        arms["turbo"].run(1)
        wgs = dec.get_param("turbo_workgroups")
        rates = {m: [] for m in ARMS}
        for _ in range(a.rounds):
            for m in ARMS:
                rates[m].append(arms[m].timed(a.steps))
        med = {m: statistics.median(rates[m]) for m in ARMS}
        stages = {m: arms[m].stages(a.steps) for m in ARMS} if lanes == 1 else {}
        for m in ARMS:
            ln = {"arm": m, "lanes": lanes, "images": N, "steps": a.steps, "rounds": a.rounds,
                  "output_bytes": arms[m].nbytes, "img_per_s_median": round(med[m], 1),
                  "img_per_s_min": round(min(rates[m]), 1),
                  "img_per_s_rounds": [round(r, 1) for r in rates[m]]}
            if m in stages:
                ln["stage_us_per_batch"] = stages[m]
            lines.append(ln)
        lines.append({"summary": True, "lanes": lanes, "turbo_workgroups": wgs,
                      "turbo_over_jfif": round(med["turbo"] / med["jfif"], 4),
                      "turbo_over_swscale": round(med["turbo"] / med["swscale"], 4),
                      "mixed_turbo_over_mixed_swscale":
                          round(med["mixed_turbo"] / med["mixed_swscale"], 4),
                      "checked": checked})
    dec.close()
    for ln in lines:
        print(json.dumps(ln))
    if a.json:
        with open(a.json, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
