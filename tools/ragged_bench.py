"""Ragged batches: one submission of images of many sizes against what a caller
had to do before, and against the kernels a plain batch runs, GPU.

  python tools/ragged_bench.py [steps] [--rounds R] [--warmup W] [--json out.jsonl]

256 images resident in HBM, decoded at native size to rgb24 u8 into one packed
buffer (spdl_hj_ragged_layout, 256-byte alignment).  Five arms, at one lane
and at the lanes the library chooses for the hardware queues in effect:

  ragged         spdl_amd.synthetic.mixed_batch(256) (gray, 4:4:4, 4:2:2, odd
                 and even 4:2:0 of several sizes) as one ragged submission:
                 fused-eligible images through idct_rgb_kernel's flat grid,
                 the rest through idct_kernel + sws_kernel
  singles        the same images as 256 single-image submissions on the same
                 context, each into its place in the same buffer -- the only
                 spelling before ragged batches
  ragged_path1   `ragged` with "output_path" 1: every image through the
                 generic kernel (no per-image split)
  uniform_ragged the 256 bench images (480x640 q90 4:2:0), submitted ragged
                 (every image eligible: the fused kernel's flat grid alone)
  uniform_plain  ... and as the plain batch they also are ([256, 480, 640, 3];
                 idct_rgb_kernel's (tile, image) grid)

The arms run interleaved, `rounds` times each in one process; an arm's figure
is the median of its rounds, with the minimum and every round beside it.
Writes one JSON line per arm and lane count, and a summary line per lane
count.  The first images of `ragged` are checked against the oracle.
"""
import argparse
import ctypes
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
OUT = Output(pix_fmt="rgb24")
ARMS = ("ragged", "singles", "ragged_path1", "uniform_ragged", "uniform_plain")


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
    def __init__(self, dec, packed, mode):
        self.dec, self.mode = dec, mode
        self.dev, self.offs, self.sizes, infos = packed
        self.infos = (_lib.ImageInfo * N)(*infos)
        self.one = [(_lib.ImageInfo * 1)(i) for i in infos]
        self.out_offs, self.boxes, st = _lib.ragged_layout(infos, OUT, align=256)
        assert not any(st)
        self.nbytes = self.out_offs[N]
        self.ragged = (ctypes.c_int64 * N)(*self.out_offs[:N])
        self.extent = [w * h * 3 for w, h in self.boxes]
        self.inflight = 2
        self.bufs = [torch.empty(self.nbytes, dtype=torch.uint8, device="cuda:0")
                     for _ in range(self.inflight + 1)]
        self.stream = torch.cuda.current_stream()
        self.k = 0

    def submit(self):
        b = self.bufs[self.k % len(self.bufs)]
        self.k += 1
        dec, dev = self.dec, self.dev
        if self.mode == "singles":
            tickets = []
            for i in range(N):
                dec.decode_batch_device(dev.data_ptr(), dev.numel(), self.offs[i:i + 1],
                                        self.sizes[i:i + 1], self.one[i], OUT,
                                        b.data_ptr() + self.out_offs[i], self.extent[i],
                                        stream=self.stream, sync=False)
                tickets.append(dec.last_ticket())
                # (the ring holds ten batches and reuses a finished one's slot,
                # waited for or not: seven in flight, all waited for before the
                # step ends)
                if len(tickets) > 6:
                    assert not any(dec.wait(tickets.pop(0), 1))
            for t in tickets:
                assert not any(dec.wait(t, 1))
            return None
        dec.set_param("output_path", 1 if self.mode == "ragged_path1" else 0)
        ragged = None if self.mode == "uniform_plain" else self.ragged
        dec.decode_batch_device(dev.data_ptr(), dev.numel(), self.offs, self.sizes, self.infos, OUT,
                                b.data_ptr(), self.nbytes, stream=self.stream, sync=False,
                                ragged=ragged)
        return dec.last_ticket(), N

    def run(self, n):
        pend = []
        for _ in range(n):
            t = self.submit()
            if t is None:
                continue
            pend.append(t)
            if len(pend) > self.inflight - 1:
                t, k = pend.pop(0)
                assert not any(self.dec.wait(t, k))
        for t, k in pend:
            assert not any(self.dec.wait(t, k))

    def timed(self, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        self.run(steps)
        torch.cuda.synchronize()
        return N * steps / (time.perf_counter() - t0)

    def image(self, i):
        b = self.bufs[(self.k - 1) % len(self.bufs)]
        w, h = self.boxes[i]
        return b[self.out_offs[i]:self.out_offs[i] + self.extent[i]].cpu().numpy().reshape(h, w, 3)


def check(datas, arm, n=8):
    from oracle import oracle as O

    for i in range(n):
        np.testing.assert_array_equal(arm.image(i), O.decode_rgb(datas[i], O.IDCT_SIMPLE, "rgb24"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("steps", nargs="?", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    mixed, uniform = mixed_batch(N), synthetic_slice(range(N))
    pm, pu = pack(mixed), pack(uniform)
    dec = _lib.Decoder(0)
    dec.set_param("lanes", 0)  # (the library's choice for the hardware queues in effect)
    default_lanes = dec.get_param("lanes")
    lines = []
    for lanes in dict.fromkeys((1, default_lanes)):
        dec.set_param("lanes", lanes)
        arms = {m: Arm(dec, pu if m.startswith("uniform") else pm, m) for m in ARMS}
        for arm in arms.values():
            arm.run(a.warmup)
        torch.cuda.synchronize()
        for m in ("ragged", "singles", "ragged_path1"):
            check(mixed, arms[m])
        for m in ("uniform_ragged", "uniform_plain"):
            check(uniform, arms[m], 2)
        arms["ragged"].run(1)
        split = {"fused_workgroups": dec.get_param("fused_workgroups"),
                 "generic_workgroups": dec.get_param("generic_workgroups")}
        rates = {m: [] for m in ARMS}
        for _ in range(a.rounds):
            for m in ARMS:
                rates[m].append(arms[m].timed(a.steps))
        med = {m: statistics.median(rates[m]) for m in ARMS}
        for m in ARMS:
            lines.append({"arm": m, "lanes": lanes, "images": N, "steps": a.steps,
                          "rounds": a.rounds, "output_bytes": arms[m].nbytes,
                          "img_per_s_median": round(med[m], 1),
                          "img_per_s_min": round(min(rates[m]), 1),
                          "img_per_s_rounds": [round(r, 1) for r in rates[m]]})
        lines.append({"summary": True, "lanes": lanes, "ragged_split": split,
                      "ragged_over_singles": round(med["ragged"] / med["singles"], 4),
                      "ragged_over_ragged_path1": round(med["ragged"] / med["ragged_path1"], 4),
                      "uniform_ragged_over_uniform_plain":
                          round(med["uniform_ragged"] / med["uniform_plain"], 4),
                      "checked": "the first images of every arm's warm-up batch bit-exact vs "
                                 "the oracle"})
    dec.set_param("output_path", 0)
    dec.close()
    for ln in lines:
        print(json.dumps(ln))
    if a.json:
        with open(a.json, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
