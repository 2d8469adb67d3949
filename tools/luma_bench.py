"""Pillow-exact grayscale: pix_fmt "L" and "Y" against rgb24 on the same build.

  python tools/luma_bench.py [steps] [--rounds R] [--warmup W] [--json out.jsonl]

The 256 bench images (480x640 q90 4:2:0) resident in HBM, csc="turbo", u8, at
one lane and at the lanes the library chooses for the hardware queues (four),
two batches in flight; seven arms:

  rgb24 / L / Y              native size (turbo_rgb_kernel<3> / <1>)
  rgb24_224 / L_224 / Y_224  pil_resize((224, 224), "bilinear") (resample_kernel<., 3> / <., 1>)
  torch                      rgb24 at native size, then the luma as a torch pass
                             over the batch (float weights: NOT Pillow's bytes)
                             -- what a pipeline did before these formats

The arms run interleaved, `rounds` times each, after `warmup` batches of every
arm; an arm's figure is the median of its rounds with every round beside it,
so the spread is on the page.  The first images of the four gray arms are
checked against Pillow.  Not measured here: f16 / bf16, ragged submissions.
"""
import argparse
import io
import json
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from spdl_amd import _lib  # noqa: E402
from spdl_amd._lib import Output, Resample  # noqa: E402
from spdl_amd.synthetic import synthetic_slice  # noqa: E402
from tools.turbo_bench import pack  # noqa: E402

N = 256
ARMS = {"rgb24": ("rgb24", None), "L": ("L", None), "Y": ("Y", None),
        "rgb24_224": ("rgb24", (224, 224)), "L_224": ("L", (224, 224)), "Y_224": ("Y", (224, 224)),
        "torch": ("rgb24", None)}


class Arm:
    def __init__(self, dec, packed, fmt, size, torch_pass=False):
        self.dec, self.torch_pass = dec, torch_pass
        self.out = Output(pix_fmt=fmt, csc="turbo")
        self.rs = Resample("bilinear", *size) if size else None
        self.dev, self.offs, self.sizes, infos = packed
        self.infos = (_lib.ImageInfo * N)(*infos)
        self.stream = torch.cuda.current_stream()
        w, h = size or (infos[0].width, infos[0].height)
        self.inflight = 2
        self.bufs = [torch.empty((N, h, w, self.out.channels), dtype=torch.uint8, device="cuda:0")
                     for _ in range(self.inflight + 1)]
        self.weights = torch.tensor([0.299, 0.587, 0.114], device="cuda:0")
        self.k = 0

    def submit(self):
        b = self.bufs[self.k % len(self.bufs)]
        self.k += 1
        self.dec.decode_batch_device(self.dev.data_ptr(), self.dev.numel(), self.offs, self.sizes,
                                     self.infos, self.out, b.data_ptr(), b.numel(),
                                     stream=self.stream, sync=False, resample=self.rs)
        return self.dec.last_ticket(), b

    def finish(self, ticket, b):
        assert not any(self.dec.wait(ticket, N))
        if self.torch_pass:
            self.gray = (b.float() @ self.weights).round().to(torch.uint8)

    def run(self, n):
        pend = []
        for _ in range(n):
            pend.append(self.submit())
            if len(pend) > self.inflight - 1:
                self.finish(*pend.pop(0))
        for t in pend:
            self.finish(*t)

    def timed(self, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        self.run(steps)
        torch.cuda.synchronize()
        return N * steps / (time.perf_counter() - t0)


def check(files, arms):
    from PIL import Image

    for k in ("L", "Y", "L_224", "Y_224"):
        got = arms[k].bufs[(arms[k].k - 1) % 3][:4].cpu().numpy()
        for i in range(4):
            im = Image.open(io.BytesIO(files[i]))
            if k[0] == "Y":
                im.draft("L", im.size)
            im = im.convert("L")
            if k.endswith("224"):
                im = im.resize((224, 224), Image.BILINEAR)
            np.testing.assert_array_equal(got[i][..., 0], np.asarray(im))
    return "the first 4 images of L, Y, L_224 and Y_224 byte-exact vs Pillow"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("steps", nargs="?", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    files = list(synthetic_slice(range(N)))
    packed = pack(files)
    dec = _lib.Decoder(0)
    dec.set_param("lanes", 0)  # (the library's choice for the hardware queues in effect)
    default_lanes = dec.get_param("lanes")
    lines = []
    for lanes in dict.fromkeys((1, default_lanes)):
        dec.set_param("lanes", lanes)
        arms = {k: Arm(dec, packed, fmt, size, k == "torch") for k, (fmt, size) in ARMS.items()}
        figures = {}
        for k, arm in arms.items():
            arm.run(a.warmup)
            figures[k] = (dec.get_param("planes_bytes"), dec.get_param("idct_workgroups"))
        checked = check(files, arms)
        rates = {k: [] for k in arms}
        for _ in range(a.rounds):
            for k, arm in arms.items():
                rates[k].append(arm.timed(a.steps))
        med = {k: statistics.median(v) for k, v in rates.items()}
        for k, v in rates.items():
            lines.append({"arm": k, "lanes": lanes, "images": N, "steps": a.steps, "warmup": a.warmup,
                          "planes_bytes": figures[k][0], "idct_workgroups": figures[k][1],
                          "img_per_s_median": round(med[k], 1),
                          "img_per_s_rounds": [round(r, 1) for r in v]})
        lines.append({"summary": True, "lanes": lanes,
                      **{f"{k}_over_rgb24": round(med[k] / med["rgb24"], 4) for k in ("L", "Y", "torch")},
                      **{f"{k}_over_rgb24_224": round(med[k] / med["rgb24_224"], 4)
                         for k in ("L_224", "Y_224")}, "checked": checked})
        del arms
    dec.close()
    for ln in lines:
        print(json.dumps(ln))
    if a.json:
        with open(a.json, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
