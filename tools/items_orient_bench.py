"""Pillow-exact orientation: oriented resample items against unoriented ones and
against what a pipeline did before them.

  python tools/items_orient_bench.py [steps] [--rounds R] [--warmup W] [--arms a,b] [--json out.jsonl]

The 256 bench images (480x640 q90 4:2:0) resident in HBM, csc="turbo", u8
rgb24, one item per image into 224 x 224 bilinear, at one lane and at the lanes
the library chooses for the hardware queues (four), two batches in flight:

  plain       items without codes: the instantiation from before orientations.
              Run with SPDL_AMD_LIB on the parent commit's library and on this
              build (--arms plain): the two agree within the spread of the
              rounds, or the unoriented instantiation was disturbed
  dealt       the eight codes dealt evenly (image k: code k % 8)
  transposed  every item code 5 (EXIF 6, the phone-portrait tag)
  torch       today's alternative: csc="turbo" at native size, then per image
              a torch permute / flip and a torch bilinear resize (one launch
              chain per image, as sizes differ in a real set; NOT Pillow's bytes)

The arms run interleaved, `rounds` times each, after `warmup` batches of every
arm; an arm's figure is the median of its rounds with every round beside it.
The first images of dealt and transposed are checked against Pillow.
"""
import argparse
import io
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from spdl_amd import _lib  # noqa: E402
from spdl_amd._lib import Output, ResampleItems  # noqa: E402
from spdl_amd.synthetic import synthetic_slice  # noqa: E402
from tools.turbo_bench import pack  # noqa: E402

N, SIZE = 256, (224, 224)
CODES = {"plain": lambda k: 0, "dealt": lambda k: k % 8, "transposed": lambda k: 5, "torch": None}


class Arm:
    def __init__(self, dec, packed, code_of):
        self.dec, self.code_of = dec, code_of
        self.out = Output(pix_fmt="rgb24", csc="turbo")
        self.dev, self.offs, self.sizes, infos = packed
        self.infos = (_lib.ImageInfo * N)(*infos)
        self.stream = torch.cuda.current_stream()
        w, h = SIZE if code_of else (infos[0].width, infos[0].height)
        self.items = None
        if code_of:
            per = w * h * 3
            rows = [(k, None, False, SIZE, (0, 0), SIZE, 0, k * per) for k in range(N)]
            if any(code_of(k) for k in range(N)):  # (plain: the tuple every earlier build takes)
                rows = [(*r, code_of(k)) for k, r in enumerate(rows)]
            self.items = ResampleItems("bilinear", rows)
        self.inflight = 2
        self.bufs = [torch.empty((N, h, w, 3), dtype=torch.uint8, device="cuda:0")
                     for _ in range(self.inflight + 1)]
        self.k = 0

    def submit(self):
        b = self.bufs[self.k % len(self.bufs)]
        self.k += 1
        self.dec.decode_batch_device(self.dev.data_ptr(), self.dev.numel(), self.offs, self.sizes,
                                     self.infos, self.out, b.data_ptr(), b.numel(),
                                     stream=self.stream, sync=False, resample_items=self.items)
        return self.dec.last_ticket(), b

    def finish(self, ticket, b):
        assert not any(self.dec.wait(ticket, N))
        if self.code_of is None:  # (per image: its own code, as its own size would force)
            outs = []
            for k in range(N):
                t, c = b[k].permute(2, 0, 1), k % 8
                t = t.transpose(1, 2) if c & 4 else t
                t = t.flip(2) if c & 1 else t
                t = t.flip(1) if c & 2 else t
                outs.append(torch.nn.functional.interpolate(t[None].float(), size=SIZE[::-1],
                                                            mode="bilinear", antialias=True))
            self.result = torch.cat(outs).round().to(torch.uint8)

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

    method = {1: 0, 2: 1, 3: 3, 4: 5, 5: 4, 6: 2, 7: 6}  # (code -> Image.Transpose value)
    done = []
    for name in ("dealt", "transposed"):
        if name not in arms:
            continue
        got = arms[name].bufs[(arms[name].k - 1) % 3][:8].cpu().numpy()
        for i in range(8):
            im, c = Image.open(io.BytesIO(files[i])).convert("RGB"), CODES[name](i)
            im = im.transpose(Image.Transpose(method[c])) if c else im
            np.testing.assert_array_equal(got[i], np.asarray(im.resize(SIZE, Image.BILINEAR)))
        done.append(name)
    return f"the first 8 images of {done} byte-exact vs Pillow"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("steps", nargs="?", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--arms", default=",".join(CODES))
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
        arms = {k: Arm(dec, packed, CODES[k]) for k in a.arms.split(",")}
        wgs = {}
        for k, arm in arms.items():
            arm.run(a.warmup)
            wgs[k] = dec.get_param("resample_item_workgroups")
        checked = check(files, arms)
        rates = {k: [] for k in arms}
        for _ in range(a.rounds):
            for k, arm in arms.items():
                rates[k].append(arm.timed(a.steps))
        for k, v in rates.items():
            lines.append({"arm": k, "lanes": lanes, "images": N, "steps": a.steps, "warmup": a.warmup,
                          "resample_item_workgroups": wgs[k],
                          "img_per_s_median": round(statistics.median(v), 1),
                          "img_per_s_rounds": [round(r, 1) for r in v]})
        lines.append({"summary": True, "lanes": lanes, "lib": os.path.basename(_lib.LIB_PATH), "checked": checked})
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
