"""Pillow-exact thumbnail: Image.thumbnail on the GPU against its nearest
earlier spelling, and the reduce kernel against the resize it shortens.

  python tools/thumbnail_bench.py [steps] [--rounds R] [--warmup W] [--json out.jsonl]

The 256 bench images (480x640 q90 4:2:0) resident in HBM, rgb24 u8, csc="turbo",
bicubic, four arms:

  thumbnail   pil_thumbnail((128, 128), reducing_gap=2.0): draft level, float
              box and reduce as Image.thumbnail resolves them
  auto        draft="auto" with pil_resize into the same size, integer box, no
              reduce: OTHER PIXELS (what there was before)
  gap         pil_resize((64, 48), reducing_gap=2.0) of the full-size decode:
              factors (5, 5), resample_reduce_kernel
  nogap       the same resize without a gap: resample_kernel, 10 : 1

The arms run interleaved, `rounds` times each; an arm's figure is the median of
its rounds with every round beside it.  The first images of `thumbnail` and
`gap` are checked against Pillow.  mixed_batch is not measured: its files
resolve to several thumbnail sizes, and one submission writes one.
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
from spdl_amd.io import pil_thumbnail  # noqa: E402
from spdl_amd.synthetic import synthetic_slice  # noqa: E402
from tools.turbo_bench import pack  # noqa: E402

N = 256
TURBO = Output(pix_fmt="rgb24", csc="turbo")


class Arm:
    def __init__(self, dec, packed, size, rs, levels):
        self.dec, self.rs, self.levels = dec, rs, levels
        self.dev, self.offs, self.sizes, infos = packed
        self.infos = (_lib.ImageInfo * N)(*infos)
        self.stream = torch.cuda.current_stream()
        self.dst = torch.empty((N, size[1], size[0], 3), dtype=torch.uint8, device="cuda:0")

    def step(self):
        st = self.dec.decode_batch_device(self.dev.data_ptr(), self.dev.numel(), self.offs,
                                          self.sizes, self.infos, TURBO, self.dst.data_ptr(),
                                          self.dst.numel(), stream=self.stream, sync=True,
                                          resample=self.rs, draft=self.levels)
        assert not any(st)

    def timed(self, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            self.step()
        torch.cuda.synchronize()
        return N * steps / (time.perf_counter() - t0)


def main():
    from PIL import Image

    ap = argparse.ArgumentParser()
    ap.add_argument("steps", nargs="?", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    files = list(synthetic_slice(range(N)))
    packed = pack(files)
    infos = packed[3]
    thumb = pil_thumbnail((128, 128), "bicubic", 2.0)
    plans = [thumb.plan(i.width, i.height) for i in infos]
    (final,) = {p[1] for p in plans}
    auto = _lib.draft_levels("auto", infos, [final] * N) or [0] * N
    dec = _lib.Decoder(0)
    arms = {
        "thumbnail": Arm(dec, packed, final,
                         Resample("bicubic", *final, tuple((p[2], final, (0, 0)) for p in plans), True, 2.0),
                         [p[0] for p in plans]),
        "auto": Arm(dec, packed, final, Resample("bicubic", *final), auto),
        "gap": Arm(dec, packed, (64, 48), Resample("bicubic", 64, 48, None, True, 2.0), None),
        "nogap": Arm(dec, packed, (64, 48), Resample("bicubic", 64, 48), None),
    }
    reduced = {}
    for k, arm in arms.items():
        for _ in range(a.warmup):
            arm.step()
        reduced[k] = dec.get_param("reduce_images")
    for k, gap in (("thumbnail", 2.0), ("gap", 2.0)):
        got = arms[k].dst[:4].cpu().numpy()
        for i in range(4):
            im = Image.open(io.BytesIO(files[i]))
            if k == "thumbnail":
                im.thumbnail((128, 128), Image.BICUBIC, reducing_gap=gap)
                im = im.convert("RGB")
            else:
                im = im.convert("RGB").resize((64, 48), Image.BICUBIC, reducing_gap=gap)
            np.testing.assert_array_equal(got[i], np.asarray(im))
    rates = {k: [] for k in arms}
    for _ in range(a.rounds):
        for k, arm in arms.items():
            rates[k].append(arm.timed(a.steps))
    lines = [{"arm": k, "images": N, "steps": a.steps, "out": list(arms[k].dst.shape[1:3]),
              "levels": sorted(set(arms[k].levels or [0])), "reduce_images": reduced[k],
              "img_per_s_median": round(statistics.median(v), 1),
              "img_per_s_rounds": [round(r, 1) for r in v]} for k, v in rates.items()]
    med = {ln["arm"]: ln["img_per_s_median"] for ln in lines}
    lines.append({"summary": True, "thumbnail_over_auto": round(med["thumbnail"] / med["auto"], 4),
                  "gap_over_nogap": round(med["gap"] / med["nogap"], 4),
                  "checked": "the first 4 images of thumbnail and gap byte-exact vs Pillow"})
    dec.close()
    for ln in lines:
        print(json.dumps(ln))
    if a.json:
        with open(a.json, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
