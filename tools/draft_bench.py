"""Pillow-exact draft: the resize of the full decode against the resize of the
draft frame, GPU.

  python tools/draft_bench.py [steps] [--rounds R] [--warmup W] [--json out.jsonl]

256 images resident in HBM into 224 x 224 rgb24 u8 with csc="turbo" and
spdl_hj_set_resample (bilinear), for three workloads -- the 256 bench images
(480x640 q90 4:2:0), spdl_amd.synthetic.mixed_batch(256), and one 12 MP image
among 255 bench images -- at one lane and at the lanes the library chooses.
Two arms:

  level0   the resize of the full-size decode: what there was before
  draft    draft="auto": per image the largest level whose frame covers the
           224 x 224 box (spdl_hj_set_draft), the resize on the draft frame.
           OTHER PIXELS than level0's, as Pillow's are after im.draft()

The arms run interleaved, `rounds` times each; an arm's figure is the median
of its rounds with every round beside it.  One profiled submission per arm
gives the IDCT and output stages' times and "planes_bytes".  The first images
of the draft arm are checked against Pillow.
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
from spdl_amd.synthetic import mixed_batch, synthetic_jpeg, synthetic_slice  # noqa: E402
from tools.turbo_bench import pack  # noqa: E402

N, SIDE = 256, 224
TURBO = Output(pix_fmt="rgb24", csc="turbo")


class Arm:
    def __init__(self, dec, packed, levels):
        self.dec, self.levels = dec, levels
        self.dev, self.offs, self.sizes, infos = packed
        self.infos = (_lib.ImageInfo * N)(*infos)
        self.stream = torch.cuda.current_stream()
        self.dst = torch.empty((N, SIDE, SIDE, 3), dtype=torch.uint8, device="cuda:0")
        self.rs = Resample("bilinear", SIDE, SIDE)

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

    def profile(self):
        """(idct us, output us, planes bytes) of one profiled submission"""
        self.dec.set_profiling(True)
        self.step()
        t = self.dec.last_timings()
        self.dec.set_profiling(False)
        return t.get("idct"), t.get("output"), self.dec.get_param("planes_bytes")


def check(datas, arm, n=4):
    from PIL import Image, features

    if not features.check_feature("libjpeg_turbo"):
        return "not checked: this Pillow is not linked against libjpeg-turbo"
    got = arm.dst[:n].cpu().numpy()
    for i in range(n):
        im = Image.open(io.BytesIO(datas[i]))
        want = _lib.draft_size(*im.size, arm.levels[i])
        im.draft("RGB", tuple(max(v >> arm.levels[i], 1) for v in im.size))
        assert im.size == want, (im.size, want)
        px = np.asarray(im.convert("RGB").resize((SIDE, SIDE), Image.BILINEAR))
        np.testing.assert_array_equal(got[i], px)
    return f"the first {n} images of the draft arm byte-exact vs Pillow"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("steps", nargs="?", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    uniform = list(synthetic_slice(range(N)))
    datas = {"uniform": uniform, "mixed": mixed_batch(N),
             "one_12mp": [synthetic_jpeg(77, 3000, 4000)] + uniform[1:]}
    dec = _lib.Decoder(0)
    dec.set_param("lanes", 0)  # (the library's choice for the hardware queues in effect)
    default_lanes = dec.get_param("lanes")
    lines = []
    for lanes in dict.fromkeys((1, default_lanes)):
        dec.set_param("lanes", lanes)
        for work, files in datas.items():
            packed = pack(files)
            auto = _lib.draft_levels("auto", packed[3], [(SIDE, SIDE)] * N) or [0] * N
            arms = {"level0": Arm(dec, packed, None), "draft": Arm(dec, packed, auto)}
            for arm in arms.values():
                for _ in range(a.warmup):
                    arm.step()
            checked = check(files, arms["draft"])
            rates = {k: [] for k in arms}
            for _ in range(a.rounds):
                for k, arm in arms.items():
                    rates[k].append(arm.timed(a.steps))
            med = {k: statistics.median(v) for k, v in rates.items()}
            for k, arm in arms.items():
                idct_us, out_us, planes = arm.profile()
                lines.append({"arm": k, "workload": work, "lanes": lanes, "images": N,
                              "steps": a.steps, "img_per_s_median": round(med[k], 1),
                              "img_per_s_rounds": [round(r, 1) for r in rates[k]],
                              "idct_us": idct_us, "output_us": out_us, "planes_bytes": planes})
            lines.append({"summary": True, "workload": work, "lanes": lanes,
                          "levels": {str(lv): auto.count(lv) for lv in sorted(set(auto))},
                          "draft_over_level0": round(med["draft"] / med["level0"], 4),
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
