"""Pillow-exact resize: resample_kernel against what it replaces, GPU.

  python tools/resample_bench.py [steps] [--rounds R] [--warmup W] [--json out.jsonl]

256 images resident in HBM into 224 x 224 rgb24 u8, for the 256 bench images
(480x640 q90 4:2:0) and for spdl_amd.synthetic.mixed_batch(256), at one lane
and at the lanes the library chooses.  Three spellings:

  resample   csc="turbo" with spdl_hj_set_resample, bilinear: one submission,
             resample_kernel writes the 224 x 224 boxes alone
  interp     what there was before: csc="turbo" at native size (one ragged
             submission for the mixed set), every full-size frame written to
             HBM, then torch.nn.functional.interpolate(mode="bilinear",
             antialias=True) per image.  OTHER PIXELS than Pillow's: the
             comparison is of cost, not of output
  swscale    the default path at 224 (scale + pad, bilinear): the ceiling,
             pinned to FFmpeg, other pixels again

The arms run interleaved, `rounds` times each; an arm's figure is the median
of its rounds with every round beside it.  One JSON line per arm, workload and
lane count, and a summary line with the two ratios.  The first images of the
resample arms are checked against Pillow.
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
import torch.nn.functional as F

sys.path.insert(0, ".")
from spdl_amd import _lib  # noqa: E402
from spdl_amd._lib import Output, Resample  # noqa: E402
from spdl_amd.synthetic import mixed_batch, synthetic_slice  # noqa: E402
from tools.turbo_bench import pack  # noqa: E402

N, SIDE = 256, 224
TURBO = Output(pix_fmt="rgb24", csc="turbo")
SWS = Output(pix_fmt="rgb24", resize=True, fit_w=SIDE, fit_h=SIDE, aspect="decrease", pad_w=SIDE,
             pad_h=SIDE, filter="bilinear")


class Arm:
    def __init__(self, dec, packed, kind):
        self.dec, self.kind = dec, kind
        self.dev, self.offs, self.sizes, infos = packed
        self.infos = (_lib.ImageInfo * N)(*infos)
        self.stream = torch.cuda.current_stream()
        self.small = torch.empty((N, SIDE, SIDE, 3), dtype=torch.uint8, device="cuda:0")
        self.kw, self.out, self.dst = {}, TURBO, self.small
        if kind == "resample":
            self.kw = dict(resample=Resample("bilinear", SIDE, SIDE))
        elif kind == "swscale":
            self.out = SWS
        else:  # native size, ragged (a uniform set packs the same way), then interpolate
            self.out_offs, self.boxes, st = _lib.ragged_layout(infos, TURBO, align=256)
            assert not any(st)
            self.dst = torch.empty(self.out_offs[N], dtype=torch.uint8, device="cuda:0")
            self.kw = dict(ragged=(ctypes.c_int64 * N)(*self.out_offs[:N]))

    def step(self):
        st = self.dec.decode_batch_device(self.dev.data_ptr(), self.dev.numel(), self.offs,
                                          self.sizes, self.infos, self.out, self.dst.data_ptr(),
                                          self.dst.numel(), stream=self.stream, sync=True, **self.kw)
        assert not any(st)
        if self.kind != "interp":
            return
        for i, (w, h) in enumerate(self.boxes):
            o = self.out_offs[i]
            px = self.dst[o:o + w * h * 3].view(1, h, w, 3).permute(0, 3, 1, 2).float()
            y = F.interpolate(px, size=(SIDE, SIDE), mode="bilinear", antialias=True)
            self.small[i] = y.round_().clamp_(0, 255).to(torch.uint8)[0].permute(1, 2, 0)

    def timed(self, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            self.step()
        torch.cuda.synchronize()
        return N * steps / (time.perf_counter() - t0)


def check(datas, arm, n=4):
    from PIL import Image, features

    if not features.check_feature("libjpeg_turbo"):
        return "not checked: this Pillow is not linked against libjpeg-turbo"
    got = arm.small[:n].cpu().numpy()
    for i in range(n):
        im = Image.open(io.BytesIO(datas[i])).convert("RGB").resize((SIDE, SIDE), Image.BILINEAR)
        np.testing.assert_array_equal(got[i], np.asarray(im))
    return f"the first {n} images of the resample arm byte-exact vs Pillow"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("steps", nargs="?", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    datas = {"uniform": synthetic_slice(range(N)), "mixed": mixed_batch(N)}
    packed = {k: pack(v) for k, v in datas.items()}
    dec = _lib.Decoder(0)
    dec.set_param("lanes", 0)  # (the library's choice for the hardware queues in effect)
    default_lanes = dec.get_param("lanes")
    lines = []
    for lanes in dict.fromkeys((1, default_lanes)):
        dec.set_param("lanes", lanes)
        for work in datas:
            arms = {k: Arm(dec, packed[work], k) for k in ("resample", "interp", "swscale")}
            for arm in arms.values():
                for _ in range(a.warmup):
                    arm.step()
            arms["resample"].step()
            checked, wgs = check(datas[work], arms["resample"]), dec.get_param("resample_workgroups")
            rates = {k: [] for k in arms}
            for _ in range(a.rounds):
                for k, arm in arms.items():
                    rates[k].append(arm.timed(a.steps))
            med = {k: statistics.median(v) for k, v in rates.items()}
            for k in arms:
                lines.append({"arm": k, "workload": work, "lanes": lanes, "images": N,
                              "steps": a.steps, "img_per_s_median": round(med[k], 1),
                              "img_per_s_rounds": [round(r, 1) for r in rates[k]]})
            lines.append({"summary": True, "workload": work, "lanes": lanes,
                          "resample_workgroups": wgs,
                          "resample_over_interp": round(med["resample"] / med["interp"], 4),
                          "resample_over_swscale": round(med["resample"] / med["swscale"], 4),
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
