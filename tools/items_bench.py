"""Resample items: one items submission against today's spellings, GPU.

  python tools/items_bench.py [steps] [--rounds R] [--warmup W] [--json out.jsonl]

256 images resident in HBM, csc="turbo", rgb24 u8, synchronous submissions, at
one lane and at four.  Three cases, each `items` against `plain`:

  multicrop   2 x 224 + 6 x 96 bicubic crops of every bench image: one items
              submission against the same eight outputs as eight resampled
              submissions (spdl_hj_set_resample with boxes)
  thumbnail   pil_thumbnail((128, 128)) of mixed_batch(256): one items
              submission against one box submission per distinct thumbnail
              size, each over the files of that size
  whole       one item per bench image, whole frame into 224 x 224 bicubic,
              against the plain resampled submission; `whole_flip` is the
              items arm with every second item mirrored

The arms run interleaved, `rounds` times each; a figure is the median of its
rounds in output images per second, with every round beside it.
"""
import argparse
import json
import random
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
from spdl_amd import _lib  # noqa: E402
from spdl_amd._lib import Output, Resample, ResampleItems  # noqa: E402
from spdl_amd.io import pil_thumbnail  # noqa: E402
from spdl_amd.synthetic import mixed_batch, synthetic_slice  # noqa: E402
from tools.turbo_bench import pack  # noqa: E402

N = 256
TURBO = Output(pix_fmt="rgb24", csc="turbo")


class Sub:
    """One submission over images `which` of a packed set, with its keywords."""

    def __init__(self, dec, packed, which, nbytes, **kw):
        dev, offs, sizes, infos = packed
        self.dec, self.dev, self.kw = dec, dev, kw
        self.offs, self.sizes = [offs[i] for i in which], [sizes[i] for i in which]
        self.infos = (_lib.ImageInfo * len(which))(*[infos[i] for i in which])
        self.dst = torch.empty((nbytes,), dtype=torch.uint8, device="cuda:0")
        self.stream = torch.cuda.current_stream()

    def step(self):
        st = self.dec.decode_batch_device(self.dev.data_ptr(), self.dev.numel(), self.offs, self.sizes,
                                          self.infos, TURBO, self.dst.data_ptr(), self.dst.numel(),
                                          stream=self.stream, sync=True, **self.kw)
        assert not any(st)


def packed_items(filt, reqs, gap=None):
    """(ResampleItems, bytes) of (image, box, clamp, size, flip) requests packed 256 bytes apart"""
    items, end = [], 0
    for image, box, clamp, (w, h), flip in reqs:
        items.append((image, box, clamp, (w, h), (0, 0), (w, h), flip, end))
        end = (end + w * h * 3 + 255) // 256 * 256
    return ResampleItems(filt, items, gap), end


def cases(dec):
    bench, mixed = pack(list(synthetic_slice(range(N)))), pack(mixed_batch(N))
    every = list(range(N))
    rng = random.Random(24)

    def crop(info, lo, hi):  # (RandomResizedCrop's box, (x, y, w, h), aspect 3/4 .. 4/3)
        area = rng.uniform(lo, hi) * info.width * info.height
        ratio = rng.uniform(3 / 4, 4 / 3)
        w = max(8, min(info.width, int(round((area * ratio) ** 0.5))))
        h = max(8, min(info.height, int(round((area / ratio) ** 0.5))))
        return rng.randint(0, info.width - w), rng.randint(0, info.height - h), w, h

    crops = [[crop(i, 0.4, 1.0) for _ in range(2)] + [crop(i, 0.05, 0.4) for _ in range(6)]
             for i in bench[3]]
    side = [224, 224, 96, 96, 96, 96, 96, 96]
    items, nbytes = packed_items("bicubic", [(i, (x, y, x + w, y + h), True, (side[k], side[k]), 0)
                                             for i in every for k, (x, y, w, h) in enumerate(crops[i])])
    plain = [Sub(dec, bench, every, N * side[k] ** 2 * 3,
                 resample=Resample("bicubic", side[k], side[k],
                                   tuple((crops[i][k], (side[k], side[k]), (0, 0)) for i in every)))
             for k in range(8)]
    yield "multicrop", 8 * N, {"items": [Sub(dec, bench, every, nbytes, resample_items=items)],
                               "plain": plain}

    thumb = pil_thumbnail((128, 128))
    plans = [thumb.plan(i.width, i.height) for i in mixed[3]]
    levels = [p[0] for p in plans]
    items, nbytes = packed_items("bicubic", [(i, p[2], False, p[1], 0) for i, p in enumerate(plans)],
                                 thumb.reducing_gap)
    plain = []
    for size in sorted({p[1] for p in plans}):
        which = [i for i in every if plans[i][1] == size]
        rs = Resample("bicubic", *size, tuple((plans[i][2], size, (0, 0)) for i in which), True,
                      thumb.reducing_gap)
        plain.append(Sub(dec, mixed, which, len(which) * size[0] * size[1] * 3, resample=rs,
                         draft=[levels[i] for i in which]))
    yield "thumbnail", N, {"items": [Sub(dec, mixed, every, nbytes, resample_items=items, draft=levels)],
                           "plain": plain}

    arms = {"plain": [Sub(dec, bench, every, N * 224 * 224 * 3, resample=Resample("bicubic", 224, 224))]}
    for name, flips in (("items", [0] * N), ("items_flip", [i & 1 for i in every])):
        items, nbytes = packed_items("bicubic", [(i, None, False, (224, 224), flips[i]) for i in every])
        arms[name] = [Sub(dec, bench, every, nbytes, resample_items=items)]
    yield "whole", N, arms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("steps", nargs="?", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dec = _lib.Decoder(0)
    lines = []
    for lanes in (1, 4):
        dec.set_param("lanes", lanes)
        for case, outputs, arms in cases(dec):
            rates = {k: [] for k in arms}
            for subs in arms.values():
                for _ in range(a.warmup):
                    for s in subs:
                        s.step()
            for _ in range(a.rounds):
                for k, subs in arms.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(a.steps):
                        for s in subs:
                            s.step()
                    torch.cuda.synchronize()
                    rates[k].append(outputs * a.steps / (time.perf_counter() - t0))
            med = {k: statistics.median(v) for k, v in rates.items()}
            lines.append({"case": case, "lanes": lanes, "outputs": outputs, "steps": a.steps,
                          "submissions": {k: len(v) for k, v in arms.items()},
                          "out_per_s_median": {k: round(v, 1) for k, v in med.items()},
                          "out_per_s_rounds": {k: [round(r, 1) for r in v] for k, v in rates.items()},
                          "over_plain": {k: round(med[k] / med["plain"], 4) for k in med if k != "plain"}})
            print(json.dumps(lines[-1]), flush=True)
    dec.close()
    if a.json:
        with open(a.json, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
