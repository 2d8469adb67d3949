"""Output-stage time of the planar format next to rgb24.

The 256 bench images (480x640 q90 4:2:0, already in HBM) -> 224x224 pad, one
lane, synchronous batches, the library's own stage timers (HIP events on the
decode stream): `pix_fmt="yuv"` (yuv_planes_kernel) and `pix_fmt="rgb24"`
(sws_kernel) alternate batch by batch on one build; prints the median and the
spread of the "output" stage and of the whole batch for both, as one JSON line.

    python tools/yuv_output_stage.py [--reps 200]
"""

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from spdl_amd import _lib  # noqa: E402
from spdl_amd._lib import Output  # noqa: E402
from spdl_amd.synthetic import synthetic_slice  # noqa: E402

PAD224 = dict(resize=True, fit_w=224, fit_h=224, aspect="decrease", pad_w=224, pad_h=224)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    datas = synthetic_slice(range(256), distinct=32)
    offs, sizes, total = [], [], 0
    for d in datas:
        offs.append(total)
        sizes.append(len(d))
        total += (len(d) + 64 + 255) // 256 * 256
    host = np.zeros(total, np.uint8)
    for o, d in zip(offs, datas):
        host[o:o + len(d)] = np.frombuffer(d, np.uint8)
    dev = torch.from_numpy(host).to("cuda:0")
    infos = (_lib.ImageInfo * len(datas))(*[_lib.get_image_info(d) for d in datas])
    offs, sizes = np.asarray(offs, np.int64), np.asarray(sizes, np.int64)
    dec = _lib.Decoder(0)
    dec.set_param("lanes", 1)
    dec.set_profiling(True)
    n = len(datas)
    specs = {"yuv": (Output(pix_fmt="yuv", **PAD224), 224 * 224 * 3 // 2),
             "rgb24": (Output(pix_fmt="rgb24", **PAD224), 224 * 224 * 3)}
    outs = {k: torch.empty(n * per, dtype=torch.uint8, device="cuda:0")
            for k, (_, per) in specs.items()}
    stream = torch.cuda.current_stream()
    times = {k: {"output": [], "batch": []} for k in specs}
    for rep in range(args.warmup + args.reps):
        for k, (spec, per) in specs.items():
            dec.decode_batch_device(dev.data_ptr(), dev.numel(), offs, sizes, infos, spec,
                                    outs[k].data_ptr(), n * per, stream=stream, sync=True)
            t = dec.last_timings()
            if rep >= args.warmup:
                times[k]["output"].append(t["output"])
                times[k]["batch"].append(sum(v for s, v in t.items() if s != "h2d"))
    res = {"images": n, "reps": args.reps, "out_bytes": {k: per for k, (_, per) in specs.items()}}
    for k in specs:
        for what, v in times[k].items():
            q = np.percentile(np.asarray(v), [10, 50, 90])
            res[f"{k}_{what}_us"] = {"p10": round(float(q[0]), 1), "median": round(float(q[1]), 1),
                                     "p90": round(float(q[2]), 1)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
