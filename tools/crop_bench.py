"""Source crops at RandomResizedCrop's rectangles vs the same batch uncropped
(device-resident, pipelined as bench.py drives it), GPU.

  python tools/crop_bench.py [steps] [--json out.json]

Workload: the 256 bench images (480x640 q90 4:2:0) resident in HBM, stretched
to 224x224 rgb24 u8.  Regions: seeded RandomResizedCrop rectangles (area 0.08-1
of the frame, aspect 3/4-4/3, torchvision's ten tries then the centre
fallback), a new set for every step -- so every batch brings up to 256
geometries the plan cache has not seen.  Both legs run on the same build, with
the library's default lanes, lanes + 2 batches in flight: img/s, the host time
inside the submissions, the IDCT workgroups per batch ("idct_workgroups"), then
per-stage times (spdl_hj_last_timings) from a profiled pass after the timed
one.  The last cropped batch's first images are checked against
tests/src_crop_ref.py.
"""
import argparse
import json
import math
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from spdl_amd import _lib  # noqa: E402
from spdl_amd._lib import Output, Rect  # noqa: E402
from spdl_amd.synthetic import synthetic_slice  # noqa: E402

N, W, H = 256, 640, 480
SPEC = Output(pix_fmt="rgb24", resize=True, fit_w=224, fit_h=224)


def random_resized_crop(rng, w=W, h=H, scale=(0.08, 1.0), ratio=(3 / 4, 4 / 3)):
    """(x, y, w, h) as torchvision's RandomResizedCrop.get_params draws it."""
    for _ in range(10):
        area = w * h * rng.uniform(*scale)
        ar = math.exp(rng.uniform(math.log(ratio[0]), math.log(ratio[1])))
        cw, ch = int(round(math.sqrt(area * ar))), int(round(math.sqrt(area / ar)))
        if 0 < cw <= w and 0 < ch <= h:
            return int(rng.integers(0, w - cw + 1)), int(rng.integers(0, h - ch + 1)), cw, ch
    r = w / h
    cw, ch = (w, int(round(w / ratio[0]))) if r < ratio[0] else \
        (int(round(h * ratio[1])), h) if r > ratio[1] else (w, h)
    return (w - cw) // 2, (h - ch) // 2, cw, ch


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
    infos = (_lib.ImageInfo * len(datas))(*[_lib.get_image_info(d) for d in datas])
    return dev, np.asarray(offs, np.int64), np.asarray(sizes, np.int64), infos


def leg(datas, rects, steps, warmup):
    """One leg: rects is None (whole frames) or a list of per-step Rect arrays."""
    dev, offs, sizes, infos = pack(datas)
    dec = _lib.Decoder(0)
    dec.set_param("lanes", 0)
    lanes = dec.get_param("lanes")
    inflight = min(10, max(2, lanes + 2))
    outs = [torch.empty((N, 224, 224, 3), dtype=torch.uint8, device="cuda:0")
            for _ in range(max(3, inflight))]
    stream = torch.cuda.current_stream()
    k = [0]
    wgs = [0]
    stages = {}

    def submit(sync):
        o = outs[k[0] % len(outs)]
        if rects is not None:
            dec.set_crops(rects[k[0] % len(rects)])
        k[0] += 1
        dec.decode_batch_device(dev.data_ptr(), dev.numel(), offs, sizes, infos, SPEC,
                                o.data_ptr(), o.numel(), stream=stream, sync=sync)
        wgs[0] += dec.get_param("idct_workgroups")
        return dec.last_ticket()

    def run(n):
        pend, host = [], 0.0
        for _ in range(n):
            ts = time.perf_counter()
            pend.append(submit(False))
            host += time.perf_counter() - ts
            if len(pend) > inflight - 1:
                assert not any(dec.wait(pend.pop(0), N))
                for s, v in dec.last_timings().items():
                    stages[s] = stages.get(s, 0.0) + v
        for t in pend:
            assert not any(dec.wait(t, N))
            for s, v in dec.last_timings().items():
                stages[s] = stages.get(s, 0.0) + v
        return host

    for _ in range(lanes):
        submit(True)
    run(max(0, warmup - lanes))
    torch.cuda.synchronize()
    wgs[0] = 0
    t0 = time.perf_counter()
    host = run(steps)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    res = {"lanes": lanes, "inflight": inflight, "steps": steps,
           "img_per_s": round(N * steps / dt, 1), "ms_per_batch": round(dt / steps * 1e3, 4),
           "host_submit_ms": round(host / steps * 1e3, 4),
           "idct_workgroups_per_batch": round(wgs[0] / steps, 1)}
    last_k = k[0] - 1
    last = outs[last_k % len(outs)][:4].cpu().numpy()
    stages.clear()
    dec.set_profiling(True)
    run(steps)
    dec.set_profiling(False)
    res["stages_ms"] = {s: round(v / steps / 1e3, 4) for s, v in stages.items()}
    dec.close()
    return res, last, last_k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("steps", nargs="?", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    datas = synthetic_slice(range(N))
    rng = np.random.default_rng(a.seed)
    nsets = a.steps * 2 + a.warmup + 8  # warm-up, timed and profiled passes: no set twice
    tuples = [[random_resized_crop(rng) for _ in range(N)] for _ in range(nsets)]
    rects = [(Rect * N)(*[Rect(*t) for t in ts]) for ts in tuples]
    out = {"workload": f"{N} x 480x640 q90 4:2:0 in HBM -> stretch 224x224 rgb24 u8"}
    out["uncropped"], _, _ = leg(datas, None, a.steps, a.warmup)
    out["cropped"], last, last_k = leg(datas, rects, a.steps, a.warmup)
    from oracle import oracle as O
    from tests import src_crop_ref as ref

    for i in range(last.shape[0]):
        r = ref.resolve_data(datas[i], tuples[last_k % nsets][i])
        np.testing.assert_array_equal(last[i], ref.rgb(datas[i], r, O.Resize(fit_w=224, fit_h=224)))
    out["checked"] = f"{last.shape[0]} images of the last cropped batch bit-exact vs tests/src_crop_ref.py"
    c, u = out["cropped"], out["uncropped"]
    out["cropped_over_uncropped"] = round(c["img_per_s"] / u["img_per_s"], 3)
    dev_ms = sum(v for s, v in c["stages_ms"].items() if s not in ("h2d", "d2h_status"))
    # the host side of a cropped batch (256 new plans) against the batch's
    # device time (its stages end to end) and its share of the pipelined step
    out["cropped_device_ms_per_batch"] = round(dev_ms, 4)
    out["host_planning_exceeds_device_time"] = bool(c["host_submit_ms"] > dev_ms)
    out["host_submit_share_of_step"] = round(c["host_submit_ms"] / c["ms_per_batch"], 3)
    print(json.dumps(out))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
