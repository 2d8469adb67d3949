"""Eight views of every image from one decode (spdl_hj_set_views) against the
same outputs made by submitting every image once per output, GPU.

  python tools/views_bench.py --mode views  [--json out.json]
  python tools/views_bench.py --mode repeat [--json out.json]

Workload: 32 bench images (480x640 q90 4:2:0) resident in HBM.  Of every image
two RandomResizedCrop rectangles (area 0.08-1, aspect 3/4-4/3) stretched to
224x224 and six smaller ones (area 0.05-0.3) stretched to 96x96, rgb24 u8: 256
outputs per batch.  The rectangles come from one seed and are the same in
every batch, so their 256 plans stay in the plan cache (512) and the host's
planning does not hide the device ("Source crop").

  views   one submission with two groups (64 views -> 224, 192 views -> 96)
  repeat  what a library without views can do: two decode_batch_device
          submissions with crops=, the images repeated 2x at 224 and 6x at 96.
          It uses no call newer than the source crop, so it runs from a
          checkout of an older commit as well:
            cd <older checkout> && python <this tree>/tools/views_bench.py --mode repeat

Reported: with one lane and synchronous batches, the library's stage timers
summed per batch (parse + destuff + entropy + idct + tables + output; for
`repeat` over both submissions): median and p10-p90 over --steps batches.
Then pipelined (four lanes, six batches in flight): outputs per second and the
host time inside the submissions.  The entropy work items per batch
("entropy_workgroups"; a build without that parameter decodes every submitted
image in one workgroup at these file sizes, so the images submitted are
reported).  In `views` mode the first rows of both groups are checked against
tests/src_crop_ref.py.
"""
import argparse
import json
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from spdl_amd import _lib  # noqa: E402
from spdl_amd._lib import Output  # noqa: E402
from spdl_amd.synthetic import synthetic_slice  # noqa: E402

sys.path.insert(0, __file__.rsplit("/", 1)[0])
from crop_bench import random_resized_crop  # noqa: E402

N, BIG, SMALL = 32, 2, 6
S224 = Output(pix_fmt="rgb24", resize=True, fit_w=224, fit_h=224)
S96 = Output(pix_fmt="rgb24", resize=True, fit_w=96, fit_h=96)
DEVICE_STAGES = ("parse", "destuff", "entropy", "idct", "tables", "output")


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


class Views:
    """One submission, two groups."""

    def __init__(self, dec, datas, big, small, nbuf):
        self.dec, self.src = dec, pack(datas)
        self.v224 = [(i, r) for i in range(N) for r in big[i]]
        self.v96 = [(i, r) for i in range(N) for r in small[i]]
        self.bufs = [(torch.empty((len(self.v224), 224, 224, 3), dtype=torch.uint8, device="cuda:0"),
                      torch.empty((len(self.v96), 96, 96, 3), dtype=torch.uint8, device="cuda:0"))
                     for _ in range(nbuf)]
        self.groups = [[_lib.ViewGroup(S224, self.v224, a.data_ptr(), a.numel()),
                        _lib.ViewGroup(S96, self.v96, b.data_ptr(), b.numel())]
                       for a, b in self.bufs]
        self.k = 0

    def submit(self, sync, stream):
        g = self.groups[self.k % len(self.groups)]
        self.k += 1
        dev, offs, sizes, infos = self.src
        self.dec.decode_batch_device(dev.data_ptr(), dev.numel(), offs, sizes, infos, S224, 0, 0,
                                     stream=stream, sync=sync, views=g)
        return [(self.dec.last_ticket(), N)]

    def work_items(self):
        return self.dec.get_param("entropy_workgroups")


class Repeat:
    """Two submissions with crops=: every image once per output."""

    def __init__(self, dec, datas, big, small, nbuf):
        self.dec = dec
        self.legs = []
        for spec, rects, size in ((S224, big, 224), (S96, small, 96)):
            rep = [d for i, d in enumerate(datas) for _ in rects[i]]
            crops = (_lib.Rect * len(rep))(*[_lib.Rect(*r) for i in range(N) for r in rects[i]])
            outs = [torch.empty((len(rep), size, size, 3), dtype=torch.uint8, device="cuda:0")
                    for _ in range(nbuf)]
            self.legs.append((spec, pack(rep), crops, outs, len(rep)))
        self.k = 0
        self.items = 0

    def submit(self, sync, stream):
        tickets = []
        self.items = 0
        for spec, (dev, offs, sizes, infos), crops, outs, n in self.legs:
            o = outs[self.k % len(outs)]
            self.dec.set_crops(crops)
            self.dec.decode_batch_device(dev.data_ptr(), dev.numel(), offs, sizes, infos, spec,
                                         o.data_ptr(), o.numel(), stream=stream, sync=sync)
            tickets.append((self.dec.last_ticket(), n))
            try:
                self.items += self.dec.get_param("entropy_workgroups")
            except ValueError:  # a build from before the parameter: one workgroup per image
                self.items += n
        self.k += 1
        return tickets

    def work_items(self):
        return self.items


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("views", "repeat"), required=True)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    datas = synthetic_slice(range(N))
    rng = np.random.default_rng(a.seed)
    big = [[random_resized_crop(rng) for _ in range(BIG)] for _ in range(N)]
    small = [[random_resized_crop(rng, scale=(0.05, 0.3)) for _ in range(SMALL)] for _ in range(N)]
    stream = torch.cuda.current_stream()
    out = {"mode": a.mode, "steps": a.steps,
           "workload": f"{N} x 480x640 q90 4:2:0 in HBM, {BIG} views -> 224x224 and {SMALL} -> "
                       f"96x96 of each, rgb24 u8: {N * (BIG + SMALL)} outputs per batch"}

    # ---- one lane, synchronous batches, the stage timers ----
    dec = _lib.Decoder(0)
    dec.set_param("lanes", 1)
    w = (Views if a.mode == "views" else Repeat)(dec, datas, big, small, 2)
    for _ in range(a.warmup):
        w.submit(True, stream)
    out["entropy_workgroups_per_batch"] = int(w.work_items())
    dec.set_profiling(True)
    sums, per_stage = [], {s: [] for s in DEVICE_STAGES}
    for _ in range(a.steps):
        st = dict.fromkeys(DEVICE_STAGES, 0.0)
        # (a synchronous submission's timings are read before the next one)
        if a.mode == "views":
            w.submit(True, stream)
            t = dec.last_timings()
            for s in DEVICE_STAGES:
                st[s] += t.get(s, 0.0)
        else:
            for spec, (dev, offs, sizes, infos), crops, outs, n in w.legs:
                dec.set_crops(crops)
                dec.decode_batch_device(dev.data_ptr(), dev.numel(), offs, sizes, infos, spec,
                                        outs[0].data_ptr(), outs[0].numel(), stream=stream,
                                        sync=True)
                t = dec.last_timings()
                for s in DEVICE_STAGES:
                    st[s] += t.get(s, 0.0)
        sums.append(sum(st.values()) / 1e3)
        for s in DEVICE_STAGES:
            per_stage[s].append(st[s] / 1e3)
    dec.set_profiling(False)
    q = np.percentile(np.asarray(sums), [10, 50, 90])
    out["stage_sum_ms"] = {"median": round(float(q[1]), 4), "p10": round(float(q[0]), 4),
                           "p90": round(float(q[2]), 4)}
    out["stages_ms_median"] = {s: round(float(np.median(v)), 4) for s, v in per_stage.items()}
    if a.mode == "views":
        from oracle import oracle as O
        from tests import src_crop_ref as ref

        a224, a96 = w.bufs[(w.k - 1) % len(w.bufs)]
        for rows, views, size in ((a224[:3].cpu().numpy(), w.v224, 224),
                                  (a96[:3].cpu().numpy(), w.v96, 96)):
            for k in range(rows.shape[0]):
                i, r = views[k]
                np.testing.assert_array_equal(
                    rows[k], ref.rgb(datas[i], ref.resolve_data(datas[i], r),
                                     O.Resize(fit_w=size, fit_h=size)))
        out["checked"] = "3 rows of each group bit-exact vs tests/src_crop_ref.py"
    dec.close()

    # ---- pipelined: four lanes, six batches in flight ----
    dec = _lib.Decoder(0)
    dec.set_param("lanes", 4)
    lanes, inflight = dec.get_param("lanes"), 6
    w = (Views if a.mode == "views" else Repeat)(dec, datas, big, small, inflight + 1)

    def run(n):
        pend, host = [], 0.0
        for _ in range(n):
            ts = time.perf_counter()
            pend.append(w.submit(False, stream))
            host += time.perf_counter() - ts
            # (a slot ring of 10: `repeat` holds two tickets per batch)
            while len(pend) > (inflight - 1 if a.mode == "views" else 3):
                for t, m in pend.pop(0):
                    assert not any(dec.wait(t, m))
        for b in pend:
            for t, m in b:
                assert not any(dec.wait(t, m))
        return host

    for _ in range(lanes):
        w.submit(True, stream)
    run(a.warmup)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    host = run(a.steps)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    out["pipelined"] = {"lanes": lanes, "batches_in_flight": inflight if a.mode == "views" else 4,
                        "views_per_s": round(N * (BIG + SMALL) * a.steps / dt, 1),
                        "ms_per_batch": round(dt / a.steps * 1e3, 4),
                        "host_submit_ms": round(host / a.steps * 1e3, 4)}
    out["pipelined"]["host_bound"] = bool(out["pipelined"]["host_submit_ms"] >
                                          0.8 * out["pipelined"]["ms_per_batch"])
    dec.close()
    print(json.dumps(out))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
