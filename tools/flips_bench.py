"""Random horizontal flips fused into the decode's store vs the same batch
without flips followed by a flip pass in torch, GPU.

  python tools/flips_bench.py [steps] [--workload scaled|fullres] [--json out.json]

scaled (default): the 256 bench images (480x640 q90 4:2:0) resident in HBM,
stretched to 224x224, as rgb24 u8 [N, 224, 224, 3] and as fp16 normalised NCHW
[N, 3, 224, 224].  Half of the images are flipped, a new seeded draw for every
step.  "fused": the flips go with the submission (spdl_hj_set_flips).
"torch": the submission without flips, then ``torch.where(mask, x.flip(w), x)``
on the same stream -- a read and a write of every output byte.  One lane, so
both legs are stream-ordered on the caller's stream; two batches in flight.

fullres: the same images at full resolution, rgb24 u8, without flips (the fused
IDCT + converter kernel) and with half of them flipped (the generic output
kernel, which a flipped full-resolution batch is routed to).

Prints one JSON line.  The first images of the last fused batch are checked
against the flipped oracle.
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

N, W, H = 256, 640, 480
FIT = dict(resize=True, fit_w=224, fit_h=224)
SUBMISSIONS = {
    "rgb24_u8": (Output(pix_fmt="rgb24", **FIT), (N, 224, 224, 3), torch.uint8, 2),
    "nchw_f16": (Output(pix_fmt="rgb", normalize=True, norm_dtype="float16", **FIT),
                 (N, 3, 224, 224), torch.float16, 3),
    "fullres_rgb24_u8": (Output(pix_fmt="rgb24"), (N, H, W, 3), torch.uint8, 2),
}


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


def leg(packed, name, mode, masks, steps, warmup):
    """mode: "none" (no flips), "fused" (flips with the submission) or "torch"
    (no flips, then the flip pass).  masks: per-step uint8 arrays of N flips."""
    out, shape, dtype, wdim = SUBMISSIONS[name]
    dev, offs, sizes, infos = packed
    dec = _lib.Decoder(0)
    dec.set_param("lanes", 1)
    inflight = 2
    bufs = [torch.empty(shape, dtype=dtype, device="cuda:0") for _ in range(inflight + 1)]
    flipped = [torch.empty_like(b) for b in bufs] if mode == "torch" else None
    dmasks = [torch.from_numpy(m.astype(bool)).to("cuda:0").view(N, 1, 1, 1) for m in masks]
    raw = [bytes(m) for m in masks]
    stream = torch.cuda.current_stream()
    k = [0]

    def submit():
        i = k[0] % len(bufs)
        if mode == "fused":
            dec.set_flips(raw[k[0] % len(raw)])
        dec.decode_batch_device(dev.data_ptr(), dev.numel(), offs, sizes, infos, out,
                                bufs[i].data_ptr(), bufs[i].numel() * bufs[i].element_size(),
                                stream=stream, sync=False)
        t = dec.last_ticket()
        if mode == "torch":
            torch.where(dmasks[k[0] % len(dmasks)], bufs[i].flip(wdim), bufs[i], out=flipped[i])
        k[0] += 1
        return t

    def run(n):
        pend = []
        for _ in range(n):
            pend.append(submit())
            if len(pend) > inflight - 1:
                assert not any(dec.wait(pend.pop(0), N))
        for t in pend:
            assert not any(dec.wait(t, N))

    run(warmup)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run(steps)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    last_k = k[0] - 1
    res = (flipped if mode == "torch" else bufs)[last_k % len(bufs)][:2].cpu()
    dec.close()
    return {"img_per_s": round(N * steps / dt, 1), "ms_per_batch": round(dt / steps * 1e3, 4)}, \
        res, last_k


def check(datas, name, got, flips):
    """The first images of a batch against the oracle, flipped along the width."""
    from oracle import oracle as O

    out, _, _, wdim = SUBMISSIONS[name]
    for i in range(got.shape[0]):
        if out.resize:
            want = O.decode_resize(datas[i], O.Resize(fit_w=224, fit_h=224), pix_fmt=out.pix_fmt,
                                   normalize=out.normalize)
        else:
            want = O.decode_rgb(datas[i], O.IDCT_SIMPLE, out.pix_fmt)
        if flips[i]:
            want = np.flip(want, wdim - 1)
        g = got[i].numpy()
        np.testing.assert_array_equal(g.view(np.uint16) if out.normalize else g,
                                      want.view(np.uint16) if out.normalize else want)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("steps", nargs="?", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--workload", choices=("scaled", "fullres"), default="scaled")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    datas = synthetic_slice(range(N))
    packed = pack(datas)
    rng = np.random.default_rng(a.seed)
    masks = []
    for _ in range(a.steps + a.warmup):  # exactly half of the images, a new draw per step
        m = np.zeros(N, np.uint8)
        m[rng.permutation(N)[: N // 2]] = _lib.FLIP_H
        masks.append(m)
    res = {"workload": a.workload, "images": N, "flipped_per_batch": N // 2, "lanes": 1,
           "steps": a.steps}
    if a.workload == "scaled":
        for name in ("rgb24_u8", "nchw_f16"):
            fused, got, last_k = leg(packed, name, "fused", masks, a.steps, a.warmup)
            check(datas, name, got, masks[last_k % len(masks)])
            plain, _, _ = leg(packed, name, "none", masks, a.steps, a.warmup)
            via_torch, got, last_k = leg(packed, name, "torch", masks, a.steps, a.warmup)
            check(datas, name, got, masks[last_k % len(masks)])
            res[name] = {"no_flips": plain, "fused": fused, "decode_then_torch_flip": via_torch,
                         "fused_over_torch": round(fused["img_per_s"] / via_torch["img_per_s"], 3),
                         "fused_over_no_flips": round(fused["img_per_s"] / plain["img_per_s"], 3)}
    else:
        name = "fullres_rgb24_u8"
        plain, got, _ = leg(packed, name, "none", masks, a.steps, a.warmup)
        check(datas, name, got, np.zeros(N, np.uint8))
        fused, got, last_k = leg(packed, name, "fused", masks, a.steps, a.warmup)
        check(datas, name, got, masks[last_k % len(masks)])
        res[name] = {"no_flips_fused_kernel": plain, "flips_generic_kernel": fused,
                     "flips_over_no_flips": round(fused["img_per_s"] / plain["img_per_s"], 3)}
    res["checked"] = "2 images of each checked batch bit-exact vs the oracle, flipped"
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
