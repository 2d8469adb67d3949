"""ms per synchronous batch of 64 progressive 480x640 q90 JPEGs (pad224 chain),
for an A/B of two builds: python tools/prog_sync_ms.py LABEL, with SPDL_AMD_LIB
naming the other build's library (profiles/r09/multiscan_overlap/ab.txt)."""
import sys, time
import numpy as np
import torch
sys.path.insert(0, ".")
from spdl_amd import _lib
from spdl_amd._lib import Output
from spdl_amd.synthetic import synthetic_jpeg

n, reps = 64, 40
spec = Output(pix_fmt="rgb24", resize=True, fit_w=224, fit_h=224, aspect="decrease", pad_w=224, pad_h=224)
dec = _lib.Decoder(0)
out = torch.empty((n, 224, 224, 3), dtype=torch.uint8, device="cuda:0")
datas = [synthetic_jpeg(2000 + i % 8, progressive=True) for i in range(n)]
for _ in range(5):
    dec.decode_batch(datas, spec, out.data_ptr(), out.numel())
torch.cuda.synchronize()
ts = []
for _ in range(reps):
    t0 = time.perf_counter()
    dec.decode_batch(datas, spec, out.data_ptr(), out.numel())
    torch.cuda.synchronize()
    ts.append((time.perf_counter() - t0) * 1e3)
dec.close()
ts = np.array(ts)
print(f"{sys.argv[1]} lib={_lib.LIB_PATH} ms/batch median {np.median(ts):.3f} min {ts.min():.3f} "
      f"p90 {np.percentile(ts, 90):.3f} sum {int(out.sum().item())}", flush=True)
