"""bench.py's plain run and --dump-outputs.

CPU: `_dump_outputs` writes a small batch whole and a large one as a fixed,
seeded sample (float32, under 64 MB, the same elements every time).
GPU: a plain `bench.py --dump-outputs` run prints the headline fields only,
times exactly --steps steps, and the dumped batch is the oracle's pixels.
"""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD224 = dict(fit_w=224, fit_h=224, aspect="decrease", pad_w=224, pad_h=224)


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_small_batch_whole(bench, tmp_path):
    import torch

    out = torch.arange(2 * 5 * 7 * 3, dtype=torch.int32).remainder(256).to(torch.uint8)
    out = out.reshape(2, 5, 7, 3)
    info = bench._dump_outputs(str(tmp_path / "d"), out)
    arr = np.load(tmp_path / "d" / "output.npy")
    assert arr.dtype == np.float32 and not info["sampled"]
    np.testing.assert_array_equal(arr, out.numpy().astype(np.float32), strict=True)


def test_dump_large_batch_seeded_sample(bench, tmp_path):
    import torch

    n = bench.DUMP_MAX_ELEMS + 12345
    out = torch.arange(n, dtype=torch.int64).remainder(251).to(torch.uint8)
    a = bench._dump_outputs(str(tmp_path / "a"), out)
    b = bench._dump_outputs(str(tmp_path / "b"), out)
    x, y = np.load(tmp_path / "a" / "output.npy"), np.load(tmp_path / "b" / "output.npy")
    assert a == b and a["sampled"] and a["of_elements"] == n
    assert x.dtype == np.float32 and x.ndim == 1 and 0 < x.nbytes <= 64 * 1024 * 1024
    np.testing.assert_array_equal(x, y, strict=True)
    idx = np.unique(np.random.default_rng(bench.DUMP_SEED).integers(0, n, size=bench.DUMP_MAX_ELEMS))
    np.testing.assert_array_equal(x, (idx % 251).astype(np.float32), strict=True)


@pytest.mark.gpu
def test_plain_run_headline_only_and_dump_matches_oracle(oracle, tmp_path):
    from spdl_amd.synthetic import synthetic_batch

    d = str(tmp_path / "dump")
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--batch", "8", "--dump-outputs", d], capture_output=True, text=True,
                       timeout=120, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in rec, k
    assert rec["steps"] == 3 and rec["unit"] == "images/sec" and rec["dtype"] == "u8"
    assert rec["value"] == pytest.approx(8 / (rec["ms_per_step"] / 1e3), rel=1e-3)
    for k in ("roofline", "cpu_baseline", "hw_queue_regimes", "stages_ms"):
        assert k not in rec, k
    arr = np.load(os.path.join(d, "output.npy"))
    assert arr.dtype == np.float32 and arr.shape == (8, 224, 224, 3)
    rs = oracle.Resize(**PAD224)
    for i, data in enumerate(synthetic_batch(8, distinct=32)):
        ref = oracle.decode_resize(data, rs, "rgb24")
        np.testing.assert_array_equal(arr[i], ref.astype(np.float32), strict=True)
