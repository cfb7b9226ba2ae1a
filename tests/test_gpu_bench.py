"""bench.py end to end on the device: a plain run times the headline only and --dump-outputs writes what the timed
LinearBin step returned; --full adds the side legs back."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
SHAPE = ("--batch", "256", "--in-features", "512", "--out-features", "384")
FULL_ONLY = ("c2_ops_level", "c2_layer_forward", "reference_ops_on_gpu", "alexnet", "extra", "cpu_baseline", "detail")


def _bench(*flags):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *SHAPE, *flags], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [json.loads(ln) for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return lines[0]


def test_plain_run_is_the_headline_and_dumps_its_output(tmp_path, oracle):
    r = _bench("--steps", "7", "--warmup", "2", "--dump-outputs", str(tmp_path))
    assert r["steps"] == 7 and r["warmup"] == 2 and r["ms_per_step"] > 0 and r["value"] > 0
    assert not [k for k in FULL_ONLY if k in r], r.keys()
    assert "kernel" not in r["roofline"] and "step_hbm" in r["roofline"]
    # the inputs bench.py draws (seeded generator on the device), and the exact +-1 product the timed layer must return
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(0x5EED)
    x = torch.randn((256, 512), device=dev, generator=gen).sign_()
    x[x == 0] = 1
    w = torch.randn((384, 512), device=dev, generator=gen) * (1.0 / 512) ** 0.5
    want = x.cpu().double().numpy() @ oracle.safe_sign(w.cpu().numpy()).astype(np.float64).T
    y = np.load(tmp_path / "y.npy")
    assert y.dtype == np.float32 and y.shape == (256, 384)
    assert np.array_equal(y, want.astype(np.float32))


def test_full_run_adds_the_side_legs():
    r = _bench("--steps", "5", "--warmup", "2", "--full", "--no-extras", "--alexnet-batch", "0", "--no-cpu-baseline")
    assert r["c2_ops_level"]["same_result_as_headline"] is True
    assert r["c2_layer_forward"]["same_result_as_ops_level_step"] is True
    assert "kernel" in r["roofline"] and "detail" in r
