#!/usr/bin/env python
"""Half-precision sign layers on the GPU: one JSON line.

  * the C2 step, LinearBin(4096, 4096).train().forward(x) on a 4096 x 4096 +-1 activation with binary_input=True, in
    (a) fp32 — the route bench.py's headline measures, the anchor of this run —, (b) bf16 and (c) fp16;
  * one BinaryNet-AlexNet-shaped conv forward (conv2: 192 -> 576, 5 x 5, padding 2, 27 x 27, batch 256) in fp32 and bf16.

Per case: median and spread (min, max, inter-quartile range) of >= 50 event-timed iterations after a warm-up, the C-ABI entry
points that ran, how many dense-library detours were counted, and the bytes the step has to move (2 or 4 bytes per element of
x, W and y).  The tool uses only what every commit of this repository has (the layers, ``binary_input``, the counters), so the
SAME file runs on a commit without the half routes — there the half cases take the counted torch expression — and

    python tools/bench_half.py --parent-line <that run's JSON line>

stores that line under "parent" of this run's.  Clocks are not touched.

    python tools/bench_half.py [--iters 100] [--out profiles/half_bench_line.json]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")))
from pytorch_quantize_impls_amd import _lib, synth  # noqa: E402
from pytorch_quantize_impls_amd.functions import _fused  # noqa: E402
from pytorch_quantize_impls_amd.layers import BinConv2d, LinearBin  # noqa: E402

DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    times.sort()
    n = len(times)
    return {"us_median": round(times[n // 2], 2), "us_min": round(times[0], 2), "us_max": round(times[-1], 2),
            "us_iqr": round(times[(3 * n) // 4] - times[n // 4], 2), "iters": n}


def run_case(make_layer, x, iters, warmup):
    layer = make_layer()
    layer.binary_input = True
    layer.train()
    before, lib_before = dict(_lib.call_counts), sum(_fused.LIBRARY_PATHS.values())
    with torch.no_grad():
        y = layer(x)
        res = timed(lambda: layer(x), iters, warmup)
    torch.cuda.synchronize()
    calls = {k: _lib.call_counts[k] - before.get(k, 0) for k in _lib.call_counts if _lib.call_counts[k] != before.get(k, 0)}
    per_call = iters + warmup + 1
    res["entry_points_per_forward"] = {k: round(v / per_call, 2) for k, v in sorted(calls.items())}
    res["library_paths_per_forward"] = round((sum(_fused.LIBRARY_PATHS.values()) - lib_before) / per_call, 2)
    res["out_dtype"] = str(y.dtype).replace("torch.", "")
    esz = x.element_size()
    res["algorithmic_MB"] = round(esz * (x.numel() + layer.weight.numel() + y.numel()) / 1e6, 1)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--only", default="", help="comma-separated case names (for profiler runs)")
    ap.add_argument("--out", default="")
    ap.add_argument("--parent-line", default="", help="JSON line of the same tool run on the parent commit")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_half.py measures on the GPU: there is no fallback"
    dev = torch.device("cuda:0")
    name, cus = _lib.device_info()
    res = {"what": "sign layers, half-precision activations", "device": name, "CUs": cus, "libqt_hip": _lib.version(), "cases": {}}
    only = {s for s in args.only.split(",") if s}
    x2 = torch.from_numpy(synth.pm1(0xB001, (4096, 4096))).to(dev)
    w2 = torch.from_numpy(synth.uniform(0xB002, (4096, 4096), -1.0, 1.0)).to(dev)
    xc = torch.from_numpy(synth.pm1(0xB003, (256, 192, 27, 27))).to(dev).contiguous(memory_format=torch.channels_last)
    wc = torch.from_numpy(synth.uniform(0xB004, (576, 192, 5, 5), -1.0, 1.0)).to(dev)

    def linear(dt):
        def make():
            lay = LinearBin(4096, 4096).to(dev)
            lay.weight.data.copy_(w2)
            return lay.to(dt)
        return make

    def conv(dt):
        def make():
            lay = BinConv2d(192, 576, 5, padding=2).to(dev)
            lay.weight.data.copy_(wc)
            return lay.to(dt).to(memory_format=torch.channels_last)
        return make

    for label, dt in DTYPES.items():
        if not only or f"c2_{label}" in only:
            res["cases"][f"c2_{label}"] = run_case(linear(dt), x2.to(dt), args.iters, args.warmup)
    for label in ("fp32", "bf16"):
        if not only or f"conv2_b256_{label}" in only:
            res["cases"][f"conv2_b256_{label}"] = run_case(conv(DTYPES[label]), xc.to(DTYPES[label]), max(50, args.iters // 2), args.warmup)
    if args.parent_line:
        with open(args.parent_line) as fh:
            res["parent"] = json.loads(fh.read().strip().splitlines()[-1])
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
