#!/usr/bin/env python
"""The depthwise 3 x 3 layers of MobileNet-v1 at batch 256 as BinConv2d(C, C, 3, stride, padding=1, groups=C) on one GPU: one JSON line.

Three ways of running each layer, forward and forward + backward, on +-1 activations:
  new   : the layer as it is — DepthwiseConv2dFn, one streaming launch forward and two calls backward (csrc/dwconv.hip);
  loop  : the route before the depthwise kernels, ``_fused.grouped_quant_conv`` called directly (one fp4 implicit-GEMM conv per
          channel, told that the activation is +-1 so that it does not stop to detect it); channel counts up to 128 only — it is slow;
  torch : what a user would write without this backend, F.conv2d(x, sign(W), b, groups=C) through torch (MIOpen).

Method: every shape runs in a child process of its own under a time limit, and nothing more is started after a child that fails
or overruns.  Inside a child the routes take turns within each of ``--rounds`` rounds; a round times ``steps`` calls with the host
clock around a run that ends in a device synchronise.  Reported per route: the median round and the range of the rounds.  ``bytes``
is what the algorithm has to move (fp32: x and y once forward; x, y, grad_x and grad_y three times in all forward + backward; the
weights are noise), ``roofline`` = (bytes / 8 TB/s) / median time of the new route.

    python tools/bench_depthwise.py [--rounds 9] [--out profiles/depthwise_bench_line.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
os.environ.setdefault("QT_AUTO_GRAPH", "0")

BATCH = 256
#: (channels, map, stride) of the depthwise layers of MobileNet-v1 at 224 x 224
SHAPES = [(32, 112, 1), (64, 112, 2), (128, 56, 1), (256, 28, 1), (512, 14, 1), (1024, 7, 1)]
LOOP_MAX_CHANNELS = 128
HBM_BYTES_PER_S = 8e12
CHILD_LIMIT_S = 420


def algorithmic_bytes(C, H, stride):
    Ho = (H + 2 - 3) // stride + 1
    x, y = 4 * BATCH * C * H * H, 4 * BATCH * C * Ho * Ho
    return {"fwd": x + y, "fwd_bwd": 3 * (x + y)}


def child(index, rounds):
    import torch
    import torch.nn.functional as F
    from pytorch_quantize_impls_amd import _lib
    from pytorch_quantize_impls_amd.functions import _fused
    from pytorch_quantize_impls_amd.layers import BinConv2d

    C, H, stride = SHAPES[index]
    dev = torch.device("cuda:0")
    torch.manual_seed(index)
    g = torch.Generator().manual_seed(index)
    layer = BinConv2d(C, C, 3, stride=stride, padding=1, groups=C).to(dev)
    layer.weight.data.uniform_(-1.2, 1.2)
    layer.binary_input = True
    x = torch.where(torch.rand(BATCH, C, H, H, generator=g) < 0.5, -1.0, 1.0).to(dev)
    xg = x.clone().requires_grad_(True)
    with torch.no_grad():
        y0 = layer(x)
    go = torch.randn(y0.shape, generator=g).to(dev)

    def new_fwd():
        with torch.no_grad():
            return layer(x)

    def new_fb():
        layer(xg).backward(go)

    def loop_fwd():
        with torch.no_grad():
            return _fused.grouped_quant_conv(layer, x, "binary", layer._op)

    def loop_fb():
        _fused.grouped_quant_conv(layer, xg, "binary", layer._op).backward(go)

    def torch_fwd():
        with torch.no_grad():
            return F.conv2d(x, torch.where(layer.weight < 0, -1.0, 1.0), layer.bias, stride, 1, 1, C)

    def torch_fb():
        wq = torch.where(layer.weight.detach() < 0, -1.0, 1.0).requires_grad_(True)
        F.conv2d(xg, wq, layer.bias, stride, 1, 1, C).backward(go)

    fns = {"fwd": {"new": new_fwd, "torch": torch_fwd}, "fwd_bwd": {"new": new_fb, "torch": torch_fb}}
    if C <= LOOP_MAX_CHANNELS:
        fns["fwd"]["loop"], fns["fwd_bwd"]["loop"] = loop_fwd, loop_fb
    # the three routes compute the same conv: integer sums plus the bias (the library's algorithm is its own choice)
    assert torch.allclose(new_fwd(), torch_fwd(), rtol=0, atol=1e-4)
    if C <= LOOP_MAX_CHANNELS:
        assert torch.equal(new_fwd(), loop_fwd())
    calls = dict(_lib.call_counts)
    new_fb()
    used = {k: v - calls.get(k, 0) for k, v in _lib.call_counts.items() if v != calls.get(k, 0)}
    assert used == {"qt_dwconv2d_f32": 1, "qt_dwconv2d_grad_input_f32": 1, "qt_dwconv2d_grad_weight_f32": 1}, used

    def run_us(fn, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6 / steps

    result = {"channels": C, "map": H, "stride": stride, "bytes": algorithmic_bytes(C, H, stride)}
    for mode, routes in fns.items():
        steps = {k: (2 if k == "loop" else 20) for k in routes}
        for k, fn in routes.items():
            for _ in range(2):
                fn()
                xg.grad = None
        samples = {k: [] for k in routes}
        for _ in range(rounds):
            for k, fn in routes.items():
                samples[k].append(run_us(fn, steps[k]))
                xg.grad = None
                layer.zero_grad(set_to_none=True)
        result[mode] = {k: {"median_us": round(sorted(v)[len(v) // 2], 1), "min_us": round(min(v), 1), "max_us": round(max(v), 1)}
                        for k, v in samples.items()}
        t = result[mode]["new"]["median_us"] * 1e-6
        result[mode]["new"]["roofline"] = round(result["bytes"][mode] / HBM_BYTES_PER_S / t, 3)
    print(json.dumps(result))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depthwise_bench_line.json"))
    ap.add_argument("--child", type=int, default=None)
    a = ap.parse_args()
    if a.child is not None:
        return child(a.child, a.rounds)
    shapes = []
    for i in range(len(SHAPES)):
        # a child per shape, each under its own limit; the first failure ends the run
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(i), "--rounds", str(a.rounds)],
                           stdout=subprocess.PIPE, text=True, timeout=CHILD_LIMIT_S)
        if p.returncode != 0:
            raise SystemExit(f"shape {SHAPES[i]}: the measuring process ended with status {p.returncode}; nothing more was started")
        shapes.append(json.loads(p.stdout.strip().splitlines()[-1]))
        print(json.dumps(shapes[-1]), file=sys.stderr)
    faster = all(s[mode]["new"]["max_us"] < s[mode]["loop"]["min_us"] for s in shapes for mode in ("fwd", "fwd_bwd") if "loop" in s[mode])
    line = {"bench": "depthwise_mobilenet_v1", "batch": BATCH, "rounds": a.rounds, "kernel": "3x3 pad 1", "dtype": "float32",
            "layout": "NCHW", "hbm_bytes_per_s": HBM_BYTES_PER_S, "shapes": shapes,
            "new_faster_than_loop_with_disjoint_ranges": faster}
    text = json.dumps(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text + "\n")
    print(text)
    if not faster:
        raise SystemExit("acceptance: the new route is not faster than the per-group loop with disjoint round ranges at every shape")


if __name__ == "__main__":
    main()
